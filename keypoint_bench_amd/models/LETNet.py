"""Drop-in for the reference's models/LETNet.py: ``LETNet(c1=8, c2=16, grayscale=False)`` (the call of model_interface.py:57) with ``load_state_dict`` /
``eval`` / ``__call__(image) -> (score [B,1,H,W], desc [B,3,H,W])`` (LETNet.py:44-52), computed by csrc/alike.hip through libkpb.so: ALIKE-t's block 1 as
every net built on it runs it (the reference's ConvBlock(3, 8) is the same class), then the letnet_head kernel -- two 1 x 1 convolutions, 8 -> 16 -> 4, whose
sigmoids are the 3-channel map (channels 0..2) and the score (channel 3).  The map is stored channels-last (the returned tensor is a [B,3,H,W] view of it), is
NOT normalised, and is what the Lucas-Kanade tracker follows in place of the frames (model_interface.py:233, 263, 285): ``tracked_maps`` says so.
H and W must be multiples of 32."""
from .. import weights as _weights
from ._base import HipNet


class LETNet(HipNet):
    ARCH = _weights.ARCH_LETNET
    tracked_maps = True

    def __init__(self, c1: int = 8, c2: int = 16, grayscale: bool = False):
        self.param = dict(c1=c1, c2=c2, grayscale=bool(grayscale))
        if self.param != _weights.LETNET_PLAN:
            raise NotImplementedError("this build carries kernels for LETNet with c1 = 8, c2 = 16, grayscale = False (model_interface.py:57) only; got %r" % (self.param,))
        super().__init__()
        self.dim, self.desc_div = 3, 1

    def load_state_dict(self, state_dict, strict=True):
        self.load_packed(_weights.pack(_weights.fold_letnet(state_dict), _weights.ARCH_LETNET))
        return "<All keys matched successfully>"
