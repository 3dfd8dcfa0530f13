"""Drop-in for the reference's models/GoodPoint.py: ``GoodPoint(params)`` with ``load_state_dict`` / ``eval`` /
``__call__(image) -> (score [B,1,H,W], desc [B,3,H,W])`` (GoodPoint.py:84-111), computed by csrc/alike.hip through libkpb.so: ALIKE-t's block 1
(the reference's ConvBlock(3, 8) is the same class), then a 3 x 3 sigmoid score head and a 1 x 1 sigmoid head of three channels, both at full
resolution.  The 3-channel map is stored channels-last (the returned tensor is a [B,3,H,W] view of it), is NOT normalised, and is what the
Lucas-Kanade tracker follows in place of the frames (model_interface.py:262-272): ``tracked_maps`` says so.  H and W must be multiples of 32."""
from .. import weights as _weights
from ._base import HipNet


class GoodPoint(HipNet):
    ARCH = _weights.ARCH_GOODPOINT
    tracked_maps = True

    def __init__(self, params):
        self.param = {k: params[k] for k in ("c0", "c1")}
        if self.param != _weights.GOODPOINT_PLAN:
            raise NotImplementedError("this build carries kernels for GoodPoint with c0 = 3, c1 = 8 (GoodPoint_params of the configs) only; got %r" % (self.param,))
        super().__init__()
        self.dim, self.desc_div = 3, 1

    def load_state_dict(self, state_dict, strict=True):
        self.load_packed(_weights.pack(_weights.fold_goodpoint(state_dict), _weights.ARCH_GOODPOINT))
        return "<All keys matched successfully>"
