"""Drop-in for the reference's models/sfd2.py: ``ResSegNetV2(outdim=128, require_stability=True)`` with ``load_state_dict`` / ``eval`` /
``__call__(image) -> (score [B,1,H,W], desc [B,128,H/4,W/4])`` (sfd2.py:144-185), computed by csrc/sfd2.hip through libkpb.so: the VGG-like trunk, three
ResBlocks with a grouped 3 x 3 (32 groups of 8 channels), SuperPoint's 65-way cell head without the maximum subtraction, multiplied by the stability factor
0.1 / 0.5 / 1.0 -- the argmax of three logits upsampled x 4 --, and an L2-normalised 128-channel descriptor map at 1/4 resolution, stored channels-last.
H and W must be multiples of 8 (the reference's own score x stability product fails otherwise)."""
from .. import weights as _weights
from ._base import HipNet


class ResSegNetV2(HipNet):
    ARCH = _weights.ARCH_SFD2

    def __init__(self, outdim=128, require_feature=False, require_stability=False, ms_detector=True):
        if outdim != 128:
            raise NotImplementedError("this build carries kernels for ResSegNetV2 with outdim = 128 only; got %r" % (outdim,))
        if not require_stability:       # sfd2.py:180-182: stability = None, then score * None raises
            raise NotImplementedError("ResSegNetV2(require_stability=False): the reference's own forward fails there (score * None); build it with require_stability=True")
        super().__init__()
        self.outdim, self.require_feature, self.require_stability, self.ms_detector = outdim, require_feature, require_stability, ms_detector
        self.dim, self.desc_div = 128, 4

    def load_state_dict(self, state_dict, strict=True):
        """The reference loads checkpoint['model'] with strict=False (sfd2.py:192): keys the forward does not read are ignored under either setting,
        the ones it reads must be there with their shapes (ValueError names the key)."""
        self.load_packed(_weights.pack(_weights.fold_sfd2(state_dict), _weights.ARCH_SFD2))
        return "<All keys matched successfully>"


def sfd2_random(seed=0) -> "ResSegNetV2":
    """SFD2 with seeded random weights (the reference checkpoint weights/sfd2.pth is not in its tree)."""
    net = ResSegNetV2(outdim=128, require_stability=True)
    net.load_state_dict(_weights.random_sfd2_state_dict(seed))
    return net
