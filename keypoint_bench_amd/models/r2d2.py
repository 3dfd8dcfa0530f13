"""Drop-in for the reference's models/r2d2.py: ``Quad_L2Net_ConfCFS()`` with ``load_state_dict`` / ``eval`` /
``__call__(image) -> (score [B,1,H,W], desc [B,128,H,W])`` (r2d2.py:132-141), computed by csrc/r2d2.hip through libkpb.so.
The descriptor map is stored channels-last.  Any H and W: every layer runs at full resolution."""
from .. import weights as _weights
from ._base import HipNet

OTHER_VARIANTS = ("L2_Net", "Quad_L2Net", "Fast_Quad_L2Net", "Fast_Quad_L2Net_ConfCFS")


class Quad_L2Net_ConfCFS(HipNet):
    ARCH = _weights.ARCH_R2D2

    def __init__(self, **kw):
        if kw:
            raise NotImplementedError("this build carries kernels for the default Quad_L2Net_ConfCFS() (dim=128, mchan=4, dilated, BatchNorm without affine); got %r" % (kw,))
        super().__init__()

    def load_state_dict(self, state_dict, strict=True):
        self.load_packed(_weights.pack(_weights.fold_r2d2(state_dict), _weights.ARCH_R2D2))
        return "<All keys matched successfully>"


def from_checkpoint(checkpoint) -> Quad_L2Net_ConfCFS:
    """The net of a reference checkpoint dict {'net': <constructor string>, 'state_dict': ...} (weights/r2d2_WASF_N16.pt).  The reference
    evaluates the string (model_interface.py:70); here it must name the one variant with kernels."""
    name = checkpoint.get("net") if hasattr(checkpoint, "get") else None
    if name != _weights.R2D2_NET:
        raise NotImplementedError("R2D2 checkpoint net %r: only %s has MI355X kernels in this build (not %s)"
                                  % (name, _weights.R2D2_NET, ", ".join(OTHER_VARIANTS)))
    net = Quad_L2Net_ConfCFS()
    net.load_state_dict(checkpoint["state_dict"])
    return net.eval()
