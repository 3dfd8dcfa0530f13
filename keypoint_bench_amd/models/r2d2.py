"""Drop-in for the reference's models/r2d2.py: ``Quad_L2Net_ConfCFS()`` with ``load_state_dict`` / ``eval`` /
``__call__(image) -> (score [B,1,H,W], desc [B,128,H,W])`` (r2d2.py:132-141), computed by csrc/r2d2.hip through libkpb.so.
The descriptor map is stored channels-last.  Any H and W: every layer runs at full resolution."""
from .. import weights as _weights
from .._lib import KpbError
from ._base import HipNet

OTHER_VARIANTS = ("L2_Net", "Quad_L2Net", "Fast_Quad_L2Net", "Fast_Quad_L2Net_ConfCFS")
KPB_E_UNSUPPORTED = -7


class Quad_L2Net_ConfCFS(HipNet):
    """matrix: "split" (default) = every product of conv1 .. conv8 as a split-f16 MFMA triple, the reference's fp32 CPU outputs to a few 1e-6;
    "f16" = one MFMA per product on operands rounded to f16, fp32 accumulation -- TF32-class, what the reference's convolutions are on its own GPU
    (score / descriptor errors of the order 1e-3).  The mode is packed into the blob (tensor matrix.mode) and fixed for the life of the net."""
    ARCH = _weights.ARCH_R2D2

    def __init__(self, matrix="split", **kw):
        _weights.matrix_mode(matrix)        # ValueError for anything but the two names
        if kw:
            raise NotImplementedError("this build carries kernels for the default Quad_L2Net_ConfCFS() (dim=128, mchan=4, dilated, BatchNorm without affine); got %r" % (kw,))
        super().__init__()
        self.matrix = matrix

    def load_state_dict(self, state_dict, strict=True):
        self.load_packed(_weights.pack(_weights.with_matrix_mode(_weights.fold_r2d2(state_dict), self.matrix), _weights.ARCH_R2D2))
        return "<All keys matched successfully>"

    def _create(self, ctx):
        try:
            return super()._create(ctx)
        except KpbError as e:       # matrix="f16" under KPB_FP32_MATRIX=1: a documented limit of the build, as the constructor's other refusals
            if e.code == KPB_E_UNSUPPORTED:
                raise NotImplementedError(str(e)) from e
            raise


def from_checkpoint(checkpoint, matrix="split") -> Quad_L2Net_ConfCFS:
    """The net of a reference checkpoint dict {'net': <constructor string>, 'state_dict': ...} (weights/r2d2_WASF_N16.pt).  The reference
    evaluates the string (model_interface.py:70); here it must name the one variant with kernels.  `matrix`: see Quad_L2Net_ConfCFS."""
    _weights.matrix_mode(matrix)
    name = checkpoint.get("net") if hasattr(checkpoint, "get") else None
    if name != _weights.R2D2_NET:
        raise NotImplementedError("R2D2 checkpoint net %r: only %s has MI355X kernels in this build (not %s)"
                                  % (name, _weights.R2D2_NET, ", ".join(OTHER_VARIANTS)))
    net = Quad_L2Net_ConfCFS(matrix=matrix)
    net.load_state_dict(checkpoint["state_dict"])
    return net.eval()
