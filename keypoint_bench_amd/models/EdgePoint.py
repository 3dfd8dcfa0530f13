"""Drop-in for the reference's models/EdgePoint.py: ``EdgePoint(param)`` with ``load_state_dict`` / ``eval`` /
``__call__(image) -> (score [B,1,H,W], desc [B,64,H/8,W/8])`` (EdgePoint.py:144-175), computed by csrc/alike.hip through libkpb.so:
ALIKE-t's trunk, then a 1 x 1 score head on block 1's features and a 64 x 64 descriptor head at 1/8 scale.
The score is a RAW LOGIT (no sigmoid; four pixels in five are negative): detect on it with ``detection(score, params, signed=True)``,
as the pipelines and the runner do for a net with ``signed_scores``.  The descriptor map is stored channels-last and is NOT normalised
(model_interface.py:206 calls the model, not extract_dense_map).  H and W must be multiples of 32."""
from .. import weights as _weights
from ._base import HipNet


class EdgePoint(HipNet):
    ARCH = _weights.ARCH_EDGEPOINT
    signed_scores = True

    def __init__(self, param=None, trainable=False):
        if param is None:
            param = dict(c1=32, c2=64, c3=128, c4=128, dim=128)     # EdgePoint.py:87-92
        self.param = {k: param[k] for k in ("c1", "c2", "c3", "c4", "dim")}
        if self.param != _weights.EDGEPOINT_PLAN:
            raise NotImplementedError("this build carries kernels for EdgePoint with c1..c4 = 8,16,32,64, dim = 64 (EdgePoint_params of the configs) only; got %r" % (self.param,))
        if trainable:
            raise NotImplementedError("EdgePoint(trainable=True): inference only (the 65-channel training heatmap of extract_dense_map is not built)")
        super().__init__()
        self.trainable = False
        self.dim, self.desc_div = self.param["dim"], 8

    def load_state_dict(self, state_dict, strict=True):
        self.load_packed(_weights.pack(_weights.fold_edgepoint(state_dict), _weights.ARCH_EDGEPOINT))
        return "<All keys matched successfully>"
