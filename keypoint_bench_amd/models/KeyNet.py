"""Drop-in for the reference's models/KeyNet.py: ``KeyNet(keynet_conf)`` with ``load_state_dict`` / ``eval`` / ``__call__(image) -> (score [B,1,H,W], None)``
(KeyNet.py:116-132), computed by csrc/keynet.hip through libkpb.so: the gray sum, two 1.2 x pyramid steps, per level the ten handcrafted gradient features and
three 5 x 5 layers (BatchNorm folded), and the 24 -> 1 fusion layer over the bilinearly upsampled levels.  The score is non-negative and UNBOUNDED (28 to
14 400 on the synthetic 480 x 640 fixture), there are no descriptors (``dim = 0``): the net feeds detection, the repeatability task and the Lucas-Kanade
tracker on the frames; anything that matches descriptors refuses it.  Any H, W >= 16."""
from .. import weights as _weights
from ._base import HipNet


class KeyNet(HipNet):
    ARCH = _weights.ARCH_KEYNET
    dense_descriptors = False

    def __init__(self, keynet_conf=None):
        conf = dict(_weights.KEYNET_PLAN if keynet_conf is None else keynet_conf)
        self.param = {k: conf.get(k) for k in _weights.KEYNET_PLAN}
        if self.param != _weights.KEYNET_PLAN:
            raise NotImplementedError("this build carries kernels for KeyNet with num_filters = 8, num_levels = 3, kernel_size = 5 only; got %r" % (self.param,))
        super().__init__()
        self.dim, self.desc_div = 0, 1

    def load_state_dict(self, state_dict, strict=True):
        self.load_packed(_weights.pack(_weights.fold_keynet(state_dict), _weights.ARCH_KEYNET))
        return "<All keys matched successfully>"

    def forward(self, image):
        score, _ = self._run(image, want_desc=False)
        return score, None

    __call__ = forward
