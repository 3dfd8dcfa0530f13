"""Drop-in for the reference's models/ALike.py: ``ALNet(param)`` with ``load_state_dict`` / ``eval`` /
``__call__(image) -> (scores_map, descriptor_map)``, computed by csrc/alike.hip through libkpb.so.
No torch.nn forward runs: tensors are containers for the image, the weights and the two outputs.

    net = ALNet({'c1': 8, 'c2': 16, 'c3': 32, 'c4': 64, 'dim': 64})      # Alike_params of the YAML configs (ALIKE-t); ALNet() is ALIKE-l, 32/64/128/128/128
    net.load_state_dict(torch.load('weights/alike-t.pth'))               # model_interface.py:43-45
    score_map, desc_map = net.eval()(img)                                # model_interface.py:205-212

``descriptor_map`` is the reference's [B, dim, H, W] tensor stored channels-last (a valid torch
memory format; ``.shape[2:4]``, ``.detach()`` and ``grid_sample`` all behave).  With
``dense_descriptors=False`` the dense map (78.6 MB/image for ALIKE-t, twice that for ALIKE-l) is not materialised: a ``LazyDescriptors``
handle is returned instead, which ``brute_force_matcher`` samples at the keypoints (same values: the
1x1 head and the bilinear sampling are both linear).
"""
from .. import weights as _weights
from ._base import KeypointOnlyNet, LazyDescriptors      # noqa: F401 -- LazyDescriptors lived here first and stays importable from here


PLANS = ((8, 16, 32, 64, 64), (32, 64, 128, 128, 128))      # (c1, c2, c3, c4, dim): ALIKE-t (csrc/alike.hip) and ALIKE-l, the reference's default (csrc/alike_l.hip)


class ALNet(KeypointOnlyNet):
    """models/ALike.py:84-164.  The native side reads the plan from the weights' shapes; ALIKE-l has no packaged checkpoint (the reference ships none):
    ``ALNet()`` needs ``load_state_dict``, as the reference's does."""

    ARCH = _weights.ARCH_ALIKE

    def __init__(self, param=None, dense_descriptors=True):
        if param is None:
            param = dict(c1=32, c2=64, c3=128, c4=128, dim=128)   # ALike.py:87-92
        self.param = dict(c1=param["c1"], c2=param["c2"], c3=param["c3"], c4=param["c4"], dim=param["dim"])
        if tuple(self.param[k] for k in ("c1", "c2", "c3", "c4", "dim")) not in PLANS:
            raise NotImplementedError("this build carries kernels for ALIKE-t (c1..c4 = 8,16,32,64, dim = 64) and "
                                      "ALIKE-l (c1..c4 = 32,64,128,128, dim = 128, the default) only")
        super().__init__(dense_descriptors)
        self.dim, self.desc_div = self.param["dim"], 1

    def load_state_dict(self, state_dict, strict=True):
        t = _weights.fold_alike(state_dict)
        want = {"b1c1.w": (self.param["c1"], 3, 3, 3), "b2c1.w": (self.param["c2"], self.param["c1"], 3, 3), "b3c1.w": (self.param["c3"], self.param["c2"], 3, 3),
                "b4c1.w": (self.param["c4"], self.param["c3"], 3, 3), "head.w": (self.dim + 1, self.dim)}
        for k, shape in want.items():
            if tuple(t[k].shape) != shape:
                raise ValueError("ALNet.load_state_dict: %s is %s in this state_dict, the plan %s needs %s" % (k, tuple(t[k].shape), self.param, shape))
        self.load_packed(_weights.pack(t, _weights.ARCH_ALIKE))
        return "<All keys matched successfully>"


def packaged_blob() -> bytes:
    """keypoint_bench_amd/weights/alike-t.kpbw: ALIKE-t folded from the reference's weights/alike-t.pth."""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "weights", "alike-t.kpbw")
    with open(path, "rb") as f:
        return f.read()


def alike_t(device=None, dense_descriptors=True) -> "ALNet":
    """ALIKE-t with the weights shipped in keypoint_bench_amd/weights/alike-t.kpbw."""
    net = ALNet(dict(c1=8, c2=16, c3=32, c4=64, dim=64), dense_descriptors=dense_descriptors)
    net.load_packed(packaged_blob())
    return net
