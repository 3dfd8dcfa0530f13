"""The EdgePoint fixtures of tests/golden/make_golden_edgepoint.py: the shapes of edgepoint*.npz, the reference checkpoint, and the net restated as a few lines
of torch.nn.functional over the folded tensors, with the closed forms of the head's strided and transposed layers (tests/test_edgepoint_cpu.py checks it
against the goldens)."""
import numpy as np

from r2d2_fixtures import load_parts  # noqa: F401  (stem-generic: load_parts("edgepoint"))

SHAPES = ((32, 32), (32, 64), (64, 96), (96, 160), (480, 640))
PARAM = {"c1": 8, "c2": 16, "c3": 32, "c4": 64, "dim": 64}


def checkpoint():
    """{name: torch tensor} as torch.load of the reference's weights/EdgePoint.pt gives it (without num_batches_tracked)."""
    import torch
    return {k: torch.from_numpy(v) for k, v in load_parts("edgepoint_state_dict").items()}


def chain(t, img):
    """(score [B,1,H,W], desc [B,64,H/8,W/8]) from the folded tensors `t` (weights.fold_edgepoint)."""
    import torch
    import torch.nn.functional as F
    _t = lambda a: torch.from_numpy(np.ascontiguousarray(a))

    def conv3(x, n):
        return F.conv2d(x, _t(t[n + ".w"]), _t(t[n + ".b"]), padding=1)

    def res(x, q):
        y = conv3(F.relu(conv3(x, q + "c1")), q + "c2")
        return F.relu(y + F.conv2d(x, _t(t[q + "ds.w"])[:, :, None, None], _t(t[q + "ds.b"])))

    def agg(x, i):
        return F.relu(F.conv2d(x, _t(t["agg%d.w" % i])[:, :, None, None]))

    x1 = F.relu(conv3(F.relu(conv3(img, "b1c1")), "b1c2"))
    x2 = res(F.max_pool2d(x1, 2, 2), "b2")
    x3 = res(F.max_pool2d(x2, 4, 4), "b3")
    x4 = res(F.max_pool2d(x3, 4, 4), "b4")
    a1, a2, a3, a4 = agg(x1, 1), agg(x2, 2), agg(x3, 3), agg(x4, 4)
    score = F.conv2d(a1, _t(t["score.w"])[None, :, None, None], _t(t["score.b"]))
    d1 = F.conv2d(a1[..., ::8, ::8], _t(t["d8.w"])[:, :, None, None], _t(t["d8.b"]))
    d2 = F.conv2d(a2[..., ::4, ::4], _t(t["d4.w"])[:, :, None, None], _t(t["d4.b"]))
    up = a4.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)                 # a4[y // 4, x // 4]
    Hc, Wc = up.shape[2:]
    wct = _t(t["ct4.w"])                                                            # [ci][co][ky][kx]
    wyx = wct[:, :, torch.arange(Hc) % 4][:, :, :, torch.arange(Wc) % 4]            # [ci][co][Hc][Wc]: the slice (y % 4, x % 4) at every pixel
    d4 = torch.einsum("bihw,iohw->bohw", up, wyx) + _t(t["ct4.b"])[None, :, None, None]
    desc = F.conv2d(torch.cat([d1, d2, a3, d4], dim=1), _t(t["head.w"])[:, :, None, None])
    return score, desc
