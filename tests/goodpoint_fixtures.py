"""The GoodPoint fixtures of tests/golden/make_golden_goodpoint.py: the shapes of goodpoint*.npz, the reference checkpoint, the tracking chain, and
the net restated as a few lines of torch.nn.functional over the folded tensors (for the test that needs no GPU)."""
import numpy as np

from r2d2_fixtures import load_parts  # noqa: F401  (stem-generic: load_parts("goodpoint"), load_parts("goodpoint_track"))

SHAPES = ((32, 32), (32, 64), (64, 96), (96, 160), (480, 640))
PARAM = {"c0": 3, "c1": 8}
TRACK_SETS = ("defaults", "fund")       # the class defaults (3, 3, 1, 40) and config_fund.yaml's (10, 21, 3, 40)
CAP_PERCENT = 5                         # at most this share of a tracking case's points may be unstable


def checkpoint():
    """{name: torch tensor} as torch.load of the reference's weights/goodpoint.pth gives it (without num_batches_tracked)."""
    import torch
    return {k: torch.from_numpy(v) for k, v in load_parts("goodpoint_state_dict").items()}


def track_params(g, name):
    d, w, lv, it = (int(v) for v in g[name + "_prm"])
    return {"distance": d, "win_size": w, "levels": lv, "interation": it, "gray": False}


def chain(t, img):
    """(score [B,1,H,W], desc [B,3,H,W]) from the folded tensors `t` (weights.fold_goodpoint): GoodPoint.py:103-109."""
    import torch
    import torch.nn.functional as F
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    x1 = F.relu(F.conv2d(F.relu(F.conv2d(img, tt(t["b1c1.w"]), tt(t["b1c1.b"]), padding=1)), tt(t["b1c2.w"]), tt(t["b1c2.b"]), padding=1))
    score = torch.sigmoid(F.conv2d(x1, tt(t["gp.score.w"])[None], padding=1))
    desc = torch.sigmoid(F.conv2d(x1, tt(t["gp.desc.w"])[:, :, None, None]))
    return score, desc
