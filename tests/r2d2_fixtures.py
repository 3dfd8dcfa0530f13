"""Loader of the R2D2 fixtures of tests/golden/make_golden_r2d2.py: arrays cut into pieces `name@i` over r2d2*.npz are joined again; and the net restated as a
few lines of torch.nn.functional over the folded tensors (tests/test_r2d2_cpu.py holds it to the reference's goldens)."""
import glob
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ((64, 96), (61, 97), (24, 40), (480, 640))


def load_parts(stem):
    files = [f for f in glob.glob(os.path.join(GOLDEN, stem + "*.npz")) if re.fullmatch(re.escape(stem) + r"(\.\d+)?\.npz", os.path.basename(f))]
    assert files, "fixture %s*.npz missing" % stem
    whole, pieces = {}, {}
    for f in files:
        with np.load(f, allow_pickle=False) as z:
            for k in z.files:
                if "@" in k:
                    name, i = k.rsplit("@", 1)
                    pieces.setdefault(name, {})[int(i)] = z[k]
                else:
                    whole[k] = z[k]
    for name, p in pieces.items():
        assert sorted(p) == list(range(len(p))), "fixture %s: pieces of %s missing" % (stem, name)
        whole[name] = np.concatenate([p[i] for i in range(len(p))], axis=0)
    return whole


def chain(t, img):
    """(score [B,1,H,W], desc [B,128,H,W]) from the folded tensors `t`, by the plan table.  float64 tensors and image give the float64 chain."""
    import torch
    import torch.nn.functional as F
    from keypoint_bench_amd import weights
    x = img
    for name, cin, cout, k, dil, bn, relu in weights.R2D2_PLAN:
        x = F.conv2d(x, torch.from_numpy(t[name + ".w"]), torch.from_numpy(t[name + ".b"]), padding=(k - 1) * dil // 2, dilation=dil)
        if relu:
            x = F.relu(x)
    sq = x * x
    clf = F.conv2d(sq, torch.from_numpy(t["clf.w"])[:, :, None, None], torch.from_numpy(t["clf.b"]))
    sal = F.softplus(F.conv2d(sq, torch.from_numpy(t["sal.w"])[:, :, None, None], torch.from_numpy(t["sal.b"])))
    score = sal / (1 + sal) * F.softmax(clf, dim=1)[:, 1:2]
    return score, x / torch.linalg.norm(x, dim=1, keepdim=True).clamp_min(1e-12)


def checkpoint():
    """{'net': str, 'state_dict': {name: torch tensor}} as torch.load of the reference's weights/r2d2_WASF_N16.pt gives it."""
    import torch
    t = load_parts("r2d2_state_dict")
    net = str(t.pop("net"))
    return {"net": net, "state_dict": {k: torch.from_numpy(v) for k, v in t.items()}}
