"""Loader of the R2D2 fixtures of tests/golden/make_golden_r2d2.py: arrays cut into pieces `name@i` over r2d2*.npz are joined again."""
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


def checkpoint():
    """{'net': str, 'state_dict': {name: torch tensor}} as torch.load of the reference's weights/r2d2_WASF_N16.pt gives it."""
    import torch
    t = load_parts("r2d2_state_dict")
    net = str(t.pop("net"))
    return {"net": net, "state_dict": {k: torch.from_numpy(v) for k, v in t.items()}}
