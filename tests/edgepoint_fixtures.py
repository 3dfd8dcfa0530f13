"""The EdgePoint fixtures of tests/golden/make_golden_edgepoint.py: the shapes of edgepoint*.npz and the reference checkpoint."""
from r2d2_fixtures import load_parts  # noqa: F401  (stem-generic: load_parts("edgepoint"))

SHAPES = ((32, 32), (32, 64), (64, 96), (96, 160), (480, 640))
PARAM = {"c1": 8, "c2": 16, "c3": 32, "c4": 64, "dim": 64}


def checkpoint():
    """{name: torch tensor} as torch.load of the reference's weights/EdgePoint.pt gives it (without num_batches_tracked)."""
    import torch
    return {k: torch.from_numpy(v) for k, v in load_parts("edgepoint_state_dict").items()}
