"""The ALIKE-l fixtures of tests/golden/make_golden_alike_l.py: the shapes of alike_l*.npz and the seeded stand-in state dict (the reference ships no
checkpoint for its default plan).  A fixture's `.desc` is the whole [H, W, 128] map for the first FULL_DESC shapes and desc[::8, ::8] for the others."""
from r2d2_fixtures import load_parts  # noqa: F401  (stem-generic: load_parts("alike_l"))

SHAPES = ((32, 32), (32, 64), (64, 96), (96, 160), (160, 224))
FULL_DESC = 2
PARAM = {"c1": 32, "c2": 64, "c3": 128, "c4": 128, "dim": 128}
# the project's ALIKE bars (tests/test_gpu_alike.py): score atol 7e-6, descriptors atol 1e-4 x max(1, max |desc_ref|) of the shape -- these maps are not unit-scale
SCORE_ATOL, DESC_ATOL = 7e-6, 1e-4


def state_dict():
    """{name: torch tensor} as ALNet().state_dict() of the reference gives it (without num_batches_tracked)."""
    import torch
    return {k: torch.from_numpy(v) for k, v in load_parts("alike_l_state_dict").items()}


def desc_of(fix, shape, desc):
    """`desc` [H, W, 128] (numpy) cut the way the fixture of `shape` stores it."""
    return desc if SHAPES.index(tuple(shape)) < FULL_DESC else desc[::8, ::8]


def desc_bar(ref_desc):
    import numpy as np
    return DESC_ATOL * max(1.0, float(np.abs(ref_desc).max()))
