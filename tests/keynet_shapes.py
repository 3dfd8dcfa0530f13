"""What tests/test_gpu_keynet_shapes.py and tests/test_keynet_shape_oracles_cpu.py share: the shapes and batches Key.Net (csrc/keynet.hip) is swept over, with
the level sizes each must produce as a literal table, the net's torch.nn.functional chain (keynet_fixtures.chain on weights.fold_keynet(checkpoint())) in fp32 and
float64, the bound of the GPU test as a function of the two chains alone, and the deliberately wrong chains that show the bound can fail.

The wrong chains are the fixtures' chain itself with ONE primitive of torch.nn.functional replaced while it runs (`wrong(kind)`, the style of
layer_net_shapes.wrong), so a variant differs from the oracle in the named respect and in nothing else:
  replicate    F.pad(mode='reflect') read as 'replicate': the blur of custom_pyrdown repeats the edge pixel
  reflect      F.pad(mode='replicate') read as 'reflect': the Sobel pairs mirror around the edge pixel instead of repeating it
  align        F.interpolate with the align_corners flag flipped (the pyramid's resize and the head's two upsamplings)
  lastcol      F.interpolate never reads the last source column: where a tap falls on it, the column before is read (`min(i0 + 1, in - 1)` as `in - 2`)

The bound (the per-net file's rule): max |device - chain64| <= M x ref_err, ref_err = max |chain32 - chain64| of the same pixels computed in the test, floored at
one fp32 unit in the last place of the float64 map's maximum (layer_net_shapes.ref_err); the border ring (the outermost 8 pixels) and the interior apart where the
interior has at least MIN_INTERIOR pixels, else the whole map at once -- on a handful of pixels ref_err is an accident of rounding (17 x 33: 4.4e-4 for the 17
interior pixels against 2.9e-3 for the ring).  M = M_H16 / M_FP32 of keynet_fixtures.

Measured on an MI355X, max |device - chain64| / ref_err (ring / interior, or the whole map where the interior is too small); batches: the largest over the images:
                 split-f16        strict fp32 (KPB_FP32_MATRIX=1)
  16 x 640       1.114            1.149
  640 x 16       1.080            1.140
  17 x 33        1.742            1.742
  20 x 39        1.122            1.170
  21 x 40        0.962            1.145
  33 x 65        1.227 / 0.907    1.396 / 0.955
  47 x 78        1.522 / 1.512    1.390 / 1.906
  31 x 97        0.933 / 1.252    1.022 / 1.090
  64 x 129       1.242 / 1.339    1.242 / 1.218
  5 at 21 x 40   2.121            1.926
  17 at 20 x 39  2.082            1.787
  3 at 47 x 78   1.107 / 1.372    1.174 / 1.312
Every case stays under the fixtures' M_H16 = 4 and M_FP32 = 8 (twice the largest ratio would be 4.24 and 3.85 -- the batch of 5 at 21 x 40 sits just where M_H16
was drawn, and holds it): no constant of this sweep's own was derived, `multiplier` hands out the fixtures' two.  Every image of every batch equals its solo run
bit for bit in both arithmetics.  No test of the two files failed for a defect in csrc."""
import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

from keypoint_bench_amd import weights
from keynet_fixtures import BORDER, M_FP32, M_H16, chain, checkpoint
from layer_net_shapes import batch_images, ref_err, sid, sweep_image  # noqa: F401  (the crop convention and the batches of both earlier sweeps)

# (H, W): (level 1, level 2) -- what each shape reaches is in the docstring of the GPU file's sweep test
LEVELS = {
    (16, 640): ((13, 533), (10, 444)),
    (640, 16): ((533, 13), (444, 10)),
    (17, 33): ((14, 27), (11, 22)),
    (20, 39): ((16, 32), (13, 26)),
    (21, 40): ((17, 33), (14, 27)),
    (33, 65): ((27, 54), (22, 45)),
    (47, 78): ((39, 65), (32, 54)),
    (31, 97): ((25, 80), (20, 66)),
    (64, 129): ((53, 107), (44, 89)),
}
SHAPES = list(LEVELS)
BATCHES = [(5, (21, 40)), (17, (20, 39)), (3, (47, 78))]
BATCH_LEVELS = {(21, 40): LEVELS[(21, 40)], (20, 39): LEVELS[(20, 39)], (47, 78): LEVELS[(47, 78)]}
MIN_INTERIOR = 256              # pixels the interior must have to be judged apart from the ring
WRONG = ("replicate", "reflect", "align", "lastcol")
TEETH = 16                      # the largest multiplier any Key.Net test may use: every wrong chain must miss TEETH x ref_err at every sweep shape


def check_levels(H, W):
    """The level sizes the library computes for H x W are the table's."""
    assert weights.keynet_level_sizes(H, W) == [(H, W)] + list(LEVELS[(H, W)]), (H, W, weights.keynet_level_sizes(H, W))


@functools.lru_cache(maxsize=None)
def tensors(double=False):
    """The folded tensors the net object of the GPU test is made from, as numpy arrays in fp32 or cast to float64."""
    return {k: np.ascontiguousarray(v, np.float64 if double else np.float32) for k, v in weights.fold_keynet(checkpoint()).items()}


@contextlib.contextmanager
def wrong(kind):
    """torch.nn.functional with one primitive wrong while the block runs (module docstring); kind None changes nothing."""
    interpolate, pad = F.interpolate, F.pad
    swap = {"reflect": "replicate", "replicate": "reflect"}

    def pad_as(src):
        return lambda x, p, mode="constant", **kw: pad(x, p, mode=swap[mode] if mode == src else mode, **kw)

    def lastcol(x, **kw):
        return interpolate(torch.cat([x[..., :-1], x[..., -2:-1]], dim=-1), **kw)

    patch = {None: {}, "replicate": {"pad": pad_as("reflect")}, "reflect": {"pad": pad_as("replicate")},
             "align": {"interpolate": lambda x, **kw: interpolate(x, **dict(kw, align_corners=not kw["align_corners"]))},
             "lastcol": {"interpolate": lastcol}}[kind]
    for k, f in patch.items():
        setattr(F, k, f)
    try:
        yield
    finally:
        F.interpolate, F.pad = interpolate, pad


def oracle(imgs, double=False, kind=None):
    """score [B,H,W] (numpy) of imgs [B,3,H,W] from the chain, in fp32 or with the folded tensors and the image cast to float64; `kind` names a wrong variant."""
    x = torch.from_numpy(np.ascontiguousarray(imgs, np.float64 if double else np.float32))
    with torch.no_grad(), wrong(kind):
        s, none = chain(tensors(double), x)
    assert none is None
    return s[:, 0].numpy()


def regions(H, W):
    """[(name, mask)]: the ring and the interior apart where the interior has MIN_INTERIOR pixels, else the whole map."""
    inner = np.zeros((H, W), bool)
    inner[BORDER:H - BORDER, BORDER:W - BORDER] = True
    if int(inner.sum()) >= MIN_INTERIOR:
        return [("ring", ~inner), ("interior", inner)]
    return [("whole", np.ones((H, W), bool))]


def judge(got, r32, r64):
    """[(region, max |got - chain64|, ref_err)] of one image's map [H,W]; the GPU test asserts error <= M x ref_err in every region."""
    d = np.abs(got.astype(np.float64) - r64)
    return [(name, float(d[m].max()), ref_err(r32, r64, m)) for name, m in regions(*got.shape)]


def multiplier():
    """(split-f16, strict fp32)"""
    return M_H16, M_FP32
