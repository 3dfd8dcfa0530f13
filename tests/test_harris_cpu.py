"""Harris without a GPU: the numpy oracle of tests/harris_fixtures.py against an independent formulation (scipy.ndimage), the gray rule, the bounds that
make the float64 response exact up to its last line, and the Python surface (models.Harris, weights.harris_plan, runner.build_model, include/kpb.h)."""
import os
import re

import numpy as np
import pytest

from keypoint_bench_amd import runner, weights
from harris_fixtures import (BLOCK_SIZES, CONFIG_PLAN, DX_MAX, TILE, gray_plane, harris_oracle, image, ramp, response64, sobel, stripes,
                             structure_tensor)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(block_size=CONFIG_PLAN[0], ksize=CONFIG_PLAN[1], k=CONFIG_PLAN[2])


# ------------------------------------------------------------------------------------------------ 1. the oracle against scipy.ndimage
def _ndimage_planes(g, b, dtype):
    from scipy.ndimage import correlate1d
    g = g.astype(dtype)
    sm = lambda a, ax: correlate1d(a, np.array([1, 2, 1], dtype), axis=ax, mode="mirror")
    df = lambda a, ax: correlate1d(a, np.array([-1, 0, 1], dtype), axis=ax, mode="mirror")
    dx, dy = df(sm(g, 0), 1), df(sm(g, 1), 0)
    box = lambda p: correlate1d(correlate1d(p, np.ones(b, dtype), axis=0, mode="mirror", origin=0), np.ones(b, dtype), axis=1, mode="mirror", origin=0)
    return dx, dy, box


@pytest.mark.parametrize("H,W", [(8, 8), (9, 13), (37, 61)])
@pytest.mark.parametrize("b", BLOCK_SIZES)
def test_oracle_integer_planes_equal_the_ndimage_formulation(H, W, b):
    g = gray_plane(image("frames", H, W, seed=3))
    assert g.min() >= 0 and g.max() <= 255 and len(np.unique(g)) > 20
    dx, dy, box = _ndimage_planes(g, b, np.int64)
    sx, sy = sobel(g)
    assert np.array_equal(dx, sx) and np.array_equal(dy, sy) and np.abs(dx).max() <= DX_MAX
    A, B, C = structure_tensor(g, b)
    assert np.array_equal(A, box(dx * dx)) and np.array_equal(B, box(dx * dy)) and np.array_equal(C, box(dy * dy))
    assert A.dtype == np.int64 and (B != 0).any()


@pytest.mark.parametrize("H,W", [(8, 8), (9, 13), (37, 61)])
@pytest.mark.parametrize("b", BLOCK_SIZES)
@pytest.mark.parametrize("k", [0.04, 0.06])
def test_oracle_against_float64_in_cv2_order(H, W, b, k):
    """cv2's order -- scale first, then square, box, response -- in float64.  Tolerance 1e-12 (|a c| + b^2 + |k| (a + c)^2) per pixel: float64 epsilon
    (1.1e-16) times about 10^4 operations' worth of head-room; derived, not measured."""
    g = gray_plane(image("frames", H, W, seed=4))
    dx, dy, box = _ndimage_planes(g, b, np.float64)
    scale = 1.0 / (2.0 ** (3 - 1) * b * 255.0)
    dx, dy = dx * scale, dy * scale
    a, bb, c = box(dx * dx), box(dx * dy), box(dy * dy)
    k32 = float(np.float32(k))
    want = a * c - bb * bb - k32 * (a + c) * (a + c)
    got = response64(g, b, k)
    tol = 1e-12 * (np.abs(a * c) + bb * bb + abs(k32) * (a + c) ** 2)
    assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) - tol).max())
    assert np.abs(want).max() > 1e-6                                    # (not a comparison of zeros)
    assert harris_oracle(image("frames", H, W, seed=4), b, k).dtype == np.float32


# ------------------------------------------------------------------------------------------------ 2. the gray rule
def test_gray_truncates_where_float32_falls_below_the_byte():
    """All 256 bytes v as channel 0 = v / 255.  float32 division is correctly rounded and (v / 255) * 255 comes back as v for EVERY v (asserted: a decoded
    image's bytes survive), so the ramp alone cannot tell truncation from rounding; the same ramp one float32 step towards zero can: its products lie just
    below v and must give v - 1."""
    x = ramp(1, 256)
    v = np.arange(256)
    f = x[0, 0] * np.float32(255.0)
    assert f.dtype == np.float32 and np.array_equal(f, v.astype(np.float32))
    assert np.array_equal(gray_plane(x)[0], v)
    lo = x.copy()
    lo[0] = np.nextafter(x[0], np.float32(0.0))
    fl = lo[0, 0] * np.float32(255.0)
    below = fl < v
    assert below.sum() > 200 and not (fl > v).any() and (v - fl).max() < 1e-4
    assert np.array_equal(gray_plane(lo)[0], np.where(below, v - 1, v))      # truncated, not rounded


def test_gray_wraps_sums_above_one_and_below_zero():
    """Dyadic channel values, so that every float32 operation is exact and the expected byte can be written down by hand."""
    cases = [((1, 0, 0), 255), ((1, 2.0 ** -8, 0), 255),            # 255.996 truncates to 255
             ((1, 2.0 ** -7, 0), 0),                                 # 256.99 -> 256 -> 0
             ((1, 0.5, 0), 382 - 256), ((1, 1, 0), 510 - 256), ((1, 1, 0.25), 573 - 512), ((1, 1, 1), 765 - 512),
             ((-(2.0 ** -8), 0, 0), 0),                              # -0.996 truncates TOWARD ZERO, not to -1
             ((-(2.0 ** -7), 0, 0), 255),                            # -1.99 -> -1 -> 255
             ((-0.25, 0, 0), 256 - 63), ((-1, 0, 0), 1), ((-1, -1, 0), 2), ((0.5, -1, 0.25), 256 - 63)]
    x = np.array([c for c, _ in cases], np.float32).T.reshape(3, 1, len(cases)).copy()
    assert gray_plane(x)[0].tolist() == [w for _, w in cases]


# ------------------------------------------------------------------------------------------------ 3. bounds
def test_worst_case_image_keeps_the_integer_terms_exact_for_block_size_6_and_not_7():
    bound = lambda b: (b * b * DX_MAX ** 2, (2 * b * b * DX_MAX ** 2) ** 2)      # A (and C) at most; t2 = (A + C)^2 at most
    assert DX_MAX ** 2 == 1040400
    a6, t6 = bound(6)
    assert a6 < 2 ** 31 and t6 < 2 ** 53 and t6 == 74908800 ** 2 and a6 * a6 < 2 ** 53      # |det| <= A C
    assert bound(7)[1] >= 2 ** 53
    for tr in (False, True):            # the bound on A (on C, transposed) is attained: |dx| = 1020 at every pixel of the stripes off the frame's edge
        g = gray_plane(stripes(16, 16, transpose=tr))
        assert set(np.unique(g).tolist()) == {0, 255}
        dx, dy = sobel(g)
        if tr:
            dx, dy = dy.T, dx.T
        assert (np.abs(dx[:, 1:-1]) == DX_MAX).all() and not dx[:, [0, -1]].any() and not dy.any()      # (reflect-101 makes the edge columns' own dx zero)
        A, B, C = structure_tensor(g, 6)
        A = C.T if tr else A
        assert (A[:, 4:-4] == a6).all() and A.max() == a6 and not B.any()
        assert np.isfinite(response64(g, 6, 0.04)).all()                 # (its own assertion: det, t2 < 2^53)
    with pytest.raises(NotImplementedError):
        weights.harris_plan(dict(PARAMS, block_size=7))


# ------------------------------------------------------------------------------------------------ 4. the Python surface
def test_harris_class_blob_and_refusals():
    from keypoint_bench_amd.models.Harris import Harris
    from keypoint_bench_amd.models._base import HipNet
    net = Harris(PARAMS)
    assert isinstance(net, HipNet) and net.signed_scores is True and net.dense_descriptors is False and net.tracked_maps is False
    assert (net.dim, net.desc_div, net.ARCH) == (0, 1, 13) and not hasattr(net, "load_state_dict")
    assert net.eval() is net and net._blob is not None                   # ready after construction
    arch, t = weights.unpack(net._blob)
    assert arch == weights.ARCH_HARRIS == 13 and list(t) == ["harris.plan"]
    assert t["harris.plan"].dtype == np.float32 and t["harris.plan"].tolist() == [5.0, 3.0, float(np.float32(0.04))]
    assert np.array_equal(weights.harris_plan(PARAMS)["harris.plan"], t["harris.plan"])
    for bad in (dict(PARAMS, ksize=5), dict(PARAMS, block_size=1), dict(PARAMS, block_size=7), dict(PARAMS, block_size=2.5), dict(PARAMS, k=float("inf")),
                dict(PARAMS, k=1e39)):
        with pytest.raises(NotImplementedError):
            Harris(bad)
    for missing in ("block_size", "ksize", "k"):                         # read with [], as the reference does
        with pytest.raises(KeyError):
            Harris({k: v for k, v in PARAMS.items() if k != missing})
    for b in (2, 3, 4, 5, 6):
        assert weights.unpack(Harris(dict(PARAMS, block_size=b, k=-0.5))._blob)[1]["harris.plan"].tolist() == [float(b), 3.0, -0.5]


def test_build_model_builds_harris_from_its_params_and_refuses_without_them():
    from keypoint_bench_amd.models.Harris import Harris
    net = runner.build_model({"model_type": "Harris", "Harris_params": dict(PARAMS)})
    assert isinstance(net, Harris) and net.params == PARAMS and net._blob is not None
    for cfg in ({"model_type": "Harris"}, {"model_type": "Harris", "Harris_params": None}, {"model_type": "Harris", "Harris_params": {}}):
        with pytest.raises(NotImplementedError, match="Harris") as e:
            runner.build_model(cfg)
        assert all(n in str(e.value) for n in ("Alike", "EdgePoint", "GoodPoint", "LETNet", "KeyNet", "sfd2", "D2Net")) and "Harris_params" in str(e.value)
    with pytest.raises(NotImplementedError):
        runner.build_model({"model_type": "Harris", "Harris_params": dict(PARAMS, ksize=5)})


def test_header_source_and_fixtures_agree():
    hdr = open(os.path.join(ROOT, "include", "kpb.h")).read()
    m = re.search(r"#define\s+KPB_ARCH_HARRIS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == weights.ARCH_HARRIS
    src = open(os.path.join(ROOT, "keypoint_bench_amd", "csrc", "harris.hip")).read()
    m = re.search(r"constexpr int HR_TH = (\d+), HR_TW = (\d+);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == TILE
    from keypoint_bench_amd import build
    assert "harris.hip" in build.SOURCES
