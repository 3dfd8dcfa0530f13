"""Sub-pixel refinement (KPB_OPT_DETECT_REFINE), the part that needs no GPU: the properties of the numpy restatement the device is pinned to
(tests/detect_refine_cases.py), the option's number in the header, the binding and the documents, the Python surface, and mode 2's tolerance."""
import os
import re

import numpy as np
import pytest

import detect_refine_cases as C
from keypoint_bench_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _dx(row, c, mode=1):
    """dx of pixel c of a one-row-high neighbourhood embedded in a 5 x len map (rows above and below are copies scaled down: the y parabola is regular)."""
    row = np.asarray(row, np.float32)
    s = np.stack([row * np.float32(0.25), row * np.float32(0.5), row, row * np.float32(0.5), row * np.float32(0.25)])
    return float(C.refine_offsets(s, [2 * len(row) + c], 5, len(row), mode)[0][0])


# ------------------------------------------------------------------------------------------------ the restatement's properties
@pytest.mark.parametrize("mode", [1, 2])
def test_a_symmetric_neighbourhood_gives_zero(mode):
    """Exactly 0 for the parabola (a - e is 0).  The soft-argmax adds its 25 weighted offsets one after the other in fp32, so mirrored taps cancel up to the
    rounding of the running sums: 25 additions, each within 2^-24 of a sum that |offset| <= 2 bounds by 2 Sw."""
    tol = 0.0 if mode == 1 else 25 * 2.0 ** -24 * 2
    assert abs(_dx([0.1, 0.2, 0.5, 0.9, 0.5, 0.2, 0.1], 3, mode)) <= tol
    s = C.bumps(9, 9, [(4.5, 4.5)], 1.5, 1.0)
    dx, dy = C.refine_offsets(s, [4 * 9 + 4], 9, 9, mode)
    assert abs(dx[0]) <= tol and abs(dy[0]) <= tol


def test_plateau_border_minimum_and_nan_give_zero():
    assert _dx([0.3, 0.7, 0.7, 0.7, 0.2], 2) == 0.0                 # a plateau: den == 0
    assert _dx([0.9, 0.5, 0.1, 0.4, 0.9], 2) == 0.0                 # a minimum: den > 0
    assert _dx([0.9, 0.5, 0.1], 0) == 0.0 and _dx([0.1, 0.5, 0.9], 2) == 0.0       # the first and the last column, whatever lies beside them
    assert _dx([0.3, np.nan, 0.7, 0.5, 0.2], 2) == 0.0              # a NaN neighbour
    assert _dx([0.3, 0.6, np.nan, 0.5, 0.2], 2) == 0.0              # a NaN centre
    assert _dx([0.3, np.inf, np.inf, 0.5, 0.2], 2) == 0.0           # inf - inf
    assert _dx([0.3, 0.4, np.inf, 0.5, 0.2], 2) == 0.0              # an infinite maximum: (a - e) / -inf is a zero, either sign (-0.0 == 0.0)
    # the same rules hold along y: the transposed maps
    s = np.array([[0.3, 0.7, 0.7, 0.7, 0.2]] * 3, np.float32).T.copy()
    assert float(C.refine_offsets(s, [2 * 3 + 1], 5, 3, 1)[1][0]) == 0.0


def test_quadratic_offsets_stay_within_half_a_pixel_and_adjacent_equal_maxima_give_half():
    assert _dx([0.1, 0.2, 0.9, 0.9, 0.2], 2) == 0.5 and _dx([0.1, 0.2, 0.9, 0.9, 0.2], 3) == -0.5
    rng = np.random.default_rng(3)
    for _ in range(20):                                             # every pixel of random maps, maxima or not, tiny and huge values mixed in
        s = (rng.random((17, 23)) * rng.choice([1e-30, 1.0, 1e30], (17, 23))).astype(np.float32)
        dx, dy = C.refine_offsets(s, np.arange(17 * 23), 17, 23, 1)
        assert dx.dtype == np.float32 and np.isfinite(dx).all() and np.isfinite(dy).all()
        assert np.abs(dx).max() <= 0.5 and np.abs(dy).max() <= 0.5
    xy = C.refine_np(s, np.arange(17 * 23), 17, 23, 1)
    assert (xy >= 0).all() and (xy <= 1).all()


def test_softargmax_rules():
    s = C.special_map()
    H, W = s.shape
    dx, dy = C.refine_offsets(s, np.arange(H * W), H, W, 2)
    assert np.isfinite(dx).all() and np.isfinite(dy).all() and np.abs(dx).max() <= 2 and np.abs(dy).max() <= 2
    # the infinite maximum leaves no tap with weight in any window that holds it (inf - inf is NaN, everything else is exp(-inf)): 0
    for r in range(5, 10):
        for c in range(9, 14):
            assert dx[r * W + c] == 0.0 and dy[r * W + c] == 0.0, (r, c)
    # taps outside the map are skipped: at the corner of a constant map the mean of the in-map offsets, (0 + 1 + 2) / 3
    one = np.ones((6, 6), np.float32)
    dx, dy = C.refine_offsets(one, [0, 35], 6, 6, 2)
    assert dx[0] == 1.0 and dy[0] == 1.0 and dx[1] == -1.0 and dy[1] == -1.0
    # the refined position stays inside the map
    xy = C.refine_np(s, np.arange(H * W), H, W, 2)
    assert (xy >= 0).all() and (xy <= 1).all()
    # mode 0 is the pixel centre, as select_topk writes it
    xy = C.refine_np(s, [W + 3], H, W, 0)
    assert xy[0, 0] == np.float32(3.5) / np.float32(W) and xy[0, 1] == np.float32(1.5) / np.float32(H)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("seed", [7, 8, 9, 10])
def test_bumps_are_localised_four_times_better_than_their_pixel_centres(seed, mode):
    """sigma 1.5, amplitude 1, centres >= 12 px apart, each 0.1 .. 0.5 px (larger coordinate) off its pixel's centre: the refined error of every bump is at most a quarter
    of the pixel-centre error.  (Over 1 900 random offsets the worst ratio is 0.104 for the parabola and 0.177 for the soft-argmax: 0.25 is met with margin.)"""
    H, W = C.BUMP_SHAPE
    cen, idx = C.bump_centres(seed)
    off = np.abs(cen - (np.floor(cen) + 0.5)).max(axis=1)
    assert len(idx) == 24 and (off >= 0.1 - 1e-12).all() and (off <= 0.5).all()
    s = C.bump_map(seed)
    assert (s.reshape(-1)[idx] >= s.reshape(-1)[idx + 1]).all() and (s.reshape(-1)[idx] >= s.reshape(-1)[idx - W]).all()     # the bump's pixel is its maximum
    ratios = C.bump_ratios(C.refine_np(s, idx, H, W, mode), idx, seed)
    print("mode %d seed %d worst ratio %.4f" % (mode, seed, ratios.max()))
    assert ratios.max() <= 0.25


# ------------------------------------------------------------------------------------------------ mode 2's tolerance
def test_soft_tolerance_covers_the_restatements_own_rounding():
    """SOFT_TOL_PX = 4 x the worst |float32 restatement - float64 restatement| over the rows of the GPU cases, in pixels: the stored figure still covers the measured one."""
    worst = {name: C.soft_deviation_px(name) for name in C.CASES}
    H, W = C.BUMP_SHAPE
    _, idx = C.bump_centres()
    worst["bumps"] = float(np.abs(C.pixels(C.refine_np(C.bump_map(), idx, H, W, 2), H, W) - C.pixels(C.refine_np(C.bump_map(), idx, H, W, 2, np.float64), H, W)).max())
    print(worst)
    assert max(worst.values()) <= C.SOFT_WORST_PX
    assert max(worst.values()) >= 0.5 * C.SOFT_WORST_PX, "the stored figure is no longer the measured one"
    assert C.SOFT_TOL_PX == 4 * C.SOFT_WORST_PX
    assert all(len(i) > 0 for name in C.CASES for i in C.kept_rows_cpu(name)), "a case without rows measures nothing"


def test_cases_reach_their_paths():
    """The premises of the GPU cases, on the CPU: rows on the map's edge; top_k cuts; two selection chunks; 64 images; negative scores beside kept rows; a non-maximum row."""
    idx = {name: C.kept_rows_cpu(name) for name in C.CASES}
    maps, prm, _, _ = C.case("raster_edges")
    r, c = idx["raster_edges"][0] // 32, idx["raster_edges"][0] % 32
    assert ((c == 0) | (c == 31)).any() and ((r == 0) | (r == 31)).any()
    maps, prm, _, _ = C.case("sorted")
    assert all(len(i) == prm["top_k"] for i in idx["sorted"]) and any((np.diff(i) < 0).any() for i in idx["sorted"])
    maps, prm, _, _ = C.case("select_scan")
    assert maps.shape[1] * maps.shape[2] > 16384 and maps.shape[0] < 64 and all((i >= 16384).any() and (i < 16384).any() for i in idx["select_scan"])
    assert C.case("bitmap")[0].shape[0] == 64 and C.case("bitmap")[1]["threshold"] == 0.0
    maps, prm, signed, _ = C.case("signed")
    assert signed and all((m < 0).any() and len(i) > 0 for m, i in zip(maps, idx["signed"]))
    i = idx["signed"][0]
    i = i[i % 96 > 0]
    assert (maps[0].reshape(-1)[i - 1] < 0).any(), "no kept row has a negative neighbour"
    maps, prm, _, _ = C.case("nms0")
    s = maps[0]
    i = idx["nms0"][0]
    inner = i[(i % 24 > 0) & (i % 24 < 23)]
    assert prm["nms_dist"] == 0 and (s.reshape(-1)[inner] < s.reshape(-1)[inner + 1]).any()
    s = C.special_map()
    assert np.isnan(s).sum() == 2 and np.isinf(s).sum() == 1 and s[5, 15] == s[5, 16] and len(idx["special"][0]) == s.size - 2


# ------------------------------------------------------------------------------------------------ the option's number, the binding, the documents
def test_option_number_in_header_binding_and_documents():
    m = re.search(r"^#define KPB_OPT_DETECT_REFINE (\d+)\b", _read("include", "kpb.h"), re.M)
    assert m and int(m.group(1)) == 7 == _lib.Context.OPT_DETECT_REFINE
    assert re.search(r"case KPB_OPT_DETECT_REFINE:", _read("keypoint_bench_amd", "csrc", "api.hip"))
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = _read(doc)
        assert "KPB_OPT_DETECT_REFINE" in text, doc
        for num in re.findall(r"KPB_OPT_DETECT_REFINE`?\s*(?:=|\(option)\s*(\d+)", text):
            assert int(num) == 7, "%s names option number %s" % (doc, num)
    assert re.search(r"KPB_OPT_DETECT_REFINE`?\s*=\s*7\b", _read("DESIGN.md")) and re.search(r"KPB_OPT_DETECT_REFINE`?\s*\(option 7\b", _read("INTEGRATION.md")), "DESIGN.md / INTEGRATION.md do not name the option's number"
    assert "(41 exports)" in _read("README.md")


def test_option_numbers_are_distinct_and_the_abi_keeps_41_exports():
    header = _read("include", "kpb.h")
    defs = dict(re.findall(r"^#define (KPB_OPT_\w+) (\d+)\b", header, re.M))
    assert len(defs) == 7 and len(set(defs.values())) == len(defs), defs
    opts = {k: v for k, v in vars(_lib.Context).items() if k.startswith("OPT_")}
    assert {"KPB_" + k: str(v) for k, v in opts.items()} == defs
    assert len(_lib.SIGNATURES) == 41
    assert len(re.findall(r"^(?:int|void|const char\*) (kpb_\w+)\(", header, re.M)) == 41


def test_refine_names():
    assert _lib.REFINE == {None: 0, "none": 0, "quadratic": 1, "softargmax": 2}
    assert [_lib.refine_id(n) for n in (None, "none", "quadratic", "softargmax")] == [0, 0, 1, 2]
    for bad in ("cubic", "Quadratic", 1, True, ["quadratic"], ""):
        with pytest.raises(ValueError):
            _lib.refine_id(bad)


def test_detect_refine_context_manager_sets_restores_and_leaves_alone():
    """Shaped like detect_signed: sets the option inside the block, restores on exit and on an exception, and does not touch it when nothing changes."""
    calls = []

    class Fake(_lib.Context):
        def __init__(self):
            pass

        def set_option(self, option, value):
            calls.append((int(option), int(value)))
            if int(option) == self.OPT_DETECT_REFINE:
                self._detect_refine = int(value)

    ctx = Fake()
    with ctx.detect_refine(0):
        pass
    assert calls == []
    with ctx.detect_refine(1):
        assert calls == [(7, 1)]
        with ctx.detect_refine(1):
            pass
        assert calls == [(7, 1)]
        with ctx.detect_refine(2):
            assert calls[-1] == (7, 2)
        assert calls == [(7, 1), (7, 2), (7, 1)]
    assert calls[-1] == (7, 0) and len(calls) == 4
    with pytest.raises(KeyError):
        with ctx.detect_refine(2):
            raise KeyError("inside")
    assert calls[-2:] == [(7, 2), (7, 0)] and ctx._detect_refine == 0


def test_host_tensors_are_refused_as_before():
    import torch
    from keypoint_bench_amd.utils.extracter import detection, detection_batch
    p = dict(nms_dist=2, threshold=0.0, border_dist=0, top_k=10, min_score=0.0, refine="quadratic")
    with pytest.raises(RuntimeError):
        detection(torch.zeros((1, 1, 16, 16)), p)
    with pytest.raises(RuntimeError):
        detection_batch(torch.zeros((2, 1, 16, 16)), dict(p, refine=None))


def test_the_shim_refuses_to_hand_a_refined_detection_to_the_reference():
    """The reference's detection does not read `refine`: routing the call there (a host tensor) would return pixel centres without a word."""
    import torch
    from keypoint_bench_amd import shim
    from keypoint_bench_amd.utils.extracter import detection
    seen = []
    g = shim.guarded("utils.extracter.detection", detection, lambda *a, **k: seen.append(a) or "reference", shim._c_detection, refuse=shim.refine_refusal)
    p = dict(nms_dist=2, threshold=0.0, border_dist=0, top_k=10, min_score=0.0)
    assert g(torch.zeros((1, 1, 16, 16)), p) == "reference" and g(torch.zeros((1, 1, 16, 16)), dict(p, refine="none")) == "reference" and len(seen) == 2
    assert g(torch.zeros((1, 1, 16, 16))) == "reference"
    with pytest.raises(ValueError, match="refine"):
        g(torch.zeros((1, 1, 16, 16)), dict(p, refine="quadratic"))
    assert len(seen) == 3
