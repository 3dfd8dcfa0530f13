"""CPU-side checks of the PyrLK-R definition (tests/pyrlk_fixtures.py): the numpy oracle that csrc/pyrlk.hip is pinned to bit for bit.

What is checked here is that the definition IS a Lucas-Kanade tracker and that its integer stencils are what they say they are: pyrDown and the Scharr pair against
an independent scipy.ndimage computation, the level-cut rule on three shapes, sub-0.05 px tracking of a known shift, the refusals of a textureless image and of
points far outside, and the Python wrapper's refusal of host tensors.  The 0.05 px bound is a condition on the ORACLE (measured: 0.013 px at worst over the cases
below); the device's own bound is bit equality with this oracle (tests/test_gpu_pyrlk.py)."""
import numpy as np
import pytest
import torch

import pyrlk_fixtures as fx


def test_integer_stencils_agree_with_scipy():
    from scipy.ndimage import correlate1d
    rng = np.random.default_rng(1)
    for H, W in ((48, 64), (45, 61), (7, 5), (4, 4)):
        g = rng.integers(0, 256, (H, W)).astype(np.int64)
        k = np.array([1, 4, 6, 4, 1], np.int64)
        full = correlate1d(correlate1d(g, k, axis=0, mode="mirror"), k, axis=1, mode="mirror")
        want = (full[::2, ::2] + 128) >> 8
        got = fx.pyr_down(g)
        assert got.shape == ((H + 1) // 2, (W + 1) // 2) and np.array_equal(got, want)
        assert got.min() >= 0 and got.max() <= 255
        s, d = np.array([3, 10, 3], np.int64), np.array([-1, 0, 1], np.int64)
        dx, dy = fx.scharr(g)
        assert np.array_equal(dx, correlate1d(correlate1d(g, s, axis=0, mode="mirror"), d, axis=1, mode="mirror"))
        assert np.array_equal(dy, correlate1d(correlate1d(g, d, axis=0, mode="mirror"), s, axis=1, mode="mirror"))
    flat = np.full((9, 11), 200, np.int64)
    assert np.array_equal(fx.pyr_down(flat), np.full((5, 6), 200)) and not fx.scharr(flat)[0].any() and not fx.scharr(flat)[1].any()
    step = np.zeros((6, 6), np.int64)
    step[:, 3:] = 255
    assert int(np.abs(fx.scharr(step)[0]).max()) == 4080        # the bound the int16 planes rely on


def test_input_bytes_follow_the_harris_rule():
    v = np.arange(256, dtype=np.float32) / np.float32(255.0)
    x = np.stack([v.reshape(16, 16), (v.reshape(16, 16) + np.float32(1.0)), -v.reshape(16, 16)])
    b = fx.to_bytes(x)
    assert np.array_equal(b[0].ravel(), np.arange(256))                             # a decoded image's bytes come back
    assert np.array_equal(b[1].ravel(), (np.arange(256) + 255) & 255)               # values above 1 wrap
    assert np.array_equal(b[2].ravel(), (-np.arange(256)) & 255)                    # negative ones wrap from 256 down


def test_level_cut_rule():
    assert fx.level_sizes(48, 64, 21, 3) == [(48, 64), (24, 32)]
    assert fx.level_sizes(45, 61, 21, 3) == [(45, 61), (23, 31)]
    assert fx.level_sizes(120, 160, 21, 3) == [(120, 160), (60, 80), (30, 40)]
    assert fx.level_sizes(120, 160, 21, 1) == [(120, 160), (60, 80)] and fx.level_sizes(120, 160, 21, 0) == [(120, 160)]
    assert fx.level_sizes(120, 160, 3, 4) == [(120, 160), (60, 80), (30, 40), (15, 20), (8, 10)]
    assert fx.level_sizes(45, 61, 31, 3) == [(45, 61)]          # 23 x 31 is not larger than the window
    a, b = fx.shifted_pair(0, 45, 61)
    pp = fx.Prepared(a, b, 21, 3)
    assert pp.top == 1 and [tuple(s) for s in pp.sizes] == [(45, 61), (23, 31)]


@pytest.mark.parametrize("shift", [(2, 3), (5, -7)])
@pytest.mark.parametrize("win", [21, 15, 7])
def test_the_definition_tracks_a_known_shift(win, shift):
    H, W, n = 120, 160, 80
    worst = 0.0
    for seed in range(3):
        a, b = fx.shifted_pair(seed, H, W, shift)
        rng = np.random.default_rng(100 + seed)
        m = win + 8
        px = np.stack([rng.uniform(m, W - 1 - m, n), rng.uniform(m, H - 1 - m, n)], 1)
        pts = (px / np.array([W - 1, H - 1])).astype(np.float32)
        out, status = fx.pyrlk_oracle(a, b, pts, pts, win, 3)
        assert status.dtype == np.uint8 and (status == 1).all(), (win, shift, seed, np.nonzero(status != 1)[0])
        got = out * np.array([W - 1, H - 1], np.float32) - fx.pixels(pts, H, W)
        err = np.abs(got - np.array(shift, np.float32)).max()
        worst = max(worst, float(err))
        assert err < 0.05, (win, shift, seed, err)
    print("win %d shift %s: worst error %.4f px" % (win, shift, worst))


def test_a_constant_image_tracks_nothing_and_moves_nothing():
    H, W = 48, 64
    a = np.full((3, H, W), 0.3, np.float32)
    pts1, pts2 = fx.point_set(3, H, W, 15, n=80)
    pts1, pts2 = pts1[:-2], pts2[:-2]                   # the finite rows
    px, status, finite = fx.track_pixels(a, a, pts1, pts2, 15, 3)
    assert finite.all() and (status == 0).all()
    start = fx.pixels(pts2, H, W)
    assert np.array_equal(px.view(np.uint32), start.view(np.uint32))        # scaled down by 2^-L and doubled L times: the guess itself
    out, st2 = fx.pyrlk_oracle(a, a, pts1, pts2, 15, 3)
    assert np.array_equal(out.view(np.uint32), (start / np.array([W - 1, H - 1], np.float32)).view(np.uint32)) and (st2 == 0).all()


def test_points_far_outside_and_rows_that_are_not_finite():
    H, W = 120, 160
    a, b = fx.shifted_pair(0, H, W)
    sc = np.array([W - 1, H - 1], np.float32)
    pts = (np.array([[400.0, 60.0], [-40.0, 60.0], [80.0, 60.0]], np.float32) / sc).astype(np.float32)
    out, status = fx.pyrlk_oracle(a, b, pts, pts, 21, 3)
    assert status.tolist() == [0, 0, 1]
    bad1 = np.array([[np.nan, 0.5], [0.5, 0.5], [0.5, 0.5]], np.float32)
    bad2 = np.array([[0.5, 0.5], [0.25, np.inf], [0.5, 0.5]], np.float32)
    out, status = fx.pyrlk_oracle(a, b, bad1, bad2, 21, 3)
    assert status.tolist() == [0, 0, 1]
    assert np.array_equal(out[:2].view(np.uint32), bad2[:2].view(np.uint32))          # returned as given


def test_point_sets_hold_what_the_device_tests_need():
    H, W, win = 45, 61, 15
    p1, p2 = fx.point_set(5, H, W, win)
    assert p1.shape == p2.shape and 190 <= p1.shape[0] <= 210 and p1.dtype == np.float32
    px = fx.pixels(p1[:-2], H, W)
    assert (px == np.floor(px)).all(1).sum() >= 10 and ((px - np.floor(px)) == 0.5).all(1).sum() >= 5
    assert (px[:, 0] < -win).any() and (px[:, 0] > W + 200).any() and (px[:, 0] == 0).any() and (px[:, 1] == H - 1).any()
    assert not np.isfinite(p1[-2]).all() and not np.isfinite(p2[-1]).all()
    d = np.abs(fx.pixels(p2[:-2], H, W) - px)
    assert 5 < d.max() <= 10.001 and (d == 0).all(1).sum() >= 60


def test_python_wrappers_refuse_host_tensors():
    from keypoint_bench_amd.utils import matcher
    pts, img = torch.rand(5, 2), torch.rand(1, 3, 48, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        matcher.optical_flow_cv(pts, pts, img, img)
    with pytest.raises(RuntimeError, match="no CPU path"):
        matcher.optical_flow_cv_batch(img, img, pts[None], pts[None], None, {"win_size": 15, "levels": 3})


def test_opt_in_is_a_key_of_the_matcher_params_and_nothing_else_moves():
    from keypoint_bench_amd.tasks import visual_odometer as vo
    base = {"matcher_params": {"type": "optical_flow", "optical_flow_params": {"win_size": 15, "levels": 3}}}
    on = {"matcher_params": dict(base["matcher_params"], pyrlk="device")}
    assert not vo.pyrlk_opt_in(base) and vo.pyrlk_opt_in(on)
    assert not vo.pyrlk_opt_in({"matcher_params": dict(base["matcher_params"], pyrlk="cv2")}) and not vo.pyrlk_opt_in({"matcher_params": dict(base["matcher_params"], pyrlk=True)})
    s = torch.zeros(1, 1, 8, 8)
    with pytest.raises(NotImplementedError, match="cv2's tracker"):
        vo.match_branch(None, None, s, None, None, None, base)
    assert vo.SHIM_PYRLK is False


def test_the_option_is_the_header_s_no_export_is_added_and_the_documents_say_what_it_is():
    import os
    import re
    from conftest import ROOT
    from keypoint_bench_amd import _lib
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    opts = {k: int(v) for k, v in re.findall(r"#define\s+KPB_OPT_([A-Z0-9_]+)\s+(\d+)", read("include", "kpb.h"))}
    assert opts["LK_PYRLK"] == _lib.Context.OPT_LK_PYRLK == 6 and len(set(opts.values())) == len(opts)
    assert len(_lib.SIGNATURES) == 41 and not [k for k in _lib.SIGNATURES if "pyrlk" in k]
    assert "(41 exports)" in read("README.md")
    for doc in ("include/kpb.h", "README.md", "DESIGN.md", "INTEGRATION.md", "SURVEY.md", "scripts/_design_template.md"):
        text = read(*doc.split("/")).lower()
        assert "kpb_opt_lk_pyrlk" in text and "optical_flow_cv" in text, doc
        assert "restated, cv2 parity unpinned" in text, doc


def test_the_context_manager_sets_and_restores_the_option():
    from keypoint_bench_amd import _lib
    calls = []

    class Fake(_lib.Context):
        def __init__(self):
            pass

        def check(self, rc):
            pass

        @property
        def lib(self):
            class L:
                @staticmethod
                def kpb_ctx_set_option(handle, option, value):
                    calls.append((option, value))
                    return 0
            return L

        handle = None

    c = Fake()
    with c.lk_pyrlk():
        assert calls == [(6, 1)] and c._lk_pyrlk == 1
        with c.lk_pyrlk():
            assert calls == [(6, 1)]
    assert calls == [(6, 1), (6, 0)] and c._lk_pyrlk == 0
    with pytest.raises(KeyError):
        with c.lk_pyrlk():
            raise KeyError("x")
    assert calls[-1] == (6, 0) and c._lk_pyrlk == 0


# ------------------------------------------------------------------------------------------------ the shim's opt-in swap
_STANDIN = {
    "utils/__init__.py": "",
    "tasks/__init__.py": "",
    "utils/matcher.py": "def optical_flow_cv(pts0, pts1, img0, img1, params=None):\n    return 'reference', (pts0, pts1, img0, img1, params)\n",
    "tasks/visual_odometer.py": "from utils.matcher import optical_flow_cv\n\n\ndef visual_odometry(*a, **k):\n    return 'reference'\n",
}


@pytest.fixture()
def standin_on_path(tmp_path):
    """A two-module layout of a reference checkout (utils/matcher.py with optical_flow_cv, tasks/visual_odometer.py importing it by name), written here."""
    import sys
    for rel, text in _STANDIN.items():
        f = tmp_path / rel
        f.parent.mkdir(exist_ok=True)
        f.write_text(text)
    before = set(sys.modules)
    sys.path.insert(0, str(tmp_path))
    old = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    from keypoint_bench_amd import shim
    shim.uninstall()
    try:
        yield shim
    finally:
        shim.uninstall()
        sys.path.remove(str(tmp_path))
        sys.dont_write_bytecode = old
        for k in set(sys.modules) - before:
            if k.split(".")[0] in ("utils", "models", "tasks"):
                del sys.modules[k]


def test_shim_swaps_optical_flow_cv_only_when_asked(standin_on_path):
    import warnings
    shim = standin_on_path
    from keypoint_bench_amd.tasks import visual_odometer as vo
    import tasks.visual_odometer as ref_vo
    import utils.matcher as ref_ma
    orig = ref_ma.optical_flow_cv
    prm = {"matcher_params": {"type": "optical_flow"}}
    host = torch.zeros(1, 1, 8, 8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert set(shim.install()) == {"tasks.visual_odometer.visual_odometry"}        # the default set: of this layout, only the task is on its list
        assert ref_ma.optical_flow_cv is orig and ref_vo.optical_flow_cv is orig and vo.SHIM_PYRLK is False
        assert vo.in_contract(0, None, None, None, None, host, None, None, None, None, prm) is not None
        shim.uninstall()
        swapped = shim.install(optical_flow_cv=True)
    assert set(swapped) == {"tasks.visual_odometer.visual_odometry", "utils.matcher.optical_flow_cv"}
    assert ref_ma.optical_flow_cv is not orig and ref_ma.optical_flow_cv.reference is orig
    assert ref_vo.optical_flow_cv is ref_ma.optical_flow_cv and "tasks.visual_odometer.optical_flow_cv" in shim.installed()["rebound"]
    assert vo.SHIM_PYRLK is True
    # host tensors are outside the contract: the reference's own function answers
    pts, img = torch.rand(4, 2), torch.rand(1, 3, 48, 64)
    tag, args = ref_ma.optical_flow_cv(pts, pts, img, img, {"win_size": 15, "levels": 3})
    assert tag == "reference" and args[0] is pts and ref_ma.optical_flow_cv.fallbacks == 1
    # the contract check names the reason (its limit rules need device tensors: tests/test_gpu_pyrlk.py)
    assert shim._c_pyrlk(pts, pts, img, img, None) == "inputs are not on a HIP device"
    shim.uninstall()
    assert ref_ma.optical_flow_cv is orig and ref_vo.optical_flow_cv is orig and vo.SHIM_PYRLK is False
