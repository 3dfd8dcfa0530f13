"""Sub-pixel refinement on the device (KPB_OPT_DETECT_REFINE, csrc/detect.hip refine_kps) against its numpy restatement (tests/detect_refine_cases.py).

Expected rows are built in two steps: an UNREFINED call gives (rows, idx, n) -- what the detection tests pin to the oracle -- and refine_np is applied to
(score map, idx).  Mode 1 (quadratic): (x, y) bit for bit.  Mode 2 (softargmax): within SOFT_TOL_PX of the float64 restatement, in pixels.  In both modes the
score, idx, n and the row order are exactly the unrefined call's."""
import ctypes

import numpy as np
import pytest
import torch

import detect_refine_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = {1: "quadratic", 2: "softargmax"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _detect(maps, prm, signed, refine=None):
    from keypoint_bench_amd.utils.extracter import detection_batch
    x = torch.tensor(maps)[:, None].to(DEV)
    kps, idx, n = detection_batch(x, dict(prm, refine=refine) if refine is not None else prm, signed=signed)
    return kps.cpu().numpy(), idx.cpu().numpy(), n.cpu().numpy()


_PLAIN = {}


def _plain(name, monkeypatch):
    """The unrefined rows of a case: computed once, shared, never written to."""
    maps, prm, signed, env = C.case(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name not in _PLAIN:
        out = _detect(maps, prm, signed)
        for a in out:
            a.setflags(write=False)
        _PLAIN[name] = out
    return _PLAIN[name]


def _assert_refined(maps, plain, got, mode, what):
    """got = (kps, idx, n) of a refined call on maps [B, H, W]; plain = the unrefined call's."""
    (k0, i0, n0), (k1, i1, n1) = plain, got
    H, W = maps.shape[1:]
    np.testing.assert_array_equal(n1, n0, err_msg=what)
    moved, worst = 0, 0.0
    for b in range(maps.shape[0]):
        nb = int(n0[b])
        np.testing.assert_array_equal(i1[b, :nb], i0[b, :nb], err_msg="%s: idx of image %d" % (what, b))
        np.testing.assert_array_equal(_bits(k1[b, :nb, 2]), _bits(k0[b, :nb, 2]), err_msg="%s: scores of image %d" % (what, b))
        np.testing.assert_array_equal(_bits(k0[b, :nb, :2]), _bits(C.refine_np(maps[b], i0[b, :nb], H, W, 0)), err_msg="%s: the unrefined rows are not pixel centres" % what)
        if mode == 1:
            np.testing.assert_array_equal(_bits(k1[b, :nb, :2]), _bits(C.refine_np(maps[b], i0[b, :nb], H, W, 1)), err_msg="%s: (x, y) of image %d" % (what, b))
        elif mode == 2 and nb:
            d = np.abs(C.pixels(k1[b, :nb, :2], H, W) - C.pixels(C.refine_np(maps[b], i0[b, :nb], H, W, 2, np.float64), H, W))
            worst = max(worst, float(d.max()))
            assert d.max() <= C.SOFT_TOL_PX, "%s: image %d row %d is %.3g px from the float64 restatement" % (what, b, int(d.max(axis=1).argmax()), d.max())
        else:
            np.testing.assert_array_equal(_bits(k1[b, :nb, :2]), _bits(k0[b, :nb, :2]), err_msg="%s: mode 0 moved image %d" % (what, b))
        moved += int((_bits(k1[b, :nb, :2]) != _bits(k0[b, :nb, :2])).any(axis=1).sum())
    if mode == 2:
        print("%s: worst |device - float64 restatement| %.3g px (SOFT_TOL_PX %.3g)" % (what, worst, C.SOFT_TOL_PX))
    assert (moved > 0) == (mode != 0), "%s: %d rows moved under mode %d" % (what, moved, mode)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(C.CASES))
def test_refined_rows_equal_the_restatement(name, mode, monkeypatch):
    maps, prm, signed, _ = C.case(name)
    plain = _plain(name, monkeypatch)
    assert plain[2].min() > 0
    _assert_refined(maps, plain, _detect(maps, prm, signed, MODES[mode]), mode, "%s, %s" % (name, MODES[mode]))


def test_mode_0_after_mode_1_gives_the_unrefined_bits_again(monkeypatch):
    from keypoint_bench_amd._lib import Context
    maps, prm, signed, _ = C.case("sorted")
    plain = _plain("sorted", monkeypatch)
    _assert_refined(maps, plain, _detect(maps, prm, signed, "quadratic"), 1, "first")
    assert Context.get(torch.device(DEV))._detect_refine == 0               # the drop-in restores the option
    for spelling in ("none", None):
        k, i, n = _detect(maps, dict(prm, refine=spelling), signed)
        _assert_refined(maps, plain, (k, i, n), 0, "mode 0 after mode 1")
    with pytest.raises(ValueError):
        _detect(maps, prm, signed, "cubic")


# ------------------------------------------------------------------------------------------------ raw calls: no index buffer, the pending call, bad values
def _raw(ctx, x, prm, sync, with_idx=True):
    """kpb_detect on a [B, 1, H, W] tensor as the options stand: (rc, kps, idx or None, n)."""
    from keypoint_bench_amd._lib import DetectParams, ptr
    B, _, H, W = x.shape
    K = min(prm["top_k"], H * W)
    p = DetectParams(prm["nms_dist"], prm["threshold"], prm["border_dist"], K, prm["min_score"])
    kps = torch.zeros((B, K, 3), dtype=torch.float32, device=x.device)
    idx = torch.zeros((B, K), dtype=torch.int32, device=x.device) if with_idx else None
    n = torch.zeros((B,), dtype=torch.int32, device=x.device)
    rc = ctx.lib.kpb_detect(ctx.handle, ptr(x), B, H, W, ctypes.byref(p), ptr(kps), ptr(idx), ptr(n), sync)
    return rc, kps, idx, n


@pytest.mark.parametrize("name", ["sorted", "select_scan"])
def test_without_an_index_buffer_the_library_carves_its_own(name, monkeypatch):
    from keypoint_bench_amd._lib import Context
    maps, prm, signed, _ = C.case(name)
    plain = _plain(name, monkeypatch)
    x = torch.tensor(maps)[:, None].to(DEV)
    ctx = Context.get(x.device)
    for mode in (1, 2):
        with ctx.detect_refine(mode):
            rc, kps, _, n = _raw(ctx, x, prm, 1, with_idx=False)
        ctx.check(rc)
        _assert_refined(maps, plain, (kps.cpu().numpy(), plain[1], n.cpu().numpy()), mode, "%s, out_idx_dev NULL, mode %d" % (name, mode))


def _ramp_case():
    """The positive ramp tests/test_gpu_detect_schedule.py uses to force extra sweeps (its premise is asserted there on the CPU): four tiled sweeps cannot decide it."""
    from test_gpu_detect_schedule import _positive_ramp
    H, W = 48, 640
    return _positive_ramp(H, W)[None], dict(nms_dist=1, threshold=0.0, border_dist=0, top_k=H * W, min_score=0.0)


@pytest.mark.parametrize("enqueued,at_check", [(1, 1), (1, 0), (0, 1)])
def test_a_pending_detection_keeps_its_mode_through_the_rewrite(enqueued, at_check, monkeypatch):
    """sync = 0 on the ramp: kpb_detect_check finds the image undecided, runs more sweeps, rewrites the rows (1) -- refined under the mode the call was ENQUEUED
    under, whatever KPB_OPT_DETECT_REFINE says by then.  (Quadratic only: the ramp is 640 wide, and SOFT_TOL_PX is worked out for the cases' widths.)"""
    from keypoint_bench_amd._lib import Context
    monkeypatch.setenv("KPB_NMS_TILED", "1")
    maps, prm = _ramp_case()
    if "ramp" not in _PLAIN:
        _PLAIN["ramp"] = _detect(maps, prm, False)
    x = torch.tensor(maps)[:, None].to(DEV)
    ctx = Context.get(x.device)
    with ctx.detect_refine(enqueued):
        rc, kps, idx, n = _raw(ctx, x, prm, 0)
        try:
            ctx.check(rc)
            ctx.set_option(ctx.OPT_DETECT_REFINE, at_check)
        finally:
            rc = ctx.lib.kpb_detect_check(ctx.handle)
    assert rc == 1, ctx.lib.kpb_last_error(ctx.handle)
    assert ctx._detect_refine == 0
    _assert_refined(maps, _PLAIN["ramp"], (kps.cpu().numpy(), idx.cpu().numpy(), n.cpu().numpy()), enqueued, "enqueued under %d, %d at the check" % (enqueued, at_check))
    counts = (ctypes.c_int32 * 1)()
    assert ctx.lib.kpb_detect_counts(ctx.handle, counts, 1) == 0 and counts[0] == int(_PLAIN["ramp"][2][0])


def test_an_invalid_value_is_refused_and_leaves_the_mode_in_force(monkeypatch):
    from keypoint_bench_amd._lib import Context
    maps, prm, signed, _ = C.case("raster_edges")
    plain = _plain("raster_edges", monkeypatch)
    x = torch.tensor(maps)[:, None].to(DEV)
    ctx = Context.get(x.device)
    with ctx.detect_refine(1):
        for bad in (3, 7, -1, 1 << 40):
            assert ctx.lib.kpb_ctx_set_option(ctx.handle, ctx.OPT_DETECT_REFINE, bad) == -1, bad      # KPB_E_INVALID
        assert b"KPB_OPT_DETECT_REFINE" in ctx.lib.kpb_last_error(ctx.handle) or b"negative" in ctx.lib.kpb_last_error(ctx.handle)
        rc, kps, idx, n = _raw(ctx, x, prm, 1)
        ctx.check(rc)
    _assert_refined(maps, plain, (kps.cpu().numpy(), idx.cpu().numpy(), n.cpu().numpy()), 1, "after the refused values")
    rc, kps, idx, n = _raw(ctx, x, prm, 1)
    ctx.check(rc)
    _assert_refined(maps, plain, (kps.cpu().numpy(), idx.cpu().numpy(), n.cpu().numpy()), 0, "after the block")


def test_one_more_launch_and_only_under_the_option(monkeypatch):
    """The default is launch for launch what it was: refine_kps appears in kpb_prof_report under modes 1 and 2 only, once per selection, beside unchanged counts."""
    from keypoint_bench_amd._lib import Context
    maps, prm, signed, _ = C.case("select_scan")
    _plain("select_scan", monkeypatch)
    ctx = Context.get(torch.device(DEV))
    reports = {}
    ctx.prof_enable(True)
    try:
        for mode in (None, "quadratic", "softargmax"):
            ctx.prof_report()
            _detect(maps, prm, signed, mode)
            reports[mode] = {k: v[0] for k, v in ctx.prof_report().items()}
    finally:
        ctx.prof_enable(False)
    assert "refine_kps" not in reports[None] and reports[None]["select_topk"] >= 1 and reports[None]["select_scan"] >= 1
    for mode in ("quadratic", "softargmax"):
        assert reports[mode] == dict(reports[None], refine_kps=reports[None]["select_topk"]), reports


# ------------------------------------------------------------------------------------------------ the 0.25 condition through the device
@pytest.mark.parametrize("mode", [1, 2])
def test_bumps_through_the_device(mode):
    H, W = C.BUMP_SHAPE
    s = C.bump_map()
    prm = dict(nms_dist=4, threshold=0.5, border_dist=0, top_k=100, min_score=0.0)
    kps, idx, n = _detect(s[None], prm, False, MODES[mode])
    assert int(n[0]) == 24
    ratios = C.bump_ratios(kps[0, :24, :2], idx[0, :24])
    print("mode %d worst ratio %.4f" % (mode, ratios.max()))
    assert ratios.max() <= 0.25


# ------------------------------------------------------------------------------------------------ the Python layers
def test_pipeline_runner_and_drop_in_read_the_key():
    """Two 64 x 96 synthetic pairs under refine: quadratic.  PairPipeline's keypoints and matched rows are the drop-in functions' (detection with the key, then
    brute_force_matcher); the runner's repeatability rows -- mean_error is a localisation metric -- are the same bits on its single-pair and batched paths, and
    not those of the same config without the key."""
    from keypoint_bench_amd import runner, synthetic
    from keypoint_bench_amd.models.ALike import alike_t
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import brute_force_matcher
    B, H, W = 2, 64, 96
    ep = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
    on = dict(ep, refine="quadratic")
    bf = dict(metric="euclidean", max_distance=5, cross_check=True)
    v = [synthetic.image_pair(100 + i, H, W) for i in range(B)]
    i0, i1 = np.stack([a for a, _ in v]), np.stack([b for _, b in v])
    pipe = PairPipeline(alike_t(dense_descriptors=True).eval(), on, bf, B, H, W, device=DEV)
    assert pipe.refine == 1
    pipe.run(torch.from_numpy(np.concatenate([i0, i1])).to(DEV))
    single = alike_t(dense_descriptors=True).eval()
    for b in range(B):
        s0, d0 = single(torch.from_numpy(i0[b])[None].to(DEV))
        s1, d1 = single(torch.from_numpy(i1[b])[None].to(DEV))
        k0, k1, p0 = detection(s0, on), detection(s1, on), detection(s0, ep)
        assert k0.shape == p0.shape and (k0[:, :2] != p0[:, :2]).any() and torch.equal(k0[:, 2], p0[:, 2])
        idx = torch.round(p0[:, 1] * H - 0.5).long() * W + torch.round(p0[:, 0] * W - 0.5).long()
        np.testing.assert_array_equal(_bits(k0[:, :2].cpu().numpy()), _bits(C.refine_np(s0[0, 0].cpu().numpy(), idx.cpu().numpy(), H, W, 1)))
        m0, m1 = brute_force_matcher(k0, k1, d0, d1, bf)
        got = pipe.pair(b)
        np.testing.assert_array_equal(_bits(got["kps0"]), _bits(k0.cpu().numpy()))
        np.testing.assert_array_equal(_bits(got["kps1"]), _bits(k1.cpu().numpy()))
        assert len(got["m0"]) > 10
        np.testing.assert_array_equal(_bits(got["m0"]), _bits(m0.cpu().numpy()))
        np.testing.assert_array_equal(_bits(got["m1"]), _bits(m1.cpu().numpy()))

    def params(e):
        return {"model_type": "Alike", "task_type": "repeatability", "Alike_params": dict(c1=8, c2=16, c3=32, c4=64, dim=64), "extractor_params": e,
                "matcher_params": {"type": "brute_force", "brute_force_params": bf}, "repeatability_params": {"th": 3}}

    hm = np.array([[1, 0, -3], [0, 1, -2], [0, 0, 1]], np.float32)
    ds = [{"image0": v[i][0], "image1": v[i][1], "dataset": "HPatches",
           "warp01_params": dict(mode="homo", homography_matrix=hm, width=np.int64(W), height=np.int64(H), resize=np.int64(W)),
           "warp10_params": dict(mode="homo", homography_matrix=np.linalg.inv(hm).astype(np.float32), width=W, height=H)} for i in range(B)]
    rows = {}
    for name, e, batch in (("on1", on, 1), ("on2", on, 2), ("off2", ep, 2)):
        r = runner.PairRunner(params(e), device=DEV, batch=batch)
        rows[name] = r.run(ds)[1]
        assert r.batched_pairs == (0 if batch == 1 else B)
    assert np.array_equal(rows["on1"].view(np.uint64), rows["on2"].view(np.uint64)), (rows["on1"], rows["on2"])
    assert (rows["on2"][:, 0] == rows["off2"][:, 0]).all() and (rows["on2"][:, 2] != rows["off2"][:, 2]).all(), rows
