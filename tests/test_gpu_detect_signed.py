"""KPB_OPT_DETECT_SIGNED (include/kpb.h; csrc/detect.hip nms_round): detection on SIGNED score maps by the reference's own synchronous rounds, which stop
as soon as the number of window maxima repeats (utils/extracter.py:49-98).  Everything is bit-exact against oracle.detection / oracle.fast_nms, the
literal restatement of that loop, on the same map.

Why clamping at zero is not enough: negative maxima are counted in round 0 only and zero maxima come and go, and both feed the count the stop rule
compares -- at the five EARLY_STOP cases below the loop on the signed map stops one round before the loop on max(map, 0) and keeps more keypoints.  The
premise is asserted on the CPU (test_early_stop_premise), so the GPU test cannot go soft if a case ever stops differing.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from keypoint_bench_amd import synthetic

gpu = pytest.mark.gpu

# (seed, H, W): uniform(-0.5, 0.5) - 0.3, nms_dist 1, threshold 0, top_k unlimited
EARLY_STOP = [(2, 64, 96), (5, 40, 56), (32, 32, 32), (44, 32, 32), (56, 32, 32)]
SHAPES = [(32, 32), (24, 72), (40, 56), (64, 96), (96, 416)]
RADII = [1, 2, 4, 6, 8, 9, 16]
KINDS = ["uniform", "shifted", "smooth"]


def _early_map(seed, H, W):
    return (np.random.default_rng(seed).uniform(-0.5, 0.5, (H, W)).astype(np.float32) - 0.3).astype(np.float32)


def _map(kind, seed, H, W):
    if kind == "uniform":
        return np.random.default_rng(seed).uniform(-0.5, 0.5, (H, W)).astype(np.float32)
    if kind == "shifted":
        return _early_map(seed, H, W)
    return (synthetic.score_smooth(seed, H, W) - np.float32(0.5)).astype(np.float32)


def _ramp(H, W):
    """A slope: every round uncovers one more maximum down the slope, so the count keeps changing for dozens of rounds."""
    y, x = np.mgrid[0:H, 0:W]
    return ((x + 0.37 * y) / np.float32(W + H) - 0.4).astype(np.float32)


def _prm(nms_dist, border=0, top_k=None, threshold=0.0, H=0, W=0):
    return dict(nms_dist=nms_dist, threshold=threshold, border_dist=border, top_k=H * W if top_k is None else top_k, min_score=0.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev():
    return torch.device("cuda:0")


def _t(s):
    return torch.from_numpy(np.ascontiguousarray(s))[None, None].to(_dev())


def _assert_rows(got, want, what):
    assert got.shape == want.shape, "%s: %d rows, oracle %d" % (what, got.shape[0], want.shape[0])
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("seed,H,W", EARLY_STOP)
def test_early_stop_premise(seed, H, W):
    s = _early_map(seed, H, W)
    p = _prm(1, H=H, W=W)
    ks, _ = oracle.detection(s, p)
    kc, _ = oracle.detection(np.maximum(s, 0), p)
    assert ks.shape[0] > kc.shape[0], "the signed loop no longer stops early here: (%d, %dx%d) has stopped being a counter-example" % (seed, H, W)
    ms, rs = oracle.fast_nms(s, 1)
    mc, rc = oracle.fast_nms(np.maximum(s, 0), 1)
    assert rs == rc - 1
    assert not np.array_equal(np.maximum(ms, 0), mc)


def test_ramp_needs_many_rounds():
    """The premise of test_async_check_enqueues_more_rounds: the first group of launches (eight) cannot decide this map."""
    _, rounds = oracle.fast_nms(_ramp(40, 72), 1)
    assert rounds > 12


# ------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("seed,H,W", EARLY_STOP)
def test_early_stop_cases(seed, H, W):
    from keypoint_bench_amd.utils.extracter import detection, fast_nms
    s = _early_map(seed, H, W)
    p = _prm(1, H=H, W=W)
    want, _ = oracle.detection(s, p)
    got = detection(_t(s), p, signed=True).cpu().numpy()
    _assert_rows(got, want, "signed rows")
    clamped = detection(_t(np.maximum(s, 0)), p).cpu().numpy()          # the default path on the clamped map: another function
    _assert_rows(clamped, oracle.detection(np.maximum(s, 0), p)[0], "clamped rows")
    assert clamped.shape[0] < got.shape[0]
    m = fast_nms(_t(s), nms_dist=1, signed=True)[0, 0].cpu().numpy()
    np.testing.assert_array_equal(_bits(m), _bits(oracle.fast_nms(s, 1)[0]))
    mc = fast_nms(_t(np.maximum(s, 0)), nms_dist=1)[0, 0].cpu().numpy()
    assert not np.array_equal(np.maximum(m, 0), mc)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_sweep(H, W, kind):
    from keypoint_bench_amd.utils.extracter import detection, fast_nms
    s = _map(kind, 7 + H + W, H, W)
    d = _t(s)
    for r in RADII:
        m = fast_nms(d, nms_dist=r, signed=True)[0, 0].cpu().numpy()
        np.testing.assert_array_equal(_bits(m), _bits(oracle.fast_nms(s, r)[0]), err_msg="map r=%d" % r)
        for border in (0, 8):
            p = _prm(r, border, H=H, W=W)
            want, _ = oracle.detection(s, p)
            _assert_rows(detection(d, p, signed=True).cpu().numpy(), want, "r=%d border=%d top_k>=N" % (r, border))
            n = want.shape[0]
            if n >= 2:      # top_k below N: the sorted form
                p = _prm(r, border, top_k=n // 2)
                _assert_rows(detection(d, p, signed=True).cpu().numpy(), oracle.detection(s, p)[0], "r=%d border=%d top_k=%d<N" % (r, border, n // 2))


@gpu
@pytest.mark.parametrize("r", [1, 2, 6])
def test_quantised_map_ties_and_zeros(r):
    """floor(8 s) / 8: heavy ties, exact zeros and -0.0 (a zero, not a negative).  top_k >= N: raster order, no tie rule of the sort involved."""
    from keypoint_bench_amd.utils.extracter import detection, fast_nms
    H, W = 40, 88
    rng = np.random.default_rng(91)
    s = (np.floor(rng.uniform(-0.5, 0.5, (H, W)).astype(np.float32) * 8) / 8).astype(np.float32)
    s[(s == 0) & (rng.random((H, W)) < 0.5)] = np.float32(-0.0)
    assert (s == 0).sum() > 100 and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all()
    p = _prm(r, H=H, W=W)
    _assert_rows(detection(_t(s), p, signed=True).cpu().numpy(), oracle.detection(s, p)[0], "quantised")
    m = fast_nms(_t(s), nms_dist=r, signed=True)[0, 0].cpu().numpy()
    np.testing.assert_array_equal(_bits(m), _bits(oracle.fast_nms(s, r)[0]))


@gpu
def test_batch_of_three_equals_single_calls():
    from keypoint_bench_amd.utils.extracter import detection, detection_batch, fast_nms
    H, W = 48, 80
    maps = [synthetic.score_uniform(3, H, W), _early_map(4, H, W), np.random.default_rng(5).uniform(-1.0, -0.1, (H, W)).astype(np.float32)]
    x = torch.from_numpy(np.stack(maps))[:, None].to(_dev())
    for r, top_k in ((1, H * W), (4, 20)):
        p = _prm(r, 4, top_k=top_k)
        kps, idx, n = detection_batch(x, p, signed=True)
        for b, s in enumerate(maps):
            want, widx = oracle.detection(s, p)
            nb = int(n[b])
            _assert_rows(kps[b, :nb].cpu().numpy(), want, "image %d r=%d" % (b, r))
            np.testing.assert_array_equal(idx[b, :nb].cpu().numpy(), widx)
            _assert_rows(detection(x[b:b + 1], p, signed=True).cpu().numpy(), want, "single %d" % b)
        assert int(n[2]) == 0
        m = fast_nms(x, nms_dist=r, signed=True).cpu().numpy()
        for b, s in enumerate(maps):
            np.testing.assert_array_equal(_bits(m[b, 0]), _bits(oracle.fast_nms(s, r)[0]), err_msg="map %d" % b)


@gpu
def test_async_check_enqueues_more_rounds():
    """sync = 0 enqueues the first group of rounds only; kpb_detect_check finds the image undecided, runs more, rewrites the rows and says so (1)."""
    from keypoint_bench_amd._lib import Context, DetectParams, ptr
    H, W = 40, 72
    s = _ramp(H, W)
    p = _prm(1, H=H, W=W)
    want, _ = oracle.detection(s, p)
    x = _t(s)
    ctx = Context.get(x.device)
    prm = DetectParams(1, 0.0, 0, H * W, 0.0)
    kps = torch.empty((1, H * W, 3), dtype=torch.float32, device=x.device)
    idx = torch.empty((1, H * W), dtype=torch.int32, device=x.device)
    n = torch.empty((1,), dtype=torch.int32, device=x.device)
    with ctx.detect_signed(True):
        ctx.check(ctx.lib.kpb_detect(ctx.handle, ptr(x), 1, H, W, ctypes.byref(prm), ptr(kps), ptr(idx), ptr(n), 0))
    rc = ctx.lib.kpb_detect_check(ctx.handle)       # the option is off again: the pending call keeps what it was enqueued under
    assert rc == 1, ctx.lib.kpb_last_error(ctx.handle)
    _assert_rows(kps[0, : int(n[0])].cpu().numpy(), want, "rows after the extra rounds")


@gpu
def test_option_values_and_errors():
    from keypoint_bench_amd._lib import Context, KpbError
    from keypoint_bench_amd.utils.extracter import detection, fast_nms
    s = _early_map(1, 32, 40)
    x = _t(s)
    ctx = Context.get(x.device)
    with pytest.raises(KpbError) as e:
        detection(x, _prm(2, H=32, W=40))                               # option off: a signed map is still refused
    assert e.value.code == -4
    with pytest.raises(KpbError) as e:
        fast_nms(x, nms_dist=2)
    assert e.value.code == -4
    with pytest.raises(KpbError) as e:
        detection(x, _prm(2, threshold=-0.1, H=32, W=40), signed=True)
    assert e.value.code == -7
    assert ctx._detect_signed == 0                                      # restored after the exception ...
    with pytest.raises(KpbError) as e:
        detection(x, _prm(2, H=32, W=40))                               # ... in the library too
    assert e.value.code == -4
    with pytest.raises(KpbError) as e:
        ctx.set_option(Context.OPT_DETECT_SIGNED, 2)
    assert e.value.code == -1
    # nms_dist 0 is untouched by the option: map > threshold, a negative threshold included
    p0 = _prm(0, threshold=-0.1, H=32, W=40)
    _assert_rows(detection(x, p0, signed=True).cpu().numpy(), oracle.detection(s, p0)[0], "nms_dist 0")
    # the context's own setting stands when a call does not ask
    ctx.set_option(Context.OPT_DETECT_SIGNED, 1)
    try:
        _assert_rows(detection(x, _prm(2, H=32, W=40)).cpu().numpy(), oracle.detection(s, _prm(2, H=32, W=40))[0], "option set on the context")
    finally:
        ctx.set_option(Context.OPT_DETECT_SIGNED, 0)


@gpu
@pytest.mark.parametrize("fam", ["uniform", "smooth"])
def test_non_negative_map_equals_default_path(fam):
    """On a non-negative map the count rule stops at the fixed point: asserted on the oracle (the rounds) against the default path, then on the option."""
    from keypoint_bench_amd.utils.extracter import detection, fast_nms
    gen = dict(uniform=synthetic.score_uniform, smooth=synthetic.score_smooth)[fam]
    for (H, W), r, top_k in (((64, 96), 2, 300), ((96, 160), 6, 100000)):
        s = gen(11, H, W)
        p = _prm(r, 8, top_k=top_k)
        want, _ = oracle.detection(s, p)
        default = detection(_t(s), p).cpu().numpy()
        _assert_rows(default, want, "default path against the oracle's rounds")
        _assert_rows(detection(_t(s), p, signed=True).cpu().numpy(), default, "rounds against the default path")
        np.testing.assert_array_equal(_bits(fast_nms(_t(s), nms_dist=r, signed=True).cpu().numpy()), _bits(fast_nms(_t(s), nms_dist=r).cpu().numpy()))


@gpu
def test_pipeline_honours_signed_scores():
    """PairPipeline detects with signed=net.signed_scores (sync = 0, completed by kpb_detect_check after the option is off again).  ALIKE's score is a
    sigmoid, so the rounds and the default path must give the same keypoints and matches, and the context's setting is back afterwards."""
    from keypoint_bench_amd._lib import Context
    from keypoint_bench_amd.models.ALike import alike_t
    from keypoint_bench_amd.pipeline import PairPipeline
    B, H, W = 2, 96, 128
    ep = dict(nms_dist=2, threshold=0.0, border_dist=8, top_k=200, min_score=0.0)
    bf = dict(metric="euclidean", max_distance=5, cross_check=True)
    v = [synthetic.image_pair(40 + i, H, W) for i in range(B)]
    images = torch.from_numpy(np.concatenate([np.stack([a for a, _ in v]), np.stack([b for _, b in v])])).to(_dev())
    out = []
    for flag in (False, True):
        net = alike_t(dense_descriptors=True).eval()
        net.signed_scores = flag
        pipe = PairPipeline(net, ep, bf, B, H, W, device="cuda:0")
        pipe.run(images)
        out.append([pipe.pair(b) for b in range(B)])
        assert Context.get(_dev())._detect_signed == 0
    for b in range(B):
        assert out[0][b]["kps0"].shape[0] > 20
        for key in ("kps0", "kps1", "pairs", "dist"):
            np.testing.assert_array_equal(out[0][b][key], out[1][b][key], err_msg="pair %d %s" % (b, key))
