"""The host side of an NMS in flight (csrc/detect.hip NmsRun): the first chunk of sweeps or rounds, the look at the status words, the further chunks,
the hand-over of the result -- under kpb_fast_nms (synchronous) and kpb_detect + kpb_detect_check (asynchronous), on both schedules (the fixed-point
sweeps and KPB_OPT_DETECT_SIGNED's rounds).  Everything is bit-exact against oracle.detection / oracle.fast_nms on the same map.

The maps are built so that one chunk cannot decide them: on the positive ramp the oracle's rounds are W/2 + H/2, a sweep runs at most 64 in-tile rounds,
the sparse tail gives up at 256, and no step advances the chain of dependent suppressions faster than one synchronous round.  The premise is asserted on
the CPU (test_ramp_premise), so the GPU tests cannot go soft.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from keypoint_bench_amd import synthetic
from test_gpu_detect_signed import _assert_rows, _bits, _early_map, _prm, _ramp, _t

gpu = pytest.mark.gpu


def _positive_ramp(H, W):
    """All values > 0 and distinct; every round uncovers one more maximum down the slope."""
    y, x = np.mgrid[0:H, 0:W]
    return ((1 + x + 0.37 * y) / np.float32(W + H + 1)).astype(np.float32)


_ORACLE = {}


def _ramp_nms(H, W):
    """(map, oracle's NMS map, oracle's rounds) of the positive ramp at nms_dist 1: computed once, shared, never written to."""
    if (H, W) not in _ORACLE:
        s = _positive_ramp(H, W)
        m, rounds = oracle.fast_nms(s, 1)
        _ORACLE[(H, W)] = (s, m, rounds)
    return _ORACLE[(H, W)]


def _detect_async(ctx, x, nms_dist, signed):
    """kpb_detect(sync=0) on a [B, 1, H, W] tensor with top_k = H * W, border 0: (rc, prm, kps, idx, n)."""
    from keypoint_bench_amd._lib import DetectParams, ptr
    B, _, H, W = x.shape
    prm = DetectParams(nms_dist, 0.0, 0, H * W, 0.0)
    kps = torch.empty((B, H * W, 3), dtype=torch.float32, device=x.device)
    idx = torch.empty((B, H * W), dtype=torch.int32, device=x.device)
    n = torch.empty((B,), dtype=torch.int32, device=x.device)
    with ctx.detect_signed(signed):
        rc = ctx.lib.kpb_detect(ctx.handle, ptr(x), B, H, W, ctypes.byref(prm), ptr(kps), ptr(idx), ptr(n), 0)
    return rc, prm, kps, idx, n


def _counts(ctx, batch):
    n = (ctypes.c_int32 * batch)()
    return ctx.lib.kpb_detect_counts(ctx.handle, n, batch), list(n)


# ------------------------------------------------------------------------------------------------ CPU
def test_ramp_premise():
    """More rounds than four sweeps (4 x 64) or the tail (256) can run at 48 x 640, more than six sweeps (6 x 64) at 48 x 832; and the signed ramp of
    test_gpu_detect_signed needs more than the first group of eight."""
    assert (_positive_ramp(48, 640) > 0).all() and np.unique(_positive_ramp(48, 640)).size == 48 * 640
    assert _ramp_nms(48, 640)[2] > 256          # measured: 344
    assert _ramp_nms(48, 832)[2] > 384          # measured: 440
    assert oracle.fast_nms(_ramp(40, 72), 1)[1] > 8         # measured: 34


# ------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("tiled", ["1", "0"])
def test_async_check_enqueues_more_sweeps(tiled, monkeypatch):
    """The sweeps' twin of test_async_check_enqueues_more_rounds.  sync = 0 enqueues the opening only -- four tiled sweeps ("1"), or sweep 0 and the
    tail, which hits its round limit and hands over ("0"); kpb_detect_check finds the image undecided, runs more sweeps, rewrites the rows and says
    so (1)."""
    from keypoint_bench_amd._lib import Context
    monkeypatch.setenv("KPB_NMS_TILED", tiled)
    H, W = 48, 640
    s = _ramp_nms(H, W)[0]
    want, widx = oracle.detection(s, _prm(1, H=H, W=W))
    x = _t(s)
    ctx = Context.get(x.device)
    rc, _, kps, idx, n = _detect_async(ctx, x, 1, False)
    ctx.check(rc)
    rc = ctx.lib.kpb_detect_check(ctx.handle)
    assert rc == 1, ctx.lib.kpb_last_error(ctx.handle)
    nb = int(n[0])
    _assert_rows(kps[0, :nb].cpu().numpy(), want, "rows after the extra sweeps")
    np.testing.assert_array_equal(idx[0, :nb].cpu().numpy(), widx)


@gpu
@pytest.mark.parametrize("signed", [False, True])
def test_pending_detection_is_protected(signed):
    """Between kpb_detect(sync=0) and kpb_detect_check the context refuses a second detection and the counts; the check then completes the first."""
    from keypoint_bench_amd._lib import Context
    H, W = 32, 40
    s = _early_map(1, H, W) if signed else synthetic.score_uniform(1, H, W)
    want, _ = oracle.detection(s, _prm(2, H=H, W=W))
    x = _t(s)
    ctx = Context.get(x.device)
    rc, _, kps, _, n = _detect_async(ctx, x, 2, signed)
    ctx.check(rc)
    try:
        rc2 = _detect_async(ctx, x, 2, signed)[0]
        rc3, _ = _counts(ctx, 1)
    finally:
        rc = ctx.lib.kpb_detect_check(ctx.handle)
    assert rc2 == -1 and rc3 == -1
    assert rc in (0, 1), ctx.lib.kpb_last_error(ctx.handle)
    nb = int(n[0])
    _assert_rows(kps[0, :nb].cpu().numpy(), want, "rows of the first call")
    assert _counts(ctx, 1) == (0, [nb])


@gpu
@pytest.mark.parametrize("tiled", ["1", "0"])
def test_fast_nms_through_more_than_one_chunk_of_sweeps(tiled, monkeypatch):
    from keypoint_bench_amd.utils.extracter import fast_nms
    monkeypatch.setenv("KPB_NMS_TILED", tiled)
    s, want, _ = _ramp_nms(48, 832)
    got = fast_nms(_t(s), nms_dist=1)[0, 0].cpu().numpy()
    np.testing.assert_array_equal(_bits(got), _bits(want))


@gpu
def test_fast_nms_through_more_than_one_chunk_of_rounds():
    from keypoint_bench_amd.utils.extracter import fast_nms
    s = _ramp(40, 72)
    got = fast_nms(_t(s), nms_dist=1, signed=True)[0, 0].cpu().numpy()
    np.testing.assert_array_equal(_bits(got), _bits(oracle.fast_nms(s, 1)[0]))


@gpu
def test_schedules_alternate_on_one_context():
    """Sweeps, rounds, an error, rounds, a batch that takes the one-workgroup-per-image selection, rounds: nothing of the other schedule's workspace or
    status words may leak into a call, also after an error."""
    from keypoint_bench_amd._lib import Context, KpbError
    from keypoint_bench_amd.utils.extracter import detection, detection_batch

    def batch(maps, p, signed):
        x = torch.from_numpy(np.stack(maps))[:, None].to(torch.device("cuda:0"))
        kps, idx, n = detection_batch(x, p, signed=signed)
        for b, s in enumerate(maps):
            want, widx = oracle.detection(s, p)
            nb = int(n[b])
            _assert_rows(kps[b, :nb].cpu().numpy(), want, "image %d of %d, %r" % (b, len(maps), p))
            np.testing.assert_array_equal(idx[b, :nb].cpu().numpy(), widx)
        return [int(v) for v in n.cpu().numpy()]

    ctx = Context.get(torch.device("cuda:0"))
    batch([synthetic.score_uniform(20, 96, 160), synthetic.score_smooth(21, 96, 160), synthetic.score_uniform(22, 96, 160)], _prm(6, 8, top_k=300), False)
    s = _early_map(1, 32, 40)
    p = _prm(2, H=32, W=40)
    want, _ = oracle.detection(s, p)
    _assert_rows(detection(_t(s), p, signed=True).cpu().numpy(), want, "signed single")
    with pytest.raises(KpbError) as e:
        detection(_t(s), p)
    assert e.value.code == -4
    _assert_rows(detection(_t(s), p, signed=True).cpu().numpy(), want, "signed single after the error")
    n = batch([(synthetic.score_smooth if b % 2 else synthetic.score_uniform)(100 + b, 64, 96) for b in range(70)], _prm(3, 4, top_k=200), False)
    assert _counts(ctx, 70) == (0, n)
    batch([synthetic.score_uniform(3, 48, 80), _early_map(4, 48, 80), np.random.default_rng(5).uniform(-1.0, -0.1, (48, 80)).astype(np.float32)],
          _prm(4, 4, top_k=20), True)
