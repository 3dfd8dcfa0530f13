"""GPU parity of N9 (LETNet: ALIKE-t's block 1 with the letnet_head kernel of csrc/alike.hip, through the C ABI) against the reference class's own fp32
CPU outputs with the checkpoint its tree ships (tests/golden/letnet*.npz), at five shapes: 32 x 32 (every head tile partial), 32 x 64 (not square), 64 x 96
and 96 x 160 (across block 1's and the head's tile edges) and 480 x 640; kpb_track_error against numpy; the VisualizeTrackingError task against the
reference's own chain on the reference's maps, keypoints and angles (tests/golden/letnet_track.npz); PairPipeline(track=...) and the runner's batched rows
against the single-pair path, bit for bit.

Net tolerances.  Both outputs are sigmoids.  The yardstick is the reference's own fp32-against-fp64 difference with this checkpoint at 480 x 640: 1.43e-6
on the score (its logit passes two more layers than GoodPoint's), 3.6e-7 on the map.  Measured on an MI355X against the five goldens, largest |error|
(score / map), both at 480 x 640: split-f16 build 2.24e-6 / 6.26e-7, strict-fp32 build 2.38e-6 / 5.96e-7 (at 32 x 32: 5.4e-7 / 3.6e-7 and 4.0e-7 / 2.4e-7).
The bounds are twice the larger of the two builds, 4.76e-6 / 1.25e-6, and may not exceed 7e-6, test_gpu_alike.py's bound for a sigmoid score that passes
through this same block 1 and much more.  Detection on the device's own 96 x 160 score map finds 951 keypoints at nms_dist 2 and 139 at 6, as on the
reference's map (printed, not asserted: the assertion is more than 100).

Tracker: test_gpu_lk.ATOL_PX = 1e-3 px on the points the reference itself reproduces under a one-ulp change of map 1 (`stable`), as test_gpu_lk_batch.py
holds the tracker to against the same reference class; at most CAP_PERCENT of a case's points are unstable.  kpb_track_error states its fp32 operations one
by one (include/kpb.h), so its rows are compared with that statement in numpy bit for bit, and with the float64 formula within 1e-5 px (test_letnet_cpu.py
derives that bound for coordinates up to 127; the random points here stay below 128)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights
from keypoint_bench_amd._lib import Context, KpbError, c_void_p, ptr
from letnet_fixtures import (CAP_PERCENT, SHAPES, TRACK_CASES, TRACK_DETECT, TRACK_HW, TRACK_SETS, checkpoint, load_parts, track_error32, track_error64,
                             track_params, track_views, wave_mean64)
from test_gpu_lk import ATOL_PX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK_SCORE, YARDSTICK_DESC = 1.43e-6, 3.6e-7
MEASURED_H16 = (2.24e-6, 6.26e-7)       # largest |score error|, |map error| over the five goldens, split-f16 build
MEASURED_FP32 = (2.38e-6, 5.96e-7)      # the same, strict-fp32 build
ATOL_SCORE, ATOL_DESC = 2 * max(MEASURED_H16[0], MEASURED_FP32[0]), 2 * max(MEASURED_H16[1], MEASURED_FP32[1])
assert ATOL_SCORE <= 7e-6 and ATOL_DESC <= 7e-6
ATOL_ERR_PX = 1e-5
EP = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
SHIFT = np.array([[1, 0, -3], [0, 1, -2], [0, 0, 1]], np.float32)
KPB_E_INVALID, KPB_E_WEIGHTS, KPB_E_UNSUPPORTED = -1, -6, -7


def _net():
    from keypoint_bench_amd.models.LETNet import LETNet
    net = LETNet(c1=8, c2=16, grayscale=False)
    net.load_state_dict(checkpoint())
    return net.eval()


def _alike():
    from keypoint_bench_amd.models.ALike import alike_t
    return alike_t()


@pytest.fixture(scope="module")
def net():
    return _net()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _img(seed, H, W, view=0):
    return _t(synthetic.image_pair(seed, H, W)[view])[None]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _homo(hm, H, W):
    return dict(mode="homo", homography_matrix=hm, width=np.int64(W), height=np.int64(H))


# ------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("H,W", SHAPES)
def test_letnet_against_reference_golden(net, H, W):
    g = load_parts("letnet")
    v0, _ = synthetic.image_pair(0, H, W)
    assert synthetic.checksum(v0) == str(g["%dx%d.img.sum" % (H, W)])
    score, desc = net(_t(v0)[None])
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 3, H, W) and desc.stride() == (H * W * 3, 1, W * 3, 3)
    d = desc[0].permute(1, 2, 0).cpu().numpy()
    s = score[0, 0].cpu().numpy()
    es, ed = float(np.abs(s - g["%dx%d.score" % (H, W)]).max()), float(np.abs(d - g["%dx%d.desc" % (H, W)]).max())
    print("letnet %dx%d %s: max |score error| %.3g, max |map error| %.3g"
          % (H, W, "fp32" if os.environ.get("KPB_FP32_MATRIX") == "1" else "split-f16", es, ed))
    assert 0.0 < float(d.min()) and float(d.max()) < 1.0 and 0.0 < float(s.min()) and float(s.max()) < 1.0
    assert es <= ATOL_SCORE and ed <= ATOL_DESC


# ------------------------------------------------------------------------------------------------ 2. batch, score only
def test_letnet_batch_equals_solo_and_score_only_writes_no_map(net):
    x = _t(np.stack([synthetic.image_pair(500 + i, 64, 96)[i & 1] for i in range(5)]))
    s, d = net._run(x)
    s, d = s.clone(), d.clone()
    s2, d2 = net._run(x)                                # the same batch again
    assert torch.equal(s, s2) and torch.equal(d, d2) and d.shape == (5, 64, 96, 3)
    for i in range(5):                                  # alone: a pixel's bits depend on neither tile nor batch
        si, di = net._run(x[i:i + 1].contiguous())
        assert torch.equal(si[0], s[i]), "score of image %d: max |d| = %g" % (i, (si[0] - s[i]).abs().max().item())
        assert torch.equal(di[0], d[i]), "map of image %d: max |d| = %g" % (i, (di[0] - d[i]).abs().max().item())
    assert not torch.equal(s[0], s[2])                  # (different images)
    ctx = Context.get(torch.device(DEV))
    ctx.prof_enable(True)
    try:
        ctx.prof_report()
        s3, d3 = net._run(x, want_desc=False)
        ctx.sync()
        only = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
    assert d3 is None and torch.equal(s, s3)
    assert only["letnet_head"][0] == 1 and sum(v[0] for k, v in only.items() if k.startswith("alike_block1")) == 1, only
    assert not [k for k in only if k.startswith(("alike_head", "alike_block2", "conv", "goodpoint", "edgepoint"))], only     # nothing of ALIKE's beyond block 1 runs
    # the C entry with a null map pointer, beside a sentinel-filled buffer of the map's size that it must not reach through any other argument
    sentinel = torch.full((5, 64, 96, 3), 7.0, device=DEV)
    score = torch.empty((5, 1, 64, 96), device=DEV)
    ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(x), 5, 64, 96, ptr(score), ptr(None)))
    ctx.sync()
    assert torch.equal(score, s) and bool((sentinel == 7.0).all())


# ------------------------------------------------------------------------------------------------ 3. detection on the net's own map
@pytest.mark.parametrize("nms_dist,ref_count", [(2, 951), (6, 139)])
def test_letnet_feeds_detection_and_sampling(net, nms_dist, ref_count):
    import oracle
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import sample_descriptors
    score, desc = net(_img(0, 96, 160))
    ep = dict(EP, nms_dist=nms_dist)
    kps = detection(score, ep)                          # a sigmoid: the default (non-negative) contract
    want, _ = oracle.detection(score[0, 0].cpu().numpy(), ep)
    np.testing.assert_array_equal(_bits(kps.cpu().numpy()), _bits(want))
    print("letnet 96x160 nms_dist %d: %d keypoints (the reference's own map gives %d)" % (nms_dist, kps.shape[0], ref_count))
    assert kps.shape[0] > 100
    np.testing.assert_array_equal(sample_descriptors(kps, desc).cpu().numpy(), oracle.sample(desc[0].cpu().numpy(), want))


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_a_shape_that_is_no_multiple_of_32_and_a_misaligned_map_are_refused_and_the_net_stays_usable(net):
    x = _img(0, 64, 96)
    s, d = net._run(x)
    s, d = s.clone(), d.clone()
    bad = _t(synthetic.image_pair(0, 40, 64)[0])[None]
    score = torch.full((1, 1, 40, 64), 7.0, device=DEV)
    desc = torch.full((1, 40, 64, 3), 7.0, device=DEV)
    ctx = net._ctx
    rc = ctx.lib.kpb_net_forward(net._handle, ptr(bad), 1, 40, 64, ptr(score), ptr(desc))
    assert rc == KPB_E_INVALID
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    assert "LETNet" in msg and "40x64" in msg, msg
    ctx.sync()
    assert bool((score == 7.0).all()) and bool((desc == 7.0).all())        # nothing written
    with pytest.raises(KpbError):
        net._run(bad)
    score = torch.full((1, 1, 64, 96), 7.0, device=DEV)
    room = torch.full((64 * 96 * 3 + 4,), 7.0, device=DEV)                  # a map pointer one float off a 16-byte boundary
    rc = ctx.lib.kpb_net_forward(net._handle, ptr(x), 1, 64, 96, ptr(score), c_void_p(room.data_ptr() + 4))
    assert rc == KPB_E_INVALID
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    assert "LETNet" in msg and "16-byte" in msg, msg
    ctx.sync()
    assert bool((score == 7.0).all()) and bool((room == 7.0).all())
    s2, d2 = net._run(x)
    assert torch.equal(s, s2) and torch.equal(d, d2)


def _create(arch, tensors, blob_arch=None):
    ctx = Context.get(torch.device(DEV))
    blob = weights.pack(tensors, arch if blob_arch is None else blob_arch)
    h = c_void_p()
    rc = ctx.lib.kpb_net_create(ctx.handle, arch, blob, len(blob), ctypes.byref(h))
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    if h.value:
        ctx.lib.kpb_net_destroy(h)
    return rc, msg, bool(h.value)


def test_create_refuses_missing_misshaped_and_foreign_blobs(net):
    from goodpoint_fixtures import checkpoint as goodpoint_checkpoint
    L, G, A = weights.ARCH_LETNET, weights.ARCH_GOODPOINT, weights.ARCH_ALIKE
    t = weights.fold_letnet(checkpoint())
    rc, msg, made = _create(L, {k: v for k, v in t.items() if k != "let.head.w"})
    assert rc == KPB_E_WEIGHTS and not made and "let.head.w" in msg and "LETNet" in msg, msg
    rc, msg, made = _create(L, dict(t, **{"let.conv1.w": t["let.conv1.w"][:8]}))
    assert rc == KPB_E_WEIGHTS and not made and "let.conv1.w" in msg and "LETNet" in msg, msg
    rc, msg, made = _create(L, dict(t, **{"b1c2.w": t["b1c2.w"][:, :4]}))
    assert rc == KPB_E_WEIGHTS and not made and "b1c2.w" in msg and "LETNet" in msg, msg
    alike, good = weights.load_alike_t(), weights.fold_goodpoint(goodpoint_checkpoint())
    for arch, tensors, names in ((L, alike, ("let.conv1.w", "LETNet")), (L, good, ("let.conv1.w", "LETNet")),       # block 1 is there, the head is not
                                 (A, t, ("b2c1.w",)), (G, t, ("gp.desc.w", "GoodPoint"))):                        # and the reverse
        rc, msg, made = _create(arch, tensors)
        assert rc == KPB_E_WEIGHTS and not made and all(n in msg for n in names), (arch, msg)
    for blob_arch, arch, tensors in ((A, L, alike), (G, L, good), (L, A, t), (L, G, t), (L, A, alike), (L, G, good)):      # a blob under another net's arch id
        rc, msg, made = _create(arch, tensors, blob_arch)
        assert rc == KPB_E_WEIGHTS and not made, (blob_arch, arch, msg)
    rc, msg, made = _create(L, t)                       # the intact one is created on the same context
    assert rc == 0 and made, msg


# ------------------------------------------------------------------------------------------------ 5. strict fp32
@pytest.mark.timeout(300)
def test_letnet_strict_fp32_kernels_pass_the_goldens():
    """KPB_FP32_MATRIX is read once per process: tests 1 and 2 again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_letnet.py::test_letnet_against_reference_golden",
           "tests/test_gpu_letnet.py::test_letnet_batch_equals_solo_and_score_only_writes_no_map"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=250)
    tail = "\n".join(p.stdout.splitlines()[-25:])
    print(tail)
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % tail
    assert "6 passed" in tail and "skipped" not in tail.split("passed")[-1], tail


# ------------------------------------------------------------------------------------------------ 6. kpb_track_error
def _track_error(kps01, tracked, n, scale, err, mean, batch=None, max_n=None, stride=None):
    ctx = Context.get(torch.device(DEV))
    B, K = kps01.shape[:2]
    rc = ctx.lib.kpb_track_error(ctx.handle, ptr(kps01), kps01.shape[2] if stride is None else stride, ptr(tracked), B if batch is None else batch,
                                 K if max_n is None else max_n, ptr(n), ptr(scale), ptr(err), ptr(mean))
    ctx.sync()
    return rc, ctx.lib.kpb_last_error(ctx.handle).decode()


def test_track_error_against_numpy_counts_sentinels_and_refusals():
    rng = np.random.default_rng(77)
    B, K = 3, 70                                        # max_n past one wave
    counts = (0, 1, 70)
    k01 = rng.uniform(0.0, 1.0, size=(B, K, 3)).astype(np.float32)          # (x, y, score) rows: a stride of 3
    trk = (k01[:, :, :2] * np.array([127, 95], np.float32) + rng.normal(0, 4.0, size=(B, K, 2))).astype(np.float32)
    scl = np.array([[127, 95], [127, 95], [63, 31]], np.float32)
    a, b, s, n = _t(k01), _t(trk), _t(scl), _t(np.array(counts, np.int32))
    err = torch.full((B, K), 7.0, device=DEV)
    mean = torch.full((B,), 7.0, dtype=torch.float64, device=DEV)
    rc, msg = _track_error(a, b, n, s, err, mean)
    assert rc == 0, msg
    e, m = err.cpu().numpy(), mean.cpu().numpy()
    assert np.isnan(m[0]) and bool((e[0] == 7.0).all())                     # n = 0: NaN like torch.mean of nothing, no row
    for j, c in enumerate(counts):
        assert bool((e[j, c:] == 7.0).all()), j                             # rows past n keep their sentinel
        if c:
            w32, w64 = track_error32(k01[j, :c], trk[j, :c], scl[j]), track_error64(k01[j, :c], trk[j, :c], scl[j])
            assert np.array_equal(_bits(e[j, :c]), _bits(w32)), (j, np.abs(e[j, :c] - w32).max())
            assert float(np.abs(e[j, :c] - w64).max()) <= ATOL_ERR_PX
            assert _bits(m[j:j + 1])[0] == _bits(np.array([wave_mean64(e[j, :c])]))[0], (j, m[j], wave_mean64(e[j, :c]))
            assert abs(m[j] - w64.mean()) <= ATOL_ERR_PX
    for j, c in enumerate(counts):                      # every pair alone gives the bits it gives in the batch
        e1 = torch.full((1, K), 7.0, device=DEV)
        m1 = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
        rc, msg = _track_error(a[j:j + 1].contiguous(), b[j:j + 1].contiguous(), n[j:j + 1].contiguous(), s[j:j + 1].contiguous(), e1, m1)
        assert rc == 0, msg
        assert np.array_equal(_bits(e1.cpu().numpy()[0]), _bits(e[j])) and np.array_equal(_bits(m1.cpu().numpy()), _bits(m[j:j + 1])), j
    e2 = torch.full((B, K), 7.0, device=DEV)            # n_dev = NULL means max_n
    m2 = torch.full((B,), 7.0, dtype=torch.float64, device=DEV)
    rc, msg = _track_error(a, b, None, s, e2, m2)
    assert rc == 0, msg
    e2, m2 = e2.cpu().numpy(), m2.cpu().numpy()
    for j in range(B):
        assert np.array_equal(_bits(e2[j]), _bits(track_error32(k01[j], trk[j], scl[j])))
        assert _bits(m2[j:j + 1])[0] == _bits(np.array([wave_mean64(e2[j])]))[0]
    assert np.array_equal(_bits(e2[2]), _bits(e[2])) and _bits(m2[2:3])[0] == _bits(m[2:3])[0]       # n = max_n either way
    # refusals write nothing
    e3 = torch.full((B, K), 7.0, device=DEV)
    m3 = torch.full((B,), 7.0, dtype=torch.float64, device=DEV)
    for kw, code in ((dict(stride=1), KPB_E_INVALID), (dict(batch=0), KPB_E_INVALID), (dict(max_n=-1), KPB_E_INVALID), (dict(batch=65536), KPB_E_UNSUPPORTED)):
        rc, msg = _track_error(a, b, n, s, e3, m3, **kw)
        assert rc == code and msg.startswith("kpb_track_error:"), (kw, rc, msg)
    ctx = Context.get(torch.device(DEV))
    for args in ((None, b, s, e3, m3), (a, None, s, e3, m3), (a, b, None, e3, m3), (a, b, s, None, m3), (a, b, s, e3, None)):
        k_, t_, s_, e_, m_ = args
        rc = ctx.lib.kpb_track_error(ctx.handle, ptr(k_), 3, ptr(t_), B, K, ptr(n), ptr(s_), ptr(e_), ptr(m_))
        assert rc == KPB_E_INVALID and ctx.lib.kpb_last_error(ctx.handle).decode().startswith("kpb_track_error:")
    assert ctx.lib.kpb_track_error(None, ptr(a), 3, ptr(b), B, K, ptr(n), ptr(s), ptr(e3), ptr(m3)) == KPB_E_INVALID
    ctx.sync()
    assert bool((e3 == 7.0).all()) and bool((m3 == 7.0).all())
    rc, msg = _track_error(a, b, n, s, e3, m3)          # and the context stays usable
    assert rc == 0 and np.array_equal(_bits(e3.cpu().numpy()), _bits(e)), msg


# ------------------------------------------------------------------------------------------------ 7. the task on the reference's maps, keypoints and angles
def _task_params(of, ep=TRACK_DETECT):
    return {"extractor_params": ep, "matcher_params": {"type": "optical_flow", "optical_flow_params": of}}


@pytest.mark.parametrize("case", [c[0] for c in TRACK_CASES])
@pytest.mark.parametrize("name", TRACK_SETS)
def test_task_on_the_reference_maps_keypoints_and_angles(monkeypatch, case, name):
    from keypoint_bench_amd.tasks.VisualizeTrackingError import visualize_tracking_error
    from keypoint_bench_amd.utils import extracter, matcher
    from keypoint_bench_amd.utils.projection import warp
    g = load_parts("letnet_track")
    H, W = TRACK_HW
    c, k = case + ".", "%s.%s_" % (case, name)
    kps, m0, m1 = _t(g[c + "kps"]), _t(g[c + "map0"])[None], _t(g[c + "map1"])[None]
    monkeypatch.setattr(extracter, "detection", lambda score, params=None: kps)          # the reference's keypoints in place of a detection
    warp01 = _homo(_t(g[c + "h01"]), H, W)
    _, _, ids, _ = warp(kps, warp01)
    assert np.array_equal(ids.cpu().numpy(), g[c + "ids"])                               # the kept ids equal the reference's
    img0 = torch.empty((1, 3, H, W), device=DEV)
    r = visualize_tracking_error(0, img0, torch.empty((1, 1, H, W), device=DEV), m0, m1, _task_params(track_params(g, case, name)), warp01,
                                 random_angle=_t(g[k + "angle"]))
    assert set(r) == {"track_error", "kps0", "kps1", "kps01"} and r["kps1"].shape == (1, ids.shape[0], 2)
    np.testing.assert_allclose(r["kps0"].cpu().numpy(), g[c + "kps0"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["kps01"].cpu().numpy(), g[c + "kps01"], rtol=0, atol=1e-6)
    scale = _t(np.array([[W - 1, H - 1]], np.float32))
    err, mean = matcher.track_error(r["kps01"][None], r["kps1"], scale)
    out, err, stable = r["kps1"][0].cpu().numpy(), err[0].cpu().numpy(), g[k + "stable"]
    assert 100 * int((~stable).sum()) <= CAP_PERCENT * stable.size
    dp, de = np.abs(out - g[k + "out"])[stable].max(), np.abs(err - g[k + "err"])[stable].max()
    print("%s %s stable %d/%d: device chain vs reference %.3g px (err %.3g); ATOL_PX %g; mean %.6f (reference, all points: %.6f)"
          % (case, name, stable.sum(), stable.size, dp, de, ATOL_PX, float(r["track_error"]), float(g[k + "mean"])))
    np.testing.assert_allclose(out[stable], g[k + "out"][stable], rtol=0, atol=ATOL_PX)
    np.testing.assert_allclose(err[stable], g[k + "err"][stable], rtol=0, atol=ATOL_PX)
    got = np.array([float(r["track_error"])])
    assert r["track_error"].dtype == torch.float64 and _bits(got)[0] == _bits(mean.cpu().numpy())[0] == _bits(np.array([wave_mean64(err)]))[0]
    assert abs(got[0] - err.astype(np.float64).mean()) <= 1e-12 * max(1.0, got[0])      # the float64 mean of the device's own per-point errors


def test_task_without_a_warp_tracks_kps0_onto_itself_and_other_matchers_are_refused(net):
    from keypoint_bench_amd.tasks.VisualizeTrackingError import visualize_tracking_error
    x = _img(300, 96, 128)
    s, d = net(x)
    prm = _task_params(dict(distance=0, win_size=7, levels=2, interation=20, gray=False))
    for warp01 in (None, {}):
        r = visualize_tracking_error(0, x, s, d, d, prm, warp01)
        assert r["kps01"] is None and r["kps0"].shape[1] == 3 and r["kps0"].shape[0] > 20 and float(r["track_error"]) == 0.0
        assert r["kps1"].shape == (1, r["kps0"].shape[0], 2)
    with pytest.raises(NotImplementedError, match="optical_flow"):
        visualize_tracking_error(0, x, s, d, d, dict(prm, matcher_params={"type": "brute_force"}), None)


# ------------------------------------------------------------------------------------------------ 8. PairPipeline(track=...)
def _pairs(n, H, W):
    """n - 1 translations (the second view of image_pair is the first moved by (3, 2)) and one viewpoint pair."""
    out = [synthetic.image_pair(100 + i, H, W) + (SHIFT,) for i in range(n - 1)]
    return out + [synthetic.warped_pair(1, H, W, strength=1.0)]


@pytest.mark.parametrize("make", [_net, _alike], ids=["LETNet-maps", "ALIKE-frames"])
def test_pair_pipeline_track_equals_the_single_pair_task(monkeypatch, make):
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.tasks.repeatability import homography_tables
    from keypoint_bench_amd.tasks.VisualizeTrackingError import visualize_tracking_error
    from keypoint_bench_amd.utils import matcher
    B, H, W = 4, 96, 128
    of = dict(distance=3, win_size=7, levels=2, interation=20, gray=False)
    pairs = _pairs(B, H, W)
    images = _t(np.concatenate([np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])]))
    warps = [_homo(p[2], H, W) for p in pairs]
    net, solo = make(), make()
    pipe = PairPipeline(net, TRACK_DETECT, None, B, H, W, device=DEV, track=of)
    K = pipe.top_k
    angles = _t((np.random.default_rng(61).normal(size=(B, K)) * 6.28).astype(np.float32))
    pipe.enqueue(images, homography_tables(warps, torch.device(DEV))[:2], angles=angles)
    pipe.finish()
    n, n0 = pipe.trk["n"].cpu().numpy(), pipe.n.cpu().numpy()
    k0, tracked, perr, mean = pipe.trk["k0"].cpu().numpy(), pipe.tracked.cpu().numpy(), pipe.point_err.cpu().numpy(), pipe.track_mean.cpu().numpy()
    seen = []
    real = matcher.optical_flow_tensor

    def recorder(pts0, pts1, img0, img1, params=None, random_angle=None):
        seen.append((img0.clone(), img1.clone()))
        return real(pts0, pts1, img0, img1, params, random_angle=random_angle)

    monkeypatch.setattr(matcher, "optical_flow_tensor", recorder)
    prm = _task_params(of)
    for b in range(B):
        x0, x1 = images[b:b + 1], images[B + b:B + b + 1]
        s0, d0 = solo(x0)
        d0 = d0.clone() if net.tracked_maps else None
        d1 = solo(x1)[1].clone() if net.tracked_maps else None
        m0, m1 = (d0, d1) if net.tracked_maps else (x0, x1)
        r = visualize_tracking_error(b, x0, s0, m0, m1, prm, warps[b], random_angle=angles[b, :n[b]])
        assert n[b] == r["kps0"].shape[0] > 20 and n[b] <= n0[b]
        assert np.array_equal(_bits(k0[b, :n[b]]), _bits(r["kps0"].cpu().numpy()))
        assert np.array_equal(_bits(tracked[b, :n[b]]), _bits(r["kps1"][0].cpu().numpy())), (b, np.abs(tracked[b, :n[b]] - r["kps1"][0].cpu().numpy()).max())
        e, _ = matcher.track_error(r["kps01"][None], r["kps1"], pipe.trk["scale"][b:b + 1])
        assert np.array_equal(_bits(perr[b, :n[b]]), _bits(e[0].cpu().numpy()))
        assert _bits(mean[b:b + 1])[0] == _bits(np.array([float(r["track_error"])]))[0], (b, mean[b], float(r["track_error"]))
        a0, a1 = seen[-1]                               # what the tracker was handed: the net's maps, or the frames
        assert a0.shape == a1.shape == (1, 3, H, W)
        if net.tracked_maps:
            assert torch.equal(a0, d0) and torch.equal(a1, d1) and not torch.equal(a0, x0)
        else:
            assert torch.equal(a0, x0) and torch.equal(a1, x1)
    assert len(seen) == B
    if net.tracked_maps:
        assert n[B - 1] < n0[B - 1]                     # the viewpoint pair loses keypoints to the covisibility filter (the reference: 217 of 221)
    with pytest.raises(ValueError, match="warp01"):
        pipe.enqueue(images)


# ------------------------------------------------------------------------------------------------ 9. runner
def test_runner_tracking_error_rows_batched_equal_single(tmp_path):
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.models.LETNet import LETNet
    path = str(tmp_path / "letnet.pth")
    torch.save(checkpoint(), path)
    H, W = 96, 128
    ds = []
    for v0, v1, hm in _pairs(5, H, W):
        ds.append({"image0": v0, "image1": v1, "dataset": "HPatches", "warp01_params": _homo(hm, H, W),
                   "warp10_params": _homo(np.linalg.inv(hm).astype(np.float32), H, W)})
    prm = {"model_type": "LETNet", "task_type": "VisualizeTrackingError", "LETNet_params": dict(weight=path), "extractor_params": TRACK_DETECT,
           "matcher_params": {"type": "optical_flow", "optical_flow_params": dict(distance=0, win_size=7, levels=2, interation=20, gray=False)}}
    single = runner.PairRunner(prm, device=DEV, batch=1)            # distance 0: the drawn angles cannot matter
    assert isinstance(single.model, LETNet) and single.model.tracked_maps
    agg1, rows1 = single.run(ds)
    assert single.batched_pairs == 0
    batched = runner.PairRunner(prm, device=DEV, batch=4)
    agg, rowsb = batched.run(ds)
    assert batched.batched_pairs == 5
    assert np.array_equal(rows1.view(np.uint64), rowsb.view(np.uint64)), (rows1[:, :2], rowsb[:, :2])
    print("runner VisualizeTrackingError rows [track_error, tracked]: %s" % rowsb[:, :2].tolist())
    assert rowsb[:, 1].min() > 20 and np.isfinite(rowsb[:, :2]).all()
    assert agg == agg1 == {"track_error": float(np.mean(rowsb[:, 0]))}
    seq = [{"image0": ds[0]["image0"], "dataset": "TartanAir"}]    # pair datasets only
    with pytest.raises(NotImplementedError, match="VisualizeTrackingError"):
        batched.run(seq)
