"""GPU parity of N10 (Key.Net: csrc/keynet.hip through the C ABI) against the reference class's own fp32 CPU score with the checkpoint its tree ships
(tests/golden/keynet*.npz), at five shapes: 16 x 16 (the smallest accepted shape, levels 13 and 10), 30 x 50 (odd levels, a multiple of nothing), 37 x 61 (odd
everywhere), 96 x 160 (several tiles) and 480 x 640; detection on the device's map against the reference's keypoints; refusals; the pipelines and the runner
against the single-pair path, bit for bit.

Tolerance.  The score is non-negative and unbounded (up to 14 400), so the yardstick is relative: per shape, `ref_err` = the reference's own
max |fp32 run - the same model in .double()| (0.003 .. 0.05, that is 4e-7 .. 3.6e-6 of the map's maximum).  The device must stay within M x ref_err, on the
border ring (the outermost 8 pixels, where the padding rules of the pyramid, the gradients and the layers act) and in the interior separately.  Measured on an
MI355X, largest max |device - reference| / ref_err over the five shapes (ring / interior):
    split-f16 MFMA triples   1.713 / 1.523      strict fp32 (KPB_FP32_MATRIX=1)   2.094 / 1.523       (all four at 37 x 61)
per shape, split-f16: 16 x 16 1.314 / -, 30 x 50 1.220 / 1.220, 96 x 160 0.413 / 0.670, 480 x 640 0.151 / 0.444; strict fp32: 1.168 / -, 1.046 / 1.046,
0.464 / 0.722, 0.142 / 0.444 (16 x 16 has no interior).  M_H16 = 4 and M_FP32 = 8 (keynet_fixtures.py) are the smallest powers of two that are at least
twice the largest ratio of their arithmetic; M_FP32 stays under the 16 above which the strict kernels would count as defective."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights
from keypoint_bench_amd._lib import Context, KpbError, c_void_p, ptr
from keynet_fixtures import (BORDER, DETECT_CAP_PERCENT, DETECT_CASES, DETECT_SHAPES, LEVELS, M_FP32, M_H16, PLAN, SHAPES, checkpoint, detect_params,
                             load_parts)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KPB_E_INVALID, KPB_E_WEIGHTS = -1, -6
SHIFT = np.array([[1, 0, -3], [0, 1, -2], [0, 0, 1]], np.float32)
EP = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)


def _net():
    from keypoint_bench_amd.models.KeyNet import KeyNet
    net = KeyNet(PLAN)
    net.load_state_dict(checkpoint())
    return net.eval()


@pytest.fixture(scope="module")
def net():
    return _net()


@pytest.fixture(scope="module")
def gold():
    return load_parts("keynet")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _homo(hm, H, W):
    return dict(mode="homo", homography_matrix=hm, width=np.int64(W), height=np.int64(H))


def _pixels(kps, H, W):
    """The set of (column, row) of detection's ((column + 0.5) / W, (row + 0.5) / H, score) rows."""
    return set(map(tuple, np.rint(np.asarray(kps, np.float64)[:, :2] * np.array([W, H]) - 0.5).astype(np.int64).tolist()))


# ------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("H,W", SHAPES)
def test_keynet_against_reference_golden(net, gold, H, W):
    tag = "%dx%d" % (H, W)
    v0, _ = synthetic.image_pair(0, H, W)
    assert synthetic.checksum(v0) == str(gold[tag + ".img.sum"])
    assert [tuple(r) for r in gold[tag + ".levels"][1:]] == list(LEVELS[(H, W)])
    score, none = net(_t(v0)[None])
    assert none is None and score.shape == (1, 1, H, W) and score.dtype == torch.float32
    s = score[0, 0].cpu().numpy()
    ref, ref_err, amax = gold[tag + ".score"], float(gold[tag + ".ref_err"]), float(gold[tag + ".amax"])
    d = np.abs(s.astype(np.float64) - ref.astype(np.float64))
    inner = np.zeros((H, W), bool)
    inner[BORDER:H - BORDER, BORDER:W - BORDER] = True
    e_ring, e_in = float(d[~inner].max()), float(d[inner].max()) if inner.any() else 0.0
    fp32 = os.environ.get("KPB_FP32_MATRIX") == "1"
    M = M_FP32 if fp32 else M_H16
    print("keynet %s %s: max |error| ring %.4g interior %.4g; ref_err %.4g (amax %.6g): ratios %.3f / %.3f, M = %d"
          % (tag, "fp32" if fp32 else "split-f16", e_ring, e_in, ref_err, amax, e_ring / ref_err, e_in / ref_err, M))
    assert np.isfinite(s).all() and float(s.min()) >= 0.0
    assert e_ring <= M * ref_err, "the border ring (outermost %d pixels) is off: %.4g > %d x %.4g" % (BORDER, e_ring, M, ref_err)
    assert e_in <= M * ref_err, "the interior is off: %.4g > %d x %.4g" % (e_in, M, ref_err)


# ------------------------------------------------------------------------------------------------ 2. batch equals solo
def test_keynet_batch_equals_solo_bit_for_bit_and_a_null_map_pointer_is_accepted(net):
    H, W = 37, 61
    x = _t(np.stack([synthetic.image_pair(500 + i, H, W)[i & 1] for i in range(3)]))
    s, d = net._run(x, want_desc=False)         # desc_out_dev = NULL
    s = s.clone()
    assert d is None and net.dim == 0 and net.desc_div == 1
    s2, _ = net._run(x, want_desc=False)
    assert torch.equal(s, s2)
    for i in range(3):                          # alone: a pixel's bits depend on neither tile nor batch
        si, _ = net._run(x[i:i + 1].contiguous(), want_desc=False)
        assert torch.equal(si[0], s[i]), "score of image %d: max |d| = %g" % (i, (si[0] - s[i]).abs().max().item())
    assert not torch.equal(s[0], s[2])          # (different images)
    sentinel = torch.full((3, H, W, 8), 7.0, device=DEV)       # a map pointer is ignored, not written through
    score = torch.empty((3, 1, H, W), device=DEV)
    ctx = net._ctx
    ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(x), 3, H, W, ptr(score), ptr(sentinel)))
    ctx.sync()
    assert torch.equal(score, s) and bool((sentinel == 7.0).all())
    with pytest.raises(KpbError):               # no descriptor map, so nothing to sample inside the net either
        ctx.check(ctx.lib.kpb_net_desc_at(net._handle, ptr(torch.zeros((4, 2), device=DEV)), 2, 4, ptr(None), ptr(torch.zeros((4, 8), device=DEV))))


# ------------------------------------------------------------------------------------------------ 3. strict fp32
@pytest.mark.timeout(300)
def test_keynet_strict_fp32_kernels_pass_the_goldens():
    """KPB_FP32_MATRIX is read once per process: tests 1 and 2 again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_keynet.py::test_keynet_against_reference_golden",
           "tests/test_gpu_keynet.py::test_keynet_batch_equals_solo_bit_for_bit_and_a_null_map_pointer_is_accepted"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=250)
    tail = "\n".join(p.stdout.splitlines()[-25:])
    print(tail)
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % tail
    assert "6 passed" in tail and "skipped" not in tail.split("passed")[-1], tail
    assert tail.count(" fp32: ") == 5, tail     # the child really ran the strict kernels


# ------------------------------------------------------------------------------------------------ 4. detection
@pytest.mark.parametrize("H,W", DETECT_SHAPES)
@pytest.mark.parametrize("nms_dist,top_k", DETECT_CASES)
def test_detection_on_the_device_map_finds_the_reference_keypoints(net, H, W, nms_dist, top_k):
    from keypoint_bench_amd.utils.extracter import detection
    want = load_parts("keynet_detect")["%dx%d.nd%d.k%d" % (H, W, nms_dist, top_k)]
    score, _ = net(_t(synthetic.image_pair(0, H, W)[0])[None])
    kps = detection(score, detect_params(nms_dist, top_k)).cpu().numpy()
    a, b = _pixels(kps, H, W), _pixels(want, H, W)
    diff = len(a ^ b)
    print("keynet detect %dx%d nms_dist %d top_k %d: %d keypoints (reference %d), symmetric difference %d" % (H, W, nms_dist, top_k, len(a), len(b), diff))
    assert len(b) == want.shape[0] and len(a) == kps.shape[0]
    assert 100 * diff <= DETECT_CAP_PERCENT * len(b)


@pytest.mark.parametrize("H,W", DETECT_SHAPES)
@pytest.mark.parametrize("nms_dist,top_k", DETECT_CASES)
def test_detection_on_the_reference_map_equals_the_reference_keypoints(gold, H, W, nms_dist, top_k):
    """A guard: scores of 10^2 .. 10^4 lie far above the [2^-62, 4) range of nms_score_bin, so every confirmed maximum falls into the last bin."""
    from keypoint_bench_amd.utils.extracter import detection
    want = load_parts("keynet_detect")["%dx%d.nd%d.k%d" % (H, W, nms_dist, top_k)]
    kps = detection(_t(gold["%dx%d.score" % (H, W)])[None, None], detect_params(nms_dist, top_k)).cpu().numpy()
    assert kps.shape == want.shape and kps.dtype == want.dtype == np.float32
    rows = lambda k: sorted(map(tuple, _bits(k).tolist()))
    assert rows(kps) == rows(want)
    if want.shape[0] == top_k:                  # cut by top_k: the reference's descending order too
        assert np.array_equal(_bits(kps), _bits(want))


# ------------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("H,W", [(15, 64), (64, 15)])
def test_a_shape_below_16_is_refused_and_the_net_stays_usable(net, H, W):
    x = _t(synthetic.image_pair(0, 32, 64)[0])[None]
    s, _ = net._run(x, want_desc=False)
    s = s.clone()
    bad = _t(synthetic.image_pair(0, H, W)[0])[None]
    score = torch.full((1, 1, H, W), 7.0, device=DEV)
    ctx = net._ctx
    rc = ctx.lib.kpb_net_forward(net._handle, ptr(bad), 1, H, W, ptr(score), ptr(None))
    assert rc == KPB_E_INVALID
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    assert "KeyNet" in msg and "%dx%d" % (H, W) in msg, msg
    ctx.sync()
    assert bool((score == 7.0).all())           # nothing written
    with pytest.raises(KpbError):
        net(bad)
    s2, _ = net._run(x, want_desc=False)
    assert torch.equal(s, s2)


def _create(arch, tensors, blob_arch=None, cut=None):
    ctx = Context.get(torch.device(DEV))
    blob = weights.pack(tensors, arch if blob_arch is None else blob_arch)
    if cut is not None:
        blob = blob[:cut]
    h = c_void_p()
    rc = ctx.lib.kpb_net_create(ctx.handle, arch, blob, len(blob), ctypes.byref(h))
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    if h.value:
        ctx.lib.kpb_net_destroy(h)
    return rc, msg, bool(h.value)


def test_create_refuses_truncated_misshaped_missing_and_foreign_blobs(net):
    from letnet_fixtures import checkpoint as letnet_checkpoint
    K, A, L = weights.ARCH_KEYNET, weights.ARCH_ALIKE, weights.ARCH_LETNET
    t = weights.fold_keynet(checkpoint())
    x = _t(synthetic.image_pair(0, 32, 64)[0])[None]
    s = net._run(x, want_desc=False)[0].clone()
    whole = len(weights.pack(t, K))
    for cut in (8, 100, whole // 2, whole - 4):
        rc, msg, made = _create(K, t, cut=cut)
        assert rc == KPB_E_WEIGHTS and not made and "malformed" in msg, (cut, msg)
    for name in ("l0.w", "l1.b", "l2.w", "last.w", "last.b"):
        rc, msg, made = _create(K, {k: v for k, v in t.items() if k != name})
        assert rc == KPB_E_WEIGHTS and not made and name in msg and "KeyNet" in msg, msg
    for name, wrong in (("l0.w", t["l0.w"][:, :8]), ("l1.w", t["l1.w"][:, :, :3, :3]), ("l2.b", t["l2.b"][:4]), ("last.w", t["last.w"][:, :16])):
        rc, msg, made = _create(K, dict(t, **{name: wrong}))
        assert rc == KPB_E_WEIGHTS and not made and name in msg and "KeyNet" in msg, msg
    alike, let = weights.load_alike_t(), weights.fold_letnet(letnet_checkpoint())
    for arch, tensors, names in ((K, alike, ("l0.w", "KeyNet")), (K, let, ("l0.w", "KeyNet")), (A, t, ("b1c1.w",)), (L, t, ("LETNet",))):
        rc, msg, made = _create(arch, tensors)
        assert rc == KPB_E_WEIGHTS and not made and all(n in msg for n in names), (arch, msg)
    for blob_arch, arch, tensors in ((A, K, alike), (K, A, t), (K, L, t), (L, K, let)):       # a blob under another net's arch id
        rc, msg, made = _create(arch, tensors, blob_arch)
        assert rc == KPB_E_WEIGHTS and not made, (blob_arch, arch, msg)
    rc, msg, made = _create(K, t)               # the intact one is created on the same context
    assert rc == 0 and made, msg
    assert torch.equal(net._run(x, want_desc=False)[0], s)


# ------------------------------------------------------------------------------------------------ 6. pipelines
def _pairs(n, H, W):
    return [synthetic.warped_pair(1 + i, H, W, strength=1.0) for i in range(n)]


def test_pair_pipeline_without_matching_equals_the_single_pair_repeatability_rows():
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.pipeline import PairPipeline
    B, H, W = 2, 96, 128
    pairs = _pairs(B, H, W)
    images = _t(np.concatenate([np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])]))
    items = [{"warp01_params": _homo(p[2], H, W), "warp10_params": _homo(np.linalg.inv(p[2]).astype(np.float32), H, W)} for p in pairs]
    prm = {"extractor_params": EP, "repeatability_params": {"th": 3}}
    pipe = PairPipeline(_net(), EP, dict(metric="euclidean", max_distance=float("inf"), cross_check=True), B, H, W, device=DEV, match=False)
    assert pipe.desc is None and pipe.C == 0
    pipe.run(images)
    rows = runner._batched_repeatability(pipe, items, prm)
    solo = _net()
    for b in range(B):
        x0, x1 = images[b:b + 1], images[B + b:B + b + 1]
        s0, s1 = solo(x0)[0].clone(), solo(x1)[0].clone()
        want = runner.repeatability_row(b, x0, s0, None, x1, s1, None, items[b]["warp01_params"], items[b]["warp10_params"], prm)
        got = [float(v) for v in rows[b]]
        assert np.array_equal(_bits(np.array(got)), _bits(np.array(want))), (b, got, want)
        assert want[0] > 20
    with pytest.raises(ValueError, match="KeyNet has no descriptors"):
        PairPipeline(_net(), EP, dict(metric="euclidean", max_distance=float("inf"), cross_check=True), B, H, W, device=DEV)
    from keypoint_bench_amd.pipeline import SequencePipeline
    with pytest.raises(ValueError, match="KeyNet has no descriptors"):
        SequencePipeline(_net(), EP, dict(metric="euclidean", max_distance=float("inf"), cross_check=True), 2, H, W, device=DEV)
    of = dict(distance=3, win_size=7, levels=2, interation=20, gray=False)
    seq = SequencePipeline(_net(), EP, None, 2, H, W, device=DEV, track=of)      # tracked on the frames
    seq.run(images[:2].contiguous(), first=True)
    assert int(seq.k[0]) == int(seq.n[0]) > 20 and bool(torch.isfinite(seq.tracked[0, :int(seq.k[0])]).all())


def test_single_pair_tasks_that_match_descriptors_refuse_in_the_same_words():
    from keypoint_bench_amd import runner
    H, W = 64, 96
    v0, v1, hm = synthetic.warped_pair(1, H, W, strength=1.0)
    item = {"image0": v0, "image1": v1, "warp01_params": _homo(hm, H, W), "warp10_params": _homo(np.linalg.inv(hm).astype(np.float32), H, W)}
    for task in ("MHA", "AUC", "match_stats", "FundamentalMatrixRansac"):
        r = runner.PairRunner({"model_type": "KeyNet", "task_type": task, "extractor_params": EP,
                               "matcher_params": {"type": "brute_force", "brute_force_params": dict(metric="euclidean", max_distance=5, cross_check=True)}},
                              model=_net(), device=DEV, batch=1)
        with pytest.raises(ValueError, match="KeyNet has no descriptors"):
            r.test_step(item, 0)


def test_pair_pipeline_track_equals_the_single_pair_task():
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.tasks.repeatability import homography_tables
    from keypoint_bench_amd.tasks.VisualizeTrackingError import visualize_tracking_error
    from keypoint_bench_amd.utils import matcher
    B, H, W = 2, 96, 128
    of = dict(distance=3, win_size=7, levels=2, interation=20, gray=False)
    pairs = [synthetic.image_pair(100, H, W) + (SHIFT,), synthetic.warped_pair(1, H, W, strength=1.0)]
    images = _t(np.concatenate([np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])]))
    warps = [_homo(p[2], H, W) for p in pairs]
    net, solo = _net(), _net()
    assert net.tracked_maps is False
    pipe = PairPipeline(net, EP, None, B, H, W, device=DEV, track=of)
    K = pipe.top_k
    angles = _t((np.random.default_rng(61).normal(size=(B, K)) * 6.28).astype(np.float32))
    pipe.enqueue(images, homography_tables(warps, torch.device(DEV))[:2], angles=angles)
    pipe.finish()
    n = pipe.trk["n"].cpu().numpy()
    k0, tracked, perr, mean = pipe.trk["k0"].cpu().numpy(), pipe.tracked.cpu().numpy(), pipe.point_err.cpu().numpy(), pipe.track_mean.cpu().numpy()
    prm = {"extractor_params": EP, "matcher_params": {"type": "optical_flow", "optical_flow_params": of}}
    for b in range(B):
        x0, x1 = images[b:b + 1], images[B + b:B + b + 1]
        s0, none = solo(x0)
        assert none is None
        r = visualize_tracking_error(b, x0, s0, x0, x1, prm, warps[b], random_angle=angles[b, :n[b]])      # the frames are tracked
        assert n[b] == r["kps0"].shape[0] > 20
        assert np.array_equal(_bits(k0[b, :n[b]]), _bits(r["kps0"].cpu().numpy()))
        assert np.array_equal(_bits(tracked[b, :n[b]]), _bits(r["kps1"][0].cpu().numpy())), (b, np.abs(tracked[b, :n[b]] - r["kps1"][0].cpu().numpy()).max())
        e, _ = matcher.track_error(r["kps01"][None], r["kps1"], pipe.trk["scale"][b:b + 1])
        assert np.array_equal(_bits(perr[b, :n[b]]), _bits(e[0].cpu().numpy()))
        assert _bits(mean[b:b + 1])[0] == _bits(np.array([float(r["track_error"])]))[0], (b, mean[b], float(r["track_error"]))


# ------------------------------------------------------------------------------------------------ 7. runner
def test_runner_repeatability_rows_batched_equal_single(tmp_path):
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.models.KeyNet import KeyNet
    path = str(tmp_path / "keynet_pytorch.pth")
    torch.save({"state_dict": checkpoint(), "optimizer": {}}, path)
    H, W = 96, 128
    ds = []
    for v0, v1, hm in _pairs(3, H, W):
        ds.append({"image0": v0, "image1": v1, "dataset": "HPatches", "warp01_params": _homo(hm, H, W),
                   "warp10_params": _homo(np.linalg.inv(hm).astype(np.float32), H, W)})
    prm = {"model_type": "KeyNet", "task_type": "repeatability", "KeyNet_params": dict(PLAN, weight=path), "extractor_params": EP,
           "matcher_params": {"type": "brute_force", "brute_force_params": dict(metric="euclidean", max_distance=5, cross_check=True)},
           "repeatability_params": {"th": 3}}
    single = runner.PairRunner(prm, device=DEV, batch=1)
    assert isinstance(single.model, KeyNet) and single.model.dim == 0
    _, rows1 = single.run(ds)
    assert single.batched_pairs == 0
    batched = runner.PairRunner(prm, device=DEV, batch=4)
    agg, rowsb = batched.run(ds)
    assert batched.batched_pairs == 3
    assert np.array_equal(rows1.view(np.uint64), rowsb.view(np.uint64)), (rows1, rowsb)
    print("runner repeatability rows [num_feat, repeatability, mean_error]: %s" % rowsb[:, :3].tolist())
    assert rowsb[:, 0].min() > 20 and np.isfinite(agg["repeatability"])
