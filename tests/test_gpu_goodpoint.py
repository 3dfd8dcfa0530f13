"""GPU parity of N8 (GoodPoint: ALIKE-t's block 1 with the goodpoint_head kernel of csrc/alike.hip, through the C ABI) against the reference class's
own fp32 CPU outputs with the checkpoint its tree ships (tests/golden/goodpoint*.npz), at five shapes: 32 x 32 (every head tile partial, every
pixel near a border), 32 x 64 (not square), 64 x 96 and 96 x 160 (across block 1's and the head's tile edges) and 480 x 640.

Tolerances.  Both outputs are sigmoids.  The yardstick is the reference's own fp32-against-fp64 difference with this checkpoint at 480 x 640:
3.0e-7 on the score, 4.1e-7 on the map.  Measured on an MI355X against the five goldens, largest |error| (score / map), both at 480 x 640: split-f16
build 4.47e-7 / 5.96e-7, strict-fp32 build 3.58e-7 / 5.36e-7 (at 32 x 32: 2.09e-7 / 2.98e-7 and 1.49e-7 / 1.79e-7).  The bounds are twice the larger
of the two builds, 8.94e-7 / 1.19e-6, and may not exceed 7e-6, test_gpu_alike.py's bound for a sigmoid score that passes through this same block 1 and
much more.  Detection on the device's own 96 x 160 score map finds 934 keypoints at nms_dist 2 and 142 at 6, as on the reference's map."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights
from keypoint_bench_amd._lib import Context, KpbError, c_void_p, ptr
from goodpoint_fixtures import PARAM, SHAPES, checkpoint, load_parts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK_SCORE, YARDSTICK_DESC = 3.0e-7, 4.1e-7
MEASURED_H16 = (4.47e-7, 5.96e-7)           # largest |score error|, |map error| over the five goldens, split-f16 build
MEASURED_FP32 = (3.58e-7, 5.36e-7)          # the same, strict-fp32 build
ATOL_SCORE, ATOL_DESC = 2 * max(MEASURED_H16[0], MEASURED_FP32[0]), 2 * max(MEASURED_H16[1], MEASURED_FP32[1])
assert ATOL_SCORE <= 7e-6 and ATOL_DESC <= 7e-6
EP = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
BF = dict(metric="euclidean", max_distance=5, cross_check=True)
KPB_E_INVALID, KPB_E_WEIGHTS = -1, -6


def _net():
    from keypoint_bench_amd.models.GoodPoint import GoodPoint
    net = GoodPoint(PARAM)
    net.load_state_dict(checkpoint())
    return net.eval()


@pytest.fixture(scope="module")
def net():
    return _net()


def _img(seed, H, W, view=0):
    return torch.from_numpy(synthetic.image_pair(seed, H, W)[view])[None].to(DEV)


# ------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("H,W", SHAPES)
def test_goodpoint_against_reference_golden(net, H, W):
    g = load_parts("goodpoint")
    v0, _ = synthetic.image_pair(0, H, W)
    assert synthetic.checksum(v0) == str(g["%dx%d.img.sum" % (H, W)])
    score, desc = net(torch.from_numpy(v0)[None].to(DEV))
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 3, H, W)
    d = desc[0].permute(1, 2, 0).cpu().numpy()
    es = float(np.abs(score[0, 0].cpu().numpy() - g["%dx%d.score" % (H, W)]).max())
    ed = float(np.abs(d - g["%dx%d.desc" % (H, W)]).max())
    print("goodpoint %dx%d %s: max |score error| %.3g, max |map error| %.3g"
          % (H, W, "fp32" if os.environ.get("KPB_FP32_MATRIX") == "1" else "split-f16", es, ed))
    assert 0.0 < float(d.min()) and float(d.max()) < 1.0
    assert es <= ATOL_SCORE and ed <= ATOL_DESC


# ------------------------------------------------------------------------------------------------ 2. batch, score only
def test_goodpoint_batch_equals_solo_and_score_only_writes_no_map(net):
    x = torch.from_numpy(np.stack([synthetic.image_pair(500 + i, 64, 96)[i & 1] for i in range(5)])).to(DEV)
    s, d = net._run(x)
    s, d = s.clone(), d.clone()
    s2, d2 = net._run(x)                                # the same batch again
    assert torch.equal(s, s2) and torch.equal(d, d2) and d.shape == (5, 64, 96, 3)
    for i in range(5):                                  # alone: no image reads another's halo
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
    assert only["goodpoint_head"][0] == 1 and only["alike_block1"][0] == 1, only
    assert not [k for k in only if k.startswith(("alike_head", "alike_block2", "conv"))], only       # nothing of ALIKE's beyond block 1 runs
    # the C entry with a null map pointer, beside a sentinel-filled buffer of the map's size that it must not reach through any other argument
    sentinel = torch.full((5, 64, 96, 3), 7.0, device=DEV)
    score = torch.empty((5, 1, 64, 96), device=DEV)
    ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(x), 5, 64, 96, ptr(score), ptr(None)))
    ctx.sync()
    assert torch.equal(score, s) and bool((sentinel == 7.0).all())


# ------------------------------------------------------------------------------------------------ 3. detection on the net's own map
@pytest.mark.parametrize("nms_dist,count", [(2, None), (6, 142)])
def test_goodpoint_feeds_detection_and_sampling(net, nms_dist, count):
    import oracle
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import sample_descriptors
    score, desc = net(_img(0, 96, 160))
    ep = dict(EP, nms_dist=nms_dist)
    kps = detection(score, ep)                          # a sigmoid: the default (non-negative) contract
    want, _ = oracle.detection(score[0, 0].cpu().numpy(), ep)
    np.testing.assert_array_equal(kps.cpu().numpy().view(np.uint32), want.view(np.uint32))
    print("goodpoint 96x160 nms_dist %d: %d keypoints" % (nms_dist, kps.shape[0]))
    if count is None:
        assert kps.shape[0] > 100                       # the reference's own map gives 934
    else:
        assert kps.shape[0] == count                    # as the reference's own map
    np.testing.assert_array_equal(sample_descriptors(kps, desc).cpu().numpy(), oracle.sample(desc[0].cpu().numpy(), want))


# ------------------------------------------------------------------------------------------------ 4. pipeline
def test_goodpoint_pipeline_equals_single_pair_path():
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import match_descriptors, sample_descriptors
    B, H, W = 4, 96, 128
    v = [synthetic.image_pair(20 + i, H, W) for i in range(B)]
    i0, i1 = np.stack([a for a, _ in v]), np.stack([b for _, b in v])
    pipe = PairPipeline(_net(), EP, BF, B, H, W, device=DEV)
    pipe.run(torch.from_numpy(np.concatenate([i0, i1])).to(DEV))
    single = _net()
    most = 0
    for b in range(B):
        got = pipe.pair(b)
        s0, d0 = single(torch.from_numpy(i0[b])[None].to(DEV))
        k0 = detection(s0, EP)
        f0 = sample_descriptors(k0, d0)
        s1, d1 = single(torch.from_numpy(i1[b])[None].to(DEV))
        k1 = detection(s1, EP)
        f1 = sample_descriptors(k1, d1)
        np.testing.assert_array_equal(got["kps0"], k0.cpu().numpy())
        np.testing.assert_array_equal(got["kps1"], k1.cpu().numpy())
        pairs, dist = match_descriptors(f0, f1, max_distance=5, cross_check=True, return_distance=True)
        np.testing.assert_array_equal(got["pairs"], pairs.cpu().numpy())
        np.testing.assert_array_equal(got["dist"], dist.cpu().numpy())
        most = max(most, got["kps0"].shape[0])
    assert most > 20


# ------------------------------------------------------------------------------------------------ 5. runner
def _params(path, task):
    return {"model_type": "GoodPoint", "task_type": task, "GoodPoint_params": dict(PARAM, weight=path),
            "extractor_params": dict(EP, nms_dist=4, top_k=300), "matcher_params": {"type": "brute_force", "brute_force_params": BF},
            "repeatability_params": {"th": 3}}


def test_runner_repeatability_rows_batched_equal_single(tmp_path):
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.models.GoodPoint import GoodPoint
    path = str(tmp_path / "goodpoint.pth")
    torch.save(checkpoint(), path)
    h, w = 96, 160
    base = np.array([[1, 0, -3], [0, 1, -2], [0, 0, 1]], np.float32)
    ds = []
    for i in range(5):
        v0, v1 = synthetic.image_pair(100 + i, h, w)
        hm = base + (0.001 * (i % 3)) * np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 0]], np.float32)
        ds.append({"image0": v0, "image1": v1, "dataset": "HPatches",
                   "warp01_params": dict(mode="homo", homography_matrix=hm, width=np.int64(w), height=np.int64(h), resize=np.int64(w)),
                   "warp10_params": dict(mode="homo", homography_matrix=np.linalg.inv(hm).astype(np.float32), width=w, height=h)})
    prm = _params(path, "repeatability")
    single = runner.PairRunner(prm, device=DEV, batch=1)
    assert isinstance(single.model, GoodPoint) and single.model.tracked_maps
    _, rows1 = single.run(ds)
    assert single.batched_pairs == 0
    batched = runner.PairRunner(prm, device=DEV, batch=4)
    agg, rowsb = batched.run(ds)
    assert batched.batched_pairs == 5
    assert np.array_equal(rows1.view(np.uint64), rowsb.view(np.uint64)), (rows1, rowsb)
    assert rowsb[:, 0].min() > 20 and np.isfinite(agg["repeatability"])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_a_shape_that_is_no_multiple_of_32_is_refused_and_the_net_stays_usable(net):
    x = _img(0, 64, 96)
    s, d = net._run(x)
    s, d = s.clone(), d.clone()
    bad = torch.from_numpy(synthetic.image_pair(0, 40, 64)[0])[None].to(DEV)
    score = torch.full((1, 1, 40, 64), 7.0, device=DEV)
    desc = torch.full((1, 40, 64, 3), 7.0, device=DEV)
    ctx = net._ctx
    rc = ctx.lib.kpb_net_forward(net._handle, ptr(bad), 1, 40, 64, ptr(score), ptr(desc))
    assert rc == KPB_E_INVALID
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    assert "GoodPoint" in msg and "40x64" in msg, msg
    ctx.sync()
    assert bool((score == 7.0).all()) and bool((desc == 7.0).all())        # nothing written
    with pytest.raises(KpbError):
        net._run(bad)
    s2, d2 = net._run(x)
    assert torch.equal(s, s2) and torch.equal(d, d2)


def _create(arch, tensors):
    ctx = Context.get(torch.device(DEV))
    blob = weights.pack(tensors, arch)
    h = c_void_p()
    rc = ctx.lib.kpb_net_create(ctx.handle, arch, blob, len(blob), ctypes.byref(h))
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    if h.value:
        ctx.lib.kpb_net_destroy(h)
    return rc, msg, bool(h.value)


def test_create_refuses_missing_misshaped_and_foreign_blobs(net):
    t = weights.fold_goodpoint(checkpoint())
    rc, msg, made = _create(weights.ARCH_GOODPOINT, {k: v for k, v in t.items() if k != "gp.score.w"})
    assert rc == KPB_E_WEIGHTS and not made and "gp.score.w" in msg and "GoodPoint" in msg, msg
    rc, msg, made = _create(weights.ARCH_GOODPOINT, dict(t, **{"gp.desc.w": t["gp.desc.w"][:2]}))
    assert rc == KPB_E_WEIGHTS and not made and "gp.desc.w" in msg and "GoodPoint" in msg, msg
    alike = weights.load_alike_t()
    rc, msg, made = _create(weights.ARCH_GOODPOINT, alike)              # ALIKE-t's tensors: block 1 is there, the heads are not
    assert rc == KPB_E_WEIGHTS and not made and "gp.desc.w" in msg and "GoodPoint" in msg, msg
    rc, msg, made = _create(weights.ARCH_ALIKE, t)                      # and the reverse
    assert rc == KPB_E_WEIGHTS and not made and "b2c1.w" in msg, msg
    ctx = Context.get(torch.device(DEV))
    for blob_arch, arch, tensors in ((weights.ARCH_ALIKE, weights.ARCH_GOODPOINT, alike), (weights.ARCH_GOODPOINT, weights.ARCH_ALIKE, t)):
        blob, h = weights.pack(tensors, blob_arch), c_void_p()          # an intact blob under the other net's arch id
        assert ctx.lib.kpb_net_create(ctx.handle, arch, blob, len(blob), ctypes.byref(h)) == KPB_E_WEIGHTS and not h.value
    rc, msg, made = _create(weights.ARCH_GOODPOINT, t)                  # the intact one is created on the same context
    assert rc == 0 and made, msg


# ------------------------------------------------------------------------------------------------ 7. strict fp32
@pytest.mark.timeout(300)
def test_goodpoint_strict_fp32_kernels_pass_the_goldens():
    """KPB_FP32_MATRIX is read once per process: tests 1 and 2 again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_goodpoint.py::test_goodpoint_against_reference_golden",
           "tests/test_gpu_goodpoint.py::test_goodpoint_batch_equals_solo_and_score_only_writes_no_map"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=250)
    tail = "\n".join(p.stdout.splitlines()[-25:])
    print(tail)
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % tail
    assert "6 passed" in tail and "skipped" not in tail.split("passed")[-1], tail
