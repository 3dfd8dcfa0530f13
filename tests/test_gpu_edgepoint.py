"""GPU parity of N7 (EdgePoint: ALIKE-t's trunk with the edgepoint_score / edgepoint_desc heads of csrc/alike.hip, through the C ABI) against the
reference class's own fp32 CPU outputs with the checkpoint its tree ships (tests/golden/edgepoint*.npz), at five shapes: 32 x 32 (one pixel at
H/32: all sixteen phases of the transposed convolution read the same a4 pixel, every trunk tile partial), 32 x 64 (not square: a swapped H and W in
the strided gathers), 64 x 96 and 96 x 160 (across the tile edges of blocks 1 .. 4) and 480 x 640.

Tolerances.  Score (a raw logit, -33 .. 8): the yardstick is the reference's own fp32-against-fp64 difference with this checkpoint, 2.7e-5 at
480 x 640; a device error above ten times that (2.7e-4) would be a bug.  Measured on an MI355X against the five goldens, largest |score error|:
split-f16 path 4.72e-5, strict-fp32 path 2.81e-5 (both at 480 x 640; 2.3e-5 / 1.1e-5 at 32 x 32); ATOL_SCORE is twice the larger, 9.4e-5.
Descriptors (not unit vectors, max |d| about 1.1): the project's 1e-4 absolute; measured 1.07e-6 / 1.19e-6."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights
from keypoint_bench_amd._lib import Context, KpbError, c_void_p, ptr
from edgepoint_fixtures import PARAM, SHAPES, checkpoint, load_parts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK = 2.7e-5
MEASURED_H16, MEASURED_FP32 = 4.72e-5, 2.81e-5        # largest |score error| over the five goldens (both at 480 x 640)
MEASURED_DESC = (1.07e-6, 1.19e-6)                    # largest |descriptor error|, split-f16 / strict fp32 (480 x 640)
ATOL_SCORE, ATOL_DESC = 2 * max(MEASURED_H16, MEASURED_FP32), 1e-4
assert ATOL_SCORE <= 10 * YARDSTICK
EP = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
BF = dict(metric="euclidean", max_distance=5, cross_check=True)
KPB_E_INVALID, KPB_E_NEGATIVE, KPB_E_WEIGHTS = -1, -4, -6


def _net():
    from keypoint_bench_amd.models.EdgePoint import EdgePoint
    net = EdgePoint(PARAM)
    net.load_state_dict(checkpoint())
    return net.eval()


@pytest.fixture(scope="module")
def net():
    return _net()


@pytest.fixture(scope="module")
def batch17():
    """17 different images of 64 x 96 (the fused-tail trunk starts at 16), computed once."""
    return torch.from_numpy(np.stack([synthetic.image_pair(500 + i, 64, 96)[i & 1] for i in range(17)])).to(DEV)


def _img(seed, H, W, view=0):
    return torch.from_numpy(synthetic.image_pair(seed, H, W)[view])[None].to(DEV)


# ------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("H,W", SHAPES)
def test_edgepoint_against_reference_golden(net, H, W):
    g = load_parts("edgepoint")
    v0, _ = synthetic.image_pair(0, H, W)
    assert synthetic.checksum(v0) == str(g["%dx%d.img.sum" % (H, W)])
    score, desc = net(torch.from_numpy(v0)[None].to(DEV))
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 64, H // 8, W // 8)
    d = desc[0].permute(1, 2, 0).cpu().numpy()
    es = float(np.abs(score[0, 0].cpu().numpy() - g["%dx%d.score" % (H, W)]).max())
    ed = float(np.abs(d - g["%dx%d.desc" % (H, W)]).max())
    print("edgepoint %dx%d %s: max |score error| %.3g, max |desc error| %.3g, max |desc| %.3g"
          % (H, W, "fp32" if os.environ.get("KPB_FP32_MATRIX") == "1" else "split-f16", es, ed, float(np.abs(d).max())))
    assert es <= ATOL_SCORE and ed <= ATOL_DESC
    assert 0.5 < float(np.abs(d).max()) < 2.0
    assert float(np.linalg.norm(d, axis=-1).min()) > 1.2        # not normalised: the reference's rows have norms 1.30 .. 1.89


# ------------------------------------------------------------------------------------------------ 2. launch regimes
@pytest.mark.parametrize("fused", [1, 0])
def test_edgepoint_launch_regimes_give_the_same_bits(net, batch17, fused):
    ctx = Context.get(torch.device(DEV))
    ctx.set_option(Context.OPT_ALIKE_COARSE_FUSED, fused)
    try:
        s, d = net._run(batch17)
        s, d = s.clone(), d.clone()
        s2, d2 = net._run(batch17)                      # the same batch again
        assert torch.equal(s, s2) and torch.equal(d, d2)
        for i in (0, 8, 16):                            # alone: the latency path (fewer than 16 images)
            si, di = net._run(batch17[i:i + 1].contiguous())
            assert torch.equal(si[0], s[i]), "score of image %d: max |d| = %g" % (i, (si[0] - s[i]).abs().max().item())
            assert torch.equal(di[0], d[i]), "descriptors of image %d: max |d| = %g" % (i, (di[0] - d[i]).abs().max().item())
    finally:
        ctx.set_option(Context.OPT_ALIKE_COARSE_FUSED, 1)
    assert torch.isfinite(s).all() and torch.isfinite(d).all() and d.shape == (17, 8, 12, 64)


# ------------------------------------------------------------------------------------------------ 3. score only
def test_edgepoint_score_only_forward_skips_the_descriptor_kernel(net):
    x = _img(5, 96, 160)
    s, d = net._run(x)
    s = s.clone()
    ctx = Context.get(torch.device(DEV))
    ctx.prof_enable(True)
    try:
        ctx.prof_report()
        s2, d2 = net._run(x, want_desc=False)
        ctx.sync()
        only = ctx.prof_report()
        net._run(x)
        ctx.sync()
        both = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
    assert d2 is None and torch.equal(s, s2)
    assert only["edgepoint_score"][0] == 1 and "edgepoint_desc" not in only, only
    assert both["edgepoint_score"][0] == 1 and both["edgepoint_desc"][0] == 1, both
    assert not [k for k in both if "head" in k], both                   # ALIKE's heads do not run


# ------------------------------------------------------------------------------------------------ 4. detection on the net's own map
@pytest.mark.parametrize("nms_dist", [2, 6])
def test_edgepoint_feeds_signed_detection_and_sampling(net, nms_dist):
    import oracle
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import sample_descriptors
    score, desc = net(_img(0, 96, 160))
    ep = dict(EP, nms_dist=nms_dist)
    with pytest.raises(KpbError) as e:
        detection(score, ep)                            # the default contract is non-negative maps
    assert e.value.code == KPB_E_NEGATIVE
    kps = detection(score, ep, signed=True)
    want, _ = oracle.detection(score[0, 0].cpu().numpy(), ep)
    np.testing.assert_array_equal(kps.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if nms_dist == 2:
        assert kps.shape[0] > 100                       # the reference's own map gives 416
    np.testing.assert_array_equal(sample_descriptors(kps, desc).cpu().numpy(), oracle.sample(desc[0].cpu().numpy(), want))


def test_edgepoint_matches_a_synthetic_pair(net):
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import brute_force_matcher
    s0, d0 = net(_img(8, 128, 160, 0))
    s0, d0 = s0.clone(), d0.clone()
    s1, d1 = net(_img(8, 128, 160, 1))
    ep = dict(EP, nms_dist=4, top_k=300)
    k0, k1 = detection(s0, ep, signed=True), detection(s1, ep, signed=True)
    m0, m1 = brute_force_matcher(k0, k1, d0, d1, BF)
    assert m0.shape == m1.shape and m0.shape[1] == 3 and m0.shape[0] > 0


# ------------------------------------------------------------------------------------------------ 5. pipeline
@pytest.mark.parametrize("B,H,W", [(4, 128, 160), (16, 64, 96)], ids=["4x128x160", "16x64x96-fused-trunk"])
def test_edgepoint_pipeline_equals_single_pair_path(B, H, W):
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import match_descriptors, sample_descriptors
    v = [synthetic.image_pair(20 + i, H, W) for i in range(B)]
    i0, i1 = np.stack([a for a, _ in v]), np.stack([b for _, b in v])
    pipe = PairPipeline(_net(), EP, BF, B, H, W, device=DEV)
    pipe.run(torch.from_numpy(np.concatenate([i0, i1])).to(DEV))
    assert Context.get(torch.device(DEV))._detect_signed == 0
    single = _net()
    most = 0
    for b in range(B):
        got = pipe.pair(b)
        s0, d0 = single(torch.from_numpy(i0[b])[None].to(DEV))
        k0 = detection(s0, EP, signed=True)
        f0 = sample_descriptors(k0, d0)
        s1, d1 = single(torch.from_numpy(i1[b])[None].to(DEV))
        k1 = detection(s1, EP, signed=True)
        f1 = sample_descriptors(k1, d1)
        np.testing.assert_array_equal(got["kps0"], k0.cpu().numpy())
        np.testing.assert_array_equal(got["kps1"], k1.cpu().numpy())
        pairs, dist = match_descriptors(f0, f1, max_distance=5, cross_check=True, return_distance=True)
        np.testing.assert_array_equal(got["pairs"], pairs.cpu().numpy())
        np.testing.assert_array_equal(got["dist"], dist.cpu().numpy())
        most = max(most, got["kps0"].shape[0])
    assert most > 20


# ------------------------------------------------------------------------------------------------ 6. runner
def _params(path, task):
    return {"model_type": "EdgePoint", "task_type": task, "EdgePoint_params": dict(PARAM, weight=path),
            "extractor_params": dict(EP, nms_dist=4, top_k=300), "matcher_params": {"type": "brute_force", "brute_force_params": BF},
            "repeatability_params": {"th": 3}}


def test_build_model_loads_a_checkpoint_file(tmp_path, net):
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.models.EdgePoint import EdgePoint
    path = str(tmp_path / "EdgePoint.pt")
    torch.save(checkpoint(), path)
    model = runner.build_model(_params(path, "repeatability"))
    assert isinstance(model, EdgePoint) and model.signed_scores
    x = _img(0, 32, 64)
    s, d = model(x)
    s, d = s.clone(), d.clone()
    assert model.dim == 64 and model.desc_div == 8
    s2, d2 = net(x)
    assert torch.equal(s, s2) and torch.equal(d, d2)


def test_runner_repeatability_rows_batched_equal_single(tmp_path):
    from keypoint_bench_amd import runner
    path = str(tmp_path / "EdgePoint.pt")
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
    _, rows1 = single.run(ds)
    assert single.batched_pairs == 0
    batched = runner.PairRunner(prm, device=DEV, batch=4)
    agg, rowsb = batched.run(ds)
    assert batched.batched_pairs == 5
    assert np.array_equal(rows1.view(np.uint64), rowsb.view(np.uint64)), (rows1, rowsb)
    assert rowsb[:, 0].min() > 20 and np.isfinite(agg["repeatability"])
    assert Context.get(torch.device(DEV))._detect_signed == 0


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_a_shape_that_is_no_multiple_of_32_is_refused_and_the_net_stays_usable(net):
    x = _img(0, 64, 96)
    s, d = net._run(x)
    s, d = s.clone(), d.clone()
    bad = torch.from_numpy(synthetic.image_pair(0, 40, 64)[0])[None].to(DEV)
    score = torch.full((1, 1, 40, 64), 7.0, device=DEV)
    desc = torch.full((1, 5, 8, 64), 7.0, device=DEV)
    ctx = net._ctx
    rc = ctx.lib.kpb_net_forward(net._handle, ptr(bad), 1, 40, 64, ptr(score), ptr(desc))
    assert rc == KPB_E_INVALID
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    assert "EdgePoint" in msg and "40x64" in msg, msg
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
    t = weights.fold_edgepoint(checkpoint())
    rc, msg, made = _create(weights.ARCH_EDGEPOINT, {k: v for k, v in t.items() if k != "ct4.w"})
    assert rc == KPB_E_WEIGHTS and not made and "ct4.w" in msg and "EdgePoint" in msg and "8,16,32,64" in msg, msg
    rc, msg, made = _create(weights.ARCH_EDGEPOINT, dict(t, **{"ct4.w": t["ct4.w"][:, :, :3, :3]}))
    assert rc == KPB_E_WEIGHTS and not made and "ct4.w" in msg, msg
    alike = weights.load_alike_t()
    rc, msg, made = _create(weights.ARCH_EDGEPOINT, alike)              # ALIKE-t's tensors: a 65-row head, no score layer
    assert rc == KPB_E_WEIGHTS and not made and "head.w" in msg, msg
    rc, msg, made = _create(weights.ARCH_ALIKE, t)                      # and the reverse
    assert rc == KPB_E_WEIGHTS and not made and "head.w" in msg, msg
    ctx = Context.get(torch.device(DEV))
    blob, h = weights.pack(alike, weights.ARCH_ALIKE), c_void_p()       # an intact blob under the other net's arch id
    assert ctx.lib.kpb_net_create(ctx.handle, weights.ARCH_EDGEPOINT, blob, len(blob), ctypes.byref(h)) == KPB_E_WEIGHTS and not h.value
    rc, msg, made = _create(weights.ARCH_EDGEPOINT, t)                  # the intact one is created on the same context
    assert rc == 0 and made, msg


# ------------------------------------------------------------------------------------------------ 8. strict fp32
@pytest.mark.timeout(600)
def test_edgepoint_strict_fp32_kernels_pass_the_goldens():
    """KPB_FP32_MATRIX is read once per process: tests 1 and 2 again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_edgepoint.py::test_edgepoint_against_reference_golden",
           "tests/test_gpu_edgepoint.py::test_edgepoint_launch_regimes_give_the_same_bits"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=500)
    tail = "\n".join(p.stdout.splitlines()[-25:])
    print(tail)
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % tail
    assert "7 passed" in tail and "skipped" not in tail.split("passed")[-1], tail
