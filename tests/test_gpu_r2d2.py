"""GPU parity of N6 (R2D2, csrc/r2d2.hip through the C ABI) against the reference class's own fp32 CPU outputs with the checkpoint its tree
ships (tests/golden/r2d2*.npz), at four shapes: 64 x 96, 61 x 97 (odd), 24 x 40 (smaller than the reach of the largest dilation) and 480 x 640.

Tolerances.  Descriptors are unit vectors: the project's 1e-4 absolute.  Score: the yardstick is the reference's own fp32-against-fp64
difference with this checkpoint, 1.9e-6; a device error above ten times that (2e-5) would be a bug.  Measured on an MI355X against the four
goldens, largest |score error|: split-f16 path 3.46e-6, strict-fp32 path 3.16e-6 (both at 480 x 640; descriptors 8.3e-7 / 1.0e-6); ATOL_SCORE is twice the larger."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic
from r2d2_fixtures import SHAPES, checkpoint, load_parts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_H16, MEASURED_FP32 = 3.46e-6, 3.16e-6
ATOL_SCORE, ATOL_DESC = 2 * max(MEASURED_H16, MEASURED_FP32), 1e-4
EP = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
BF = dict(metric="euclidean", max_distance=5, cross_check=True)


def _net():
    from keypoint_bench_amd.models.r2d2 import from_checkpoint
    return from_checkpoint(checkpoint())


@pytest.fixture(scope="module")
def net():
    return _net()


@pytest.mark.parametrize("H,W", SHAPES)
def test_r2d2_against_reference_golden(net, H, W):
    g = load_parts("r2d2")
    v0, _ = synthetic.image_pair(0, H, W)
    score, desc = net(torch.from_numpy(v0)[None].to(DEV))
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 128, H, W)
    d = desc[0].permute(1, 2, 0).cpu().numpy()
    if H >= 480:
        d = d[::8, ::8]
    es = float(np.abs(score[0, 0].cpu().numpy() - g["%dx%d.score" % (H, W)]).max())
    ed = float(np.abs(d - g["%dx%d.desc" % (H, W)]).max())
    print("r2d2 %dx%d %s: max |score error| %.3g, max |desc error| %.3g" % (H, W, "fp32" if os.environ.get("KPB_FP32_MATRIX") == "1" else "split-f16", es, ed))
    assert es <= ATOL_SCORE and ed <= ATOL_DESC
    n = torch.linalg.norm(desc[0], dim=0)
    np.testing.assert_allclose(n.cpu().numpy(), 1.0, rtol=0, atol=1e-5)


def test_r2d2_batching_does_not_change_bits(net):
    v0, v1 = synthetic.image_pair(3, 61, 97)
    s, d = net(torch.from_numpy(np.stack([v0, v1])).to(DEV))
    s, d = s.clone(), d.clone()
    for i, v in enumerate((v0, v1)):
        si, di = net(torch.from_numpy(v)[None].to(DEV))
        assert torch.equal(si[0], s[i]) and torch.equal(di[0], d[i])


def test_r2d2_three_runs_are_bit_identical(net):
    v0, v1 = synthetic.image_pair(4, 128, 160)
    x = torch.from_numpy(np.stack([v0, v1])).to(DEV)
    s0, d0 = net(x)
    s0, d0 = s0.clone(), d0.clone()
    for _ in range(2):
        s, d = net(x)
        assert torch.equal(s, s0) and torch.equal(d, d0)


def test_r2d2_feeds_detection_and_matcher(net):
    import oracle
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import brute_force_matcher, sample_descriptors
    v0, v1 = synthetic.image_pair(8, 128, 160)
    s0, d0 = net(torch.from_numpy(v0)[None].to(DEV))
    s1, d1 = net(torch.from_numpy(v1)[None].to(DEV))
    ep = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
    k0, k1 = detection(s0, ep), detection(s1, ep)
    ok0, _ = oracle.detection(s0[0, 0].cpu().numpy(), ep)
    np.testing.assert_array_equal(k0.cpu().numpy().view(np.uint32), ok0.view(np.uint32))
    np.testing.assert_array_equal(sample_descriptors(k0, d0).cpu().numpy(), oracle.sample(d0[0].cpu().numpy(), ok0))
    m0, m1 = brute_force_matcher(k0, k1, d0, d1, {"metric": "euclidean", "max_distance": 5, "cross_check": True})
    assert m0.shape == m1.shape and m0.shape[1] == 3 and m0.shape[0] > 0


def test_r2d2_pipeline_equals_single_pair_path():
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import match_descriptors, sample_descriptors
    B, H, W = 4, 128, 160
    v = [synthetic.image_pair(20 + i, H, W) for i in range(B)]
    i0, i1 = np.stack([a for a, _ in v]), np.stack([b for _, b in v])
    pipe = PairPipeline(_net(), EP, BF, B, H, W, device=DEV)
    pipe.run(torch.from_numpy(np.concatenate([i0, i1])).to(DEV))
    single = _net()
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
        assert got["kps0"].shape[0] > 20


def test_build_model_loads_a_checkpoint_file(tmp_path, net):
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.models.r2d2 import Quad_L2Net_ConfCFS
    path = str(tmp_path / "r2d2_WASF_N16.pt")
    torch.save(checkpoint(), path)
    model = runner.build_model({"model_type": "r2d2", "r2d2_params": {"weight": path}})
    assert isinstance(model, Quad_L2Net_ConfCFS)
    v0, _ = synthetic.image_pair(0, 24, 40)
    x = torch.from_numpy(v0)[None].to(DEV)
    s, d = model(x)
    assert model.dim == 128 and model.desc_div == 1
    s2, d2 = net(x)
    assert torch.equal(s, s2) and torch.equal(d, d2)


@pytest.mark.timeout(900)
def test_r2d2_strict_fp32_kernels_pass_the_goldens():
    """KPB_FP32_MATRIX is read once per process: the goldens again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_r2d2.py::test_r2d2_against_reference_golden", "tests/test_gpu_r2d2.py::test_r2d2_batching_does_not_change_bits",
           "tests/test_gpu_r2d2.py::test_r2d2_three_runs_are_bit_identical"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=800)
    tail = "\n".join(p.stdout.splitlines()[-25:])
    print(tail)
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % tail
    assert "6 passed" in tail and "skipped" not in tail.split("passed")[-1], tail
