"""DISK's keypoint-only mode on the GPU: kpb_net_forward(desc_out_dev = NULL) and kpb_net_desc_at through the C ABI, then through the Python model and PairPipeline.

1. score      forward(desc NULL) gives the BITS of forward(desc): up_3's score channel is accumulated on the VALU from the staged tile in both forms (strict fp32: the
              fifth tile's accumulator chain), so the keypoints cannot move.
2. desc_at    against the torch-fp32 oracle (oracle.disk_ref.disk_forward, then oracle.sample on ITS descriptor map): max |difference| <= 1e-4, the project's bound
              for DISK descriptors against this oracle (ATOL_DESC of test_gpu_disk.py, TOL["disk"] of test_gpu_net_shapes.py).  The points are the places where the
              tap arithmetic can go wrong: the corners, integer pixels of both parities (the two phases of the x2 upsampling), x = W - 1 / y = H - 1 (a tap outside the
              map: a select, not a product), points within 2 px of every border (the zero padding of the ACTIVATED input), half pixels, near-integers, random ones.
              max_n = 45 is no multiple of the 8 keypoints of a workgroup; n = [45, 29, 0]; the rows at or past n[b] keep their sentinel.
              Printed, not asserted: the deviation from kpb_sample on the same build's dense map.
3. refusals   desc_at before any forward.
4. one pair   through detection and brute_force_matcher, dense against keypoint-only: equal keypoints, the matches as sets within 1 % of each other; the stale handle.
5. PairPipeline  B = 2: equal n and kps, no map allocated, k within 1; LightGlue refused.
Shapes (tests 1-3): 16 x 32 and 32 x 16 are the smallest DISK runs (every level below one tile, the fused upsampling stages a clamped source), 16 x 272 a strip,
48 x 80 (B = 3) and 64 x 96 (B = 2) have more than one tile and more than one image.  Tests 1-3 run again in a child process under KPB_FP32_MATRIX=1.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights
from keypoint_bench_amd._lib import Context, KpbError, c_void_p, ptr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32 = os.environ.get("KPB_FP32_MATRIX") == "1"
ARITH = "fp32" if FP32 else "split-f16"
ATOL_DESC = 1e-4
SENTINEL = 7.5
MAX_N = 45
SHAPES = [(16, 32, 1), (32, 16, 1), (16, 272, 1), (48, 80, 3), (64, 96, 2)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
COUNTS = [45, 29, 0]


class Native:
    """One DISK kpb_net (disk_random(5)) behind the C ABI."""

    def __init__(self):
        from keypoint_bench_amd.models.disk import disk_random
        blob = disk_random(5)._blob
        self.ctx = Context.get(DEV)
        self.h = c_void_p()
        self.ctx.check(self.ctx.lib.kpb_net_create(self.ctx.handle, weights.ARCH_DISK, blob, len(blob), ctypes.byref(self.h)))

    def forward(self, x, dense):
        B, _, H, W = x.shape
        score = torch.full((B, H, W), SENTINEL, dtype=torch.float32, device=DEV)
        desc = torch.empty((B, H, W, 128), dtype=torch.float32, device=DEV) if dense else None
        self.ctx.check(self.ctx.lib.kpb_net_forward(self.h, ptr(x), B, H, W, ptr(score), ptr(desc)))
        return score, desc

    def desc_at(self, pts, n=None):
        B, max_n, cols = pts.shape
        out = torch.full((B, max_n, 128), SENTINEL, dtype=torch.float32, device=DEV)
        self.ctx.check(self.ctx.lib.kpb_net_desc_at(self.h, ptr(pts), cols, max_n, ptr(n), ptr(out)))
        return out

    def close(self):
        if self.h is not None:
            self.ctx.lib.kpb_net_destroy(self.h)
            self.h = None


@pytest.fixture
def net():
    n = Native()
    yield n
    n.close()


def _images(H, W, B):
    return np.stack([synthetic.image_pair(20 + i, H, W)[i & 1] for i in range(B)])


def _points(H, W, seed):
    """[MAX_N, 2] normalised (x, y): pixel coordinate / (size - 1), as the detector writes them."""
    w1, h1 = W - 1.0, H - 1.0
    px = [(0, 0), (w1, 0), (0, h1), (w1, h1),                                               # the corners
          (4, 6), (5, 7), (4, 7), (5, 6),                                                   # integer pixels, both parities in x and in y
          (w1, 3.3), (2.7, h1),                                                             # the second tap is outside the map
          (0.6, 5.2), (1.4, 8.5), (w1 - 0.6, 4.4), (w1 - 1.3, 9.1), (6.3, 0.7), (7.8, 1.5), (5.5, h1 - 0.3), (9.2, h1 - 1.4),      # within 2 px of each border
          (3.5, 4.5), (8.5, 2.5), (6.5, 7.0),                                               # half pixels
          (7.999, 8.001), (8.001, 3.999), (11.999, 12.001)]                                 # near-integers
    rng = np.random.RandomState(seed)
    while len(px) < MAX_N:
        px.append((rng.uniform(0, w1), rng.uniform(0, h1)))
    p = np.asarray(px, np.float64)
    assert p.shape == (MAX_N, 2) and p[:, 0].max() <= w1 and p[:, 1].max() <= h1 and p.min() >= 0
    return (p / np.array([w1, h1])).astype(np.float32)


_ORACLE = {}


def _oracle(H, W, B):
    """(images, points [B, MAX_N, 2], oracle.sample of the oracle's descriptor map at them [B, MAX_N, 128]); computed once per shape, never modified."""
    if (H, W, B) not in _ORACLE:
        import oracle
        from oracle import disk_ref
        imgs = _images(H, W, B)
        pts = np.stack([_points(H, W, 3 * b + H) for b in range(B)])
        t = {k: torch.from_numpy(v) for k, v in weights.tensors_disk(weights.random_disk_state_dict(5)).items()}
        with torch.no_grad():
            _, do = disk_ref.disk_forward(torch.from_numpy(imgs), t)
        want = np.stack([oracle.sample(do[b].numpy(), pts[b]) for b in range(B)])
        for a in (imgs, pts, want):
            a.setflags(write=False)
        _ORACLE[(H, W, B)] = (imgs, pts, want)
    return _ORACLE[(H, W, B)]


# ------------------------------------------------------------------------------------------------ 1. score
@pytest.mark.parametrize("H,W,B", SHAPES, ids=IDS)
def test_keypoint_only_score_has_the_dense_forward_bits(net, H, W, B):
    x = torch.from_numpy(_images(H, W, B)).to(DEV)
    s_kp, none = net.forward(x, dense=False)
    s_dense, desc = net.forward(x, dense=True)
    assert none is None and desc is not None
    assert float(s_dense.min()) >= 0.0 and float(s_dense.max()) <= 1.0 and float(s_dense.std()) > 0.0       # a sigmoid, and the sentinel is gone
    d = (s_kp - s_dense).abs().max().item()
    print("disk keypoint-only score %dx%dx%d %s: max |score - dense score| = %g" % (H, W, B, ARITH, d))
    assert torch.equal(s_kp, s_dense), "max |d| = %g" % d
    s_again, _ = net.forward(x, dense=False)        # after a dense forward on the same net object
    assert torch.equal(s_again, s_dense)


# ------------------------------------------------------------------------------------------------ 2. desc_at
@pytest.mark.parametrize("H,W,B", SHAPES, ids=IDS)
def test_desc_at_against_the_oracle(net, H, W, B):
    from keypoint_bench_amd.utils.matcher import sample_descriptors
    imgs, pts_np, want_np = _oracle(H, W, B)
    x, pts, want = torch.tensor(imgs, device=DEV), torch.tensor(pts_np, device=DEV), torch.tensor(want_np, device=DEV)
    counts = COUNTS[:B]
    n = torch.tensor(counts, dtype=torch.int32, device=DEV)
    assert float(want.abs().max()) > 0.05          # a zero output cannot pass
    net.forward(x, dense=False)
    got = net.desc_at(pts, n)
    for b, c in enumerate(counts):
        assert torch.all(got[b, c:] == SENTINEL), "rows at or past n[%d] = %d were written" % (b, c)
        if c:
            err = (got[b, :c] - want[b, :c]).abs().max().item()
            print("disk desc_at %dx%d image %d %s: max |desc_at - oracle| = %.3g over %d points" % (H, W, b, ARITH, err, c))
            assert err <= ATOL_DESC, "image %d: %g" % (b, err)
    assert torch.equal(net.desc_at(pts, n), got)        # the same run against run
    # three-column (x, y, score) rows without counts: the same bits as the two-column rows with counts
    pts3 = torch.cat([pts, torch.full((B, MAX_N, 1), 0.25, device=DEV)], 2).contiguous()
    full = net.desc_at(pts3, None)
    assert not torch.any(full == SENTINEL)
    for b, c in enumerate(counts):
        assert torch.equal(full[b, :c], got[b, :c])
    if B > 1:       # the last image has n = 0 above: its rows against the oracle here
        assert (full - want).abs().max().item() <= ATOL_DESC
    # ONE dense forward: the net keeps what up_3 read after either kind of forward, so desc_at reads the same activations
    _, dense = net.forward(x, dense=True)
    assert torch.equal(net.desc_at(pts3, None), full)
    sampled = torch.stack([sample_descriptors(pts[b], dense[b:b + 1].permute(0, 3, 1, 2)) for b in range(B)])
    print("disk desc_at %dx%dx%d %s: max |desc_at - kpb_sample(dense map)| = %.3g (not asserted); max |kpb_sample(dense map) - oracle| = %.3g"
          % (H, W, B, ARITH, (full - sampled).abs().max().item(), (sampled - want).abs().max().item()))


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_desc_at_needs_a_forward(net):
    imgs, pts_np, _ = _oracle(16, 32, 1)
    pts = torch.tensor(pts_np, device=DEV)
    with pytest.raises(KpbError, match="kpb_net_desc_at: no forward has run"):
        net.desc_at(pts)
    net.forward(torch.tensor(imgs, device=DEV), dense=False)
    assert not torch.any(net.desc_at(pts) == SENTINEL)
    with pytest.raises(KpbError, match="kpb_net_desc_at: bad argument"):
        net.ctx.check(net.ctx.lib.kpb_net_desc_at(net.h, ptr(pts), 1, MAX_N, ptr(None), ptr(torch.empty((MAX_N, 128), device=DEV))))


@pytest.mark.timeout(300)
def test_strict_fp32_kernels_pass_the_same_tests():
    """KPB_FP32_MATRIX is read once per process: tests 1 to 3 again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    me = "tests/test_gpu_disk_keypoint_only.py::"
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", me + "test_keypoint_only_score_has_the_dense_forward_bits",
           me + "test_desc_at_against_the_oracle", me + "test_desc_at_needs_a_forward"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=250)
    out = "\n".join(l for l in p.stdout.splitlines() if "disk " in l or "passed" in l or "failed" in l or "rror" in l)
    print(out)
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % "\n".join(p.stdout.splitlines()[-40:])
    assert "%d passed" % (2 * len(SHAPES) + 1) in out and "skipped" not in out
    assert out.count(" fp32: ") >= 2 * len(SHAPES) and " split-f16: " not in out         # every case ran under the knob


# ------------------------------------------------------------------------------------------------ 4. one pair through the seams
EP = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
BF = {"metric": "euclidean", "max_distance": 5, "cross_check": True}


def test_one_pair_dense_against_keypoint_only():
    from keypoint_bench_amd.models._base import LazyDescriptors
    from keypoint_bench_amd.models.disk import disk_random
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import brute_force_matcher, sample_descriptors
    v0, v1 = synthetic.image_pair(8, 128, 160)
    x0, x1 = torch.from_numpy(v0)[None].to(DEV), torch.from_numpy(v1)[None].to(DEV)
    res = {}
    for dense in (True, False):
        m = disk_random(2, dense_descriptors=dense).eval()
        s0, d0 = m(x0)
        s1, d1 = m(x1)
        assert isinstance(d0, LazyDescriptors) != dense and tuple(d0.shape) == (1, 128, 128, 160)
        k0, k1 = detection(s0, EP), detection(s1, EP)
        m0, m1 = brute_force_matcher(k0, k1, d0, d1, BF)
        res[dense] = (k0.cpu().numpy(), k1.cpu().numpy(), m0.cpu().numpy(), m1.cpu().numpy())
        if not dense:
            assert sample_descriptors(k0, d0).shape == (k0.shape[0], 128)
            for _ in range(m.KEEP):
                m(x1)
            with pytest.raises(RuntimeError, match="LazyDescriptors used after 2 later forwards"):
                d0.sample(k0)
    (k0, k1, m0, m1), (l0, l1, lm0, lm1) = res[True], res[False]
    assert k0.shape[0] > 50 and m0.shape[0] > 20
    np.testing.assert_array_equal(k0.view(np.uint32), l0.view(np.uint32))
    np.testing.assert_array_equal(k1.view(np.uint32), l1.view(np.uint32))
    # the keypoints are equal and distinct, so a matched pair of rows names its index pair
    pairs = lambda a, b: {(r0.tobytes(), r1.tobytes()) for r0, r1 in zip(a, b)}
    dense_set, kp_set = pairs(m0, m1), pairs(lm0, lm1)
    diff = len(dense_set ^ kp_set)
    print("disk one pair: %d keypoints, %d dense matches, %d keypoint-only matches, symmetric difference %d" % (k0.shape[0], len(dense_set), len(kp_set), diff))
    assert diff <= 0.01 * len(dense_set)


# ------------------------------------------------------------------------------------------------ 5. PairPipeline
def test_pair_pipeline_keypoint_only_against_dense():
    from keypoint_bench_amd.models.disk import disk_random
    from keypoint_bench_amd.models.lightglue import LightGlue
    from keypoint_bench_amd.pipeline import PairPipeline
    B, H, W = 2, 64, 96
    ep = dict(EP, top_k=100)
    v = [synthetic.image_pair(40 + i, H, W) for i in range(B)]
    images = torch.from_numpy(np.concatenate([np.stack([a for a, _ in v]), np.stack([b for _, b in v])])).to(DEV)
    pipes = {}
    for dense in (True, False):
        pipes[dense] = PairPipeline(disk_random(5, dense_descriptors=dense).eval(), ep, BF, B, H, W, device=DEV).run(images)
    d, s = pipes[True], pipes[False]
    assert s.desc is None and d.desc is not None
    n = d.n.cpu().numpy()
    assert n.min() > 10
    np.testing.assert_array_equal(s.n.cpu().numpy(), n)
    for i, c in enumerate(n):
        np.testing.assert_array_equal(s.kps[i, :c].cpu().numpy().view(np.uint32), d.kps[i, :c].cpu().numpy().view(np.uint32))
    kd, ks = d.k.cpu().numpy().astype(np.int64), s.k.cpu().numpy().astype(np.int64)
    print("disk PairPipeline: n", n.tolist(), "k dense", kd.tolist(), "k keypoint-only", ks.tolist())
    assert kd.min() > 0 and np.abs(kd - ks).max() <= 1
    with pytest.raises(ValueError, match="the LightGlue matcher samples the dense descriptor map"):
        PairPipeline(disk_random(5, dense_descriptors=False).eval(), ep, BF, B, H, W, device=DEV, lightglue=LightGlue(features=None, desc_scale=1))
