"""GPU parity of ALIKE-l (csrc/alike_l.hip through the C ABI and through models/ALike.py): the reference's default ALNet(), c1..c4 = 32, 64, 128, 128,
dim = 128, on SEEDED STAND-IN weights (tests/golden/make_golden_alike_l.py: the reference ships no checkpoint for this plan), against the reference class's own
fp32 CPU outputs at five shapes -- 32 x 32 (a4 is one pixel: a constant under the x 32 upsampling), 32 x 64 (not square), 64 x 96, 96 x 160 and 160 x 224
(across the tile edges of every block; more than one 32-pixel head segment per row, more than one workgroup of the head) -- and against the torch-fp32
oracle (oracle/alike_ref.py on the same folded tensors) for the whole descriptor map.

Bars: the project's ALIKE bars (tests/test_gpu_alike.py), score atol 7e-6 and descriptors atol 1e-4, the latter multiplied by max(1, max |desc_ref|) of the
shape because these maps are not unit-scale (max |desc| 2.5 .. 4.5).  Keypoint-only mode against the dense one: 2e-6 on the score, 2e-5 x max(1, max |desc|)
on sampled descriptors -- the project's bars for "linear re-association only".  Every test prints what it measured before it asserts.
Measured on an MI355X, largest error over the five shapes (score / descriptors): split-f16 1.1e-6 / 5.6e-6, strict fp32 1.34e-6 / 5.48e-6 (MEASURED below);
keypoint-only score = dense score bit for bit (the same accumulation), desc_at against sampling the dense map 1.2e-6."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights
from keypoint_bench_amd._lib import Context, c_void_p, ptr
from alike_l_fixtures import FULL_DESC, PARAM, SCORE_ATOL, SHAPES, desc_bar, desc_of, load_parts, state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32 = os.environ.get("KPB_FP32_MATRIX") == "1"
MODE = "fp32" if FP32 else "split-f16"
EP = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
BF = dict(metric="euclidean", max_distance=float("inf"), cross_check=True)
KPB_E_INVALID, KPB_E_WEIGHTS = -1, -6
BOTH_PLANS = ("8,16,32,64, dim = 64", "32,64,128,128, dim = 128")
# largest |error| against the reference fixtures over the five shapes, MI355X: (score, descriptors), both at 160 x 224 where max |desc_ref| is 4.52 -- the
# strict-fp32 kernels stay inside the project's bars, so the bars stand as they are and nothing was derived from the split-f16 path's own error
MEASURED = {"split-f16": (1.1e-6, 5.6e-6), "fp32": (1.34e-6, 5.48e-6)}


def _net(dense=True):
    from keypoint_bench_amd.models.ALike import ALNet
    net = ALNet(dense_descriptors=dense)
    net.load_state_dict(state_dict())
    return net.eval()


@pytest.fixture(scope="module")
def net():
    return _net()


@pytest.fixture(scope="module")
def folded():
    return weights.fold_alike(state_dict())


@pytest.fixture(scope="module")
def oracle_maps(folded):
    """(score [H, W], desc [H, W, 128]) of the torch-fp32 oracle for the fixture image of every shape, computed once."""
    from oracle.alike_ref import alnet_forward
    t = {k: torch.from_numpy(v) for k, v in folded.items()}
    out = {}
    with torch.no_grad():
        for H, W in SHAPES:
            s, d = alnet_forward(torch.from_numpy(synthetic.image_pair(0, H, W)[0])[None], t)
            out[(H, W)] = (s[0, 0].numpy(), d[0].permute(1, 2, 0).contiguous().numpy())
    return out


def _img(seed, H, W, view=0):
    return torch.from_numpy(synthetic.image_pair(seed, H, W)[view])[None].to(DEV)


class Native:
    """One kpb_net behind the C ABI."""

    def __init__(self, blob, arch=weights.ARCH_ALIKE):
        self.ctx = Context.get(torch.device(DEV))
        self.h = c_void_p()
        self.ctx.check(self.ctx.lib.kpb_net_create(self.ctx.handle, arch, blob, len(blob), ctypes.byref(self.h)))
        self.dim, self.div = self.ctx.lib.kpb_net_desc_dim(self.h), self.ctx.lib.kpb_net_desc_div(self.h)

    def forward(self, x, dense=True):
        B, _, H, W = x.shape
        score = torch.empty((B, H, W), dtype=torch.float32, device=DEV)
        desc = torch.empty((B, H, W, self.dim), dtype=torch.float32, device=DEV) if dense else None
        self.ctx.check(self.ctx.lib.kpb_net_forward(self.h, ptr(x), B, H, W, ptr(score), ptr(desc)))
        return score, desc

    def close(self):
        if self.h is not None:
            self.ctx.lib.kpb_net_destroy(self.h)
            self.h = None


@pytest.fixture(scope="module")
def native(folded):
    n = Native(weights.pack(folded, weights.ARCH_ALIKE))
    yield n
    n.close()


# ------------------------------------------------------------------------------------------------ 1. dense forward against the fixtures and the oracle
@pytest.mark.parametrize("H,W", SHAPES)
def test_dense_forward_against_reference_fixture_and_oracle(net, oracle_maps, H, W):
    g = load_parts("alike_l")
    v0, _ = synthetic.image_pair(0, H, W)
    assert synthetic.checksum(v0) == str(g["%dx%d.img.sum" % (H, W)])
    score, desc = net(torch.from_numpy(v0)[None].to(DEV))
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 128, H, W) and net.dim == 128 and net.desc_div == 1
    s, d = score[0, 0].cpu().numpy(), desc[0].permute(1, 2, 0).contiguous().cpu().numpy()
    ref_s, ref_d = g["%dx%d.score" % (H, W)], g["%dx%d.desc" % (H, W)]
    so, do = oracle_maps[(H, W)]
    bar = desc_bar(ref_d)
    es, ed = float(np.abs(s - ref_s).max()), float(np.abs(desc_of(g, (H, W), d) - ref_d).max())
    eso, edo = float(np.abs(s - so).max()), float(np.abs(d - do).max())
    print("alike_l %dx%d %s: against the reference max |score error| %.3g (bar %.3g), max |desc error| %.3g (bar %.3g = 1e-4 x %.3g); against the oracle "
          "%.3g / %.3g (whole map)" % (H, W, MODE, es, SCORE_ATOL, ed, bar, bar / 1e-4, eso, edo))
    assert es <= SCORE_ATOL and ed <= bar
    assert eso <= SCORE_ATOL and edo <= desc_bar(do)
    assert np.abs(d).max() > 1.0                                        # not normalised, not unit-scale


# ------------------------------------------------------------------------------------------------ 2. batch
def test_a_batch_of_three_equals_the_single_image_runs_and_repeats_bit_for_bit(net):
    x = torch.from_numpy(np.stack([synthetic.image_pair(40 + i, 64, 96)[i & 1] for i in range(3)])).to(DEV)
    sb, db = net._run(x)
    sb, db = sb.clone(), db.clone()
    s2, d2 = net._run(x)
    assert torch.equal(sb, s2) and torch.equal(db, d2), "two identical runs differ"
    assert not torch.equal(sb[0], sb[1]) and not torch.equal(sb[1], sb[2])
    for i in range(3):
        si, di = net._run(x[i:i + 1].contiguous())
        es, ed = float((si[0] - sb[i]).abs().max()), float((di[0] - db[i]).abs().max())
        bar = desc_bar(di.cpu().numpy())
        print("alike_l batch of 3, image %d %s: against its single-image run max |score difference| %.3g, max |desc difference| %.3g (bar %.3g)" % (i, MODE, es, ed, bar))
        assert es <= SCORE_ATOL and ed <= bar
    assert torch.isfinite(sb).all() and torch.isfinite(db).all() and db.shape == (3, 64, 96, 128)


# ------------------------------------------------------------------------------------------------ 3. keypoint-only mode
def _points(H, W, n_random, seed):
    """Normalised (x, y) rows: the four image corners, exact integer pixels, points on the edges of the 2 / 8 / 32-pixel cells, then random ones."""
    px = lambda x, y: [x / (W - 1), y / (H - 1)]                        # grid_sample(align_corners = True): pixel (x, y) exactly
    rows = [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]
    rows += [px(5, 7), px(32, 32), px(W - 2, H - 2), px(17, 0), px(0, 23)]
    rows += [px(2.0, 3.5), px(8.0, 11.25), px(32.0, 40.5), px(31.5, 32.0), px(15.999, 8.001), px(63.5, 31.999)]
    rng = np.random.default_rng(seed)
    rows += rng.random((n_random, 2)).tolist()
    return np.asarray(rows, np.float32)


def test_keypoint_only_forward_and_desc_at_equal_the_dense_path(native):
    from keypoint_bench_amd.utils.matcher import sample_descriptors
    H, W, K = 64, 96, 48
    x = torch.from_numpy(np.stack([synthetic.image_pair(70, H, W)[0], synthetic.image_pair(71, H, W)[1]])).to(DEV)
    sd, dd = native.forward(x, dense=True)
    sd, dd = sd.clone(), dd.clone()
    sk, none = native.forward(x, dense=False)
    assert none is None
    es = float((sk - sd).abs().max())
    print("alike_l keypoint-only %s: max |score - dense score| %.3g (bar 2e-6)" % (MODE, es))
    assert es <= 2e-6
    pts = torch.from_numpy(np.stack([_points(H, W, K - 15, 1), _points(H, W, K - 15, 2)])).to(DEV)
    assert pts.shape == (2, K, 2)
    n = torch.tensor([K, 29], dtype=torch.int32, device=DEV)            # ragged: image 1 has 29 keypoints
    out = torch.full((2, K, 128), 7.0, dtype=torch.float32, device=DEV)
    ctx = native.ctx
    ctx.check(ctx.lib.kpb_net_desc_at(native.h, ptr(pts), 2, K, ptr(n), ptr(out)))
    ctx.sync()
    assert bool((out[1, 29:] == 7.0).all()), "rows at or past n[b] were written"
    scale = max(1.0, float(dd.abs().max()))
    for b, nb in ((0, K), (1, 29)):
        want = sample_descriptors(pts[b, :nb], dd[b:b + 1].permute(0, 3, 1, 2))
        e = float((out[b, :nb] - want).abs().max())
        print("alike_l desc_at image %d %s: max |desc_at - sample(dense)| %.3g (bar %.3g = 2e-5 x %.3g)" % (b, MODE, e, 2e-5 * scale, scale))
        assert e <= 2e-5 * scale
        assert float(want.abs().max()) > 0.5
    # three-column (x, y, score) rows, no count: every row written
    pts3 = torch.cat([pts[:1], torch.rand((1, K, 1), device=DEV)], dim=2).contiguous()
    out3 = torch.full((1, K, 128), 7.0, dtype=torch.float32, device=DEV)
    single = native.forward(x[:1].contiguous(), dense=False)[0]
    assert torch.equal(single[0], sk[0])
    ctx.check(ctx.lib.kpb_net_desc_at(native.h, ptr(pts3), 3, K, ptr(None), ptr(out3)))
    assert torch.equal(out3[0], out[0])


# ------------------------------------------------------------------------------------------------ 4. the two ways to load
def test_load_state_dict_and_load_packed_give_the_same_bits(net, folded):
    from keypoint_bench_amd.models.ALike import ALNet
    packed = ALNet().load_packed(weights.pack(folded, weights.ARCH_ALIKE)).eval()
    x = _img(3, 64, 96)
    s1, d1 = net(x)
    s1, d1 = s1.clone(), d1.clone()
    s2, d2 = packed(x)
    assert packed.dim == 128 and torch.equal(s1, s2) and torch.equal(d1, d2)


# ------------------------------------------------------------------------------------------------ 5. refusals through the C ABI
def _good_forward(native):
    x = _img(0, 32, 64)
    s, d = native.forward(x)
    return s.clone(), d.clone()


def test_a_shape_that_is_no_multiple_of_32_is_refused_and_nothing_is_written(native):
    s0, d0 = _good_forward(native)
    ctx = native.ctx
    for H, W in ((48, 48), (48, 64), (64, 48)):
        bad = torch.from_numpy(synthetic.image_pair(0, 64, 64)[0][:, :H, :W].copy())[None].to(DEV)
        score = torch.full((1, H, W), 7.0, device=DEV)
        desc = torch.full((1, H, W, 128), 7.0, device=DEV)
        rc = ctx.lib.kpb_net_forward(native.h, ptr(bad), 1, H, W, ptr(score), ptr(desc))
        assert rc == KPB_E_INVALID
        msg = ctx.lib.kpb_last_error(ctx.handle).decode()
        assert msg == "kpb_net_forward: ALIKE needs H and W multiples of 32 (got %dx%d)" % (H, W), msg
        ctx.sync()
        assert bool((score == 7.0).all()) and bool((desc == 7.0).all())
    s1, d1 = _good_forward(native)
    assert torch.equal(s0, s1) and torch.equal(d0, d1)


def test_a_blob_of_another_plan_is_refused_with_both_plans_named(native, folded):
    ctx = native.ctx
    rng = np.random.default_rng(0)
    c1, c2, c3, c4, dim = 16, 32, 64, 128, 128                          # ALIKE-n: the head is 129 x 128 as ALIKE-l's, the trunk is not
    n = {"b1c1.w": (c1, 3, 3, 3), "b1c1.b": (c1,), "b1c2.w": (c1, c1, 3, 3), "b1c2.b": (c1,)}
    for q, ci, co in (("b2", c1, c2), ("b3", c2, c3), ("b4", c3, c4)):
        n.update({q + "c1.w": (co, ci, 3, 3), q + "c1.b": (co,), q + "c2.w": (co, co, 3, 3), q + "c2.b": (co,), q + "ds.w": (co, ci), q + "ds.b": (co,)})
    n.update({"agg1.w": (dim // 4, c1), "agg2.w": (dim // 4, c2), "agg3.w": (dim // 4, c3), "agg4.w": (dim // 4, c4), "head.w": (dim + 1, dim)})
    alike_n = {k: rng.standard_normal(s).astype(np.float32) for k, s in n.items()}
    cases = [(alike_n, "b1c1.w"), ({k: v for k, v in folded.items() if k != "b3ds.b"}, "b3ds.b"), (dict(folded, **{"agg1.w": folded["agg1.w"][:, :16]}), "agg1.w")]
    ctx.prof_enable(True)
    try:
        ctx.prof_report()
        for tensors, name in cases:
            blob, h = weights.pack(tensors, weights.ARCH_ALIKE), c_void_p()
            rc = ctx.lib.kpb_net_create(ctx.handle, weights.ARCH_ALIKE, blob, len(blob), ctypes.byref(h))
            msg = ctx.lib.kpb_last_error(ctx.handle).decode()
            assert rc == KPB_E_WEIGHTS and not h.value, (rc, msg)
            assert msg == "kpb_net_create: tensor %s missing or not ALIKE shaped (this build supports c1..c4 = %s and c1..c4 = %s)" % ((name,) + BOTH_PLANS), msg
        assert ctx.prof_report() == {}, "a refused kpb_net_create launched a kernel"
    finally:
        ctx.prof_enable(False)
    s, d = _good_forward(native)                                        # the context is intact, and so is a net made before
    assert bool(torch.isfinite(s).all()) and float(d.abs().max()) > 0.5
    fresh = Native(weights.pack(folded, weights.ARCH_ALIKE))
    try:
        s2, d2 = _good_forward(fresh)
        assert fresh.dim == 128 and fresh.div == 1 and torch.equal(s, s2) and torch.equal(d, d2)
    finally:
        fresh.close()


def test_desc_at_before_a_forward_is_refused(folded):
    fresh = Native(weights.pack(folded, weights.ARCH_ALIKE))
    try:
        ctx = fresh.ctx
        pts = torch.rand((1, 8, 2), device=DEV)
        out = torch.full((1, 8, 128), 7.0, device=DEV)
        rc = ctx.lib.kpb_net_desc_at(fresh.h, ptr(pts), 2, 8, ptr(None), ptr(out))
        assert rc == KPB_E_INVALID
        assert ctx.lib.kpb_last_error(ctx.handle).decode() == "kpb_net_desc_at: no forward has run"
        ctx.sync()
        assert bool((out == 7.0).all())
        s, _ = fresh.forward(_img(0, 32, 64), dense=False)              # a good forward afterwards, and then the call goes through
        ctx.check(ctx.lib.kpb_net_desc_at(fresh.h, ptr(pts), 2, 8, ptr(None), ptr(out)))
        ctx.sync()
        assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ 6. strict fp32
@pytest.mark.timeout(600)
def test_strict_fp32_kernels_pass_the_same_fixtures():
    """KPB_FP32_MATRIX is read once per process: tests 1, 2 and 3 again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_alike_l.py::test_dense_forward_against_reference_fixture_and_oracle",
           "tests/test_gpu_alike_l.py::test_a_batch_of_three_equals_the_single_image_runs_and_repeats_bit_for_bit",
           "tests/test_gpu_alike_l.py::test_keypoint_only_forward_and_desc_at_equal_the_dense_path"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    tail = "\n".join(p.stdout.splitlines()[-30:])
    print(tail)
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % tail
    assert "7 passed" in tail and "skipped" not in tail.split("passed")[-1], tail
    assert "fp32:" in p.stdout and "split-f16" not in p.stdout


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_end_to_end_dense_lazy_and_pipeline_agree():
    from keypoint_bench_amd.models.ALike import LazyDescriptors
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import brute_force_matcher, match_descriptors, sample_descriptors
    H, W = 96, 160
    v = [synthetic.image_pair(90 + i, H, W) for i in range(2)]
    res = {}
    for dense in (True, False):
        m = _net(dense)
        per_pair = []
        for v0, v1 in v:
            s0, d0 = m(torch.from_numpy(v0)[None].to(DEV))
            s1, d1 = m(torch.from_numpy(v1)[None].to(DEV))
            assert isinstance(d0, LazyDescriptors) != dense and tuple(d0.shape) == (1, 128, H, W)
            k0, k1 = detection(s0, EP), detection(s1, EP)
            m0, m1 = brute_force_matcher(k0, k1, d0, d1, BF)
            pairs = match_descriptors(sample_descriptors(k0, d0), sample_descriptors(k1, d1), max_distance=BF["max_distance"], cross_check=True)
            per_pair.append((k0.cpu().numpy(), k1.cpu().numpy(), pairs.cpu().numpy(), m0.cpu().numpy(), m1.cpu().numpy()))
        res[dense] = per_pair
    for (k0, k1, pr, m0, m1), (l0, l1, lpr, lm0, lm1) in zip(res[True], res[False]):
        assert k0.shape[0] > 50 and pr.shape[0] > 10
        np.testing.assert_array_equal(k0.view(np.uint32), l0.view(np.uint32))
        np.testing.assert_array_equal(k1.view(np.uint32), l1.view(np.uint32))
        np.testing.assert_array_equal(pr, lpr)
        np.testing.assert_array_equal(m0, lm0)
        np.testing.assert_array_equal(m1, lm1)
    images = torch.from_numpy(np.concatenate([np.stack([a for a, _ in v]), np.stack([b for _, b in v])])).to(DEV)
    for dense in (True, False):
        pipe = PairPipeline(_net(dense), EP, BF, 2, H, W, device=DEV).run(images)
        for b in range(2):
            got = pipe.pair(b)
            k0, k1, pr, m0, m1 = res[True][b]
            np.testing.assert_array_equal(got["kps0"].view(np.uint32), k0.view(np.uint32))
            np.testing.assert_array_equal(got["kps1"].view(np.uint32), k1.view(np.uint32))
            np.testing.assert_array_equal(got["pairs"], pr)
            np.testing.assert_array_equal(got["m0"], m0)
            np.testing.assert_array_equal(got["m1"], m1)
