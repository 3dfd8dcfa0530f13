"""R2D2's single-f16 matrix mode (Quad_L2Net_ConfCFS(matrix="f16"): conv1 .. conv8 as one MFMA a_hi b_hi per product, csrc/conv_mfma.h CmForm::h1) on the GPU.

Accuracy is stated against the reference's own fp32 CPU outputs with its checkpoint (tests/golden/r2d2*.npz) and against the CPU emulation of the mode's
definition (tests/r2d2_matrix_fixtures.py).  Measured on an MI355X, 2026-10-21, largest error of the f16-mode net against the goldens, with the emulation's
error beside it:

    shape        |score error|  (emulation)     |desc error|  (emulation)
    64 x 96      1.462e-3       1.55e-3          6.74e-4       6.3e-4
    61 x 97      1.078e-3       1.09e-3          5.91e-4       6.0e-4
    24 x 40      9.70e-4        1.07e-3          4.98e-4       5.5e-4
    480 x 640    2.158e-3       (not emulated)   8.10e-4       (every eighth pixel)

(The split path at the same shapes: 3.5e-6 / 8.3e-7.)  At the shapes of FORM_SHAPES the device's error against the float64 chain was 0.76 .. 1.16 x the emulation's
(score) and 0.86 .. 0.95 x (descriptors); the device and the emulation themselves differ by up to 9e-4 / 4e-4 -- both are roundings of the same operands, and an
activation that differs in its last fp32 bit can round to the other f16 neighbour, so they agree in size of error, not value by value.

ATOL_F16_SCORE / ATOL_F16_DESC are twice the largest measured value, the rule tests/test_gpu_r2d2.py uses for ATOL_SCORE.  Two conditions hold whatever is
measured: the mode is ENGAGED (at 64 x 96 the score error is at least 1e-4: the split path's is 3.5e-6, so a net that silently ran the split kernels fails here),
and nothing but operand rounding is wrong (CAP: the device's error against a reference is at most 4 x the emulation's error against the same reference -- the
factor covers fp32 accumulation order and the few activations whose rounding flips between device and emulation; it is a cap, not the gate).  At shapes
without a golden the reference is the float64 chain of the plan table (tests/r2d2_fixtures.chain, held to the goldens by tests/test_r2d2_cpu.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic
from layer_net_shapes import constant_per_channel, is_constant
from r2d2_fixtures import SHAPES, checkpoint
from r2d2_matrix_fixtures import SMALL_SHAPES, case, errors, golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_F16_SCORE, MEASURED_F16_DESC = 2.158e-3, 8.10e-4      # largest over the four golden shapes (table above)
ATOL_F16_SCORE, ATOL_F16_DESC = 2 * MEASURED_F16_SCORE, 2 * MEASURED_F16_DESC
ENGAGED, CAP = 1e-4, 4.0
EP = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
BF = dict(metric="euclidean", max_distance=5, cross_check=True)
# shapes where the forms can go wrong: 8 x 8 (every conv8 tap is padding), 9 x 9 (only the four corner pixels have one conv8 tap inside the map), odd shapes below the dilation-16 reach, and
# several 16-row tiles and 128-pixel gemm_h row groups with ragged ends
FORM_SHAPES = ((8, 8), (9, 9), (15, 17), (17, 33), (24, 40), (136, 200))


def _f16():
    from keypoint_bench_amd.models.r2d2 import from_checkpoint
    return from_checkpoint(checkpoint(), matrix="f16")


def _split():
    from keypoint_bench_amd.models.r2d2 import from_checkpoint
    return from_checkpoint(checkpoint())


def _run(net, img):
    """(score [H,W], desc [H,W,128]) of one image [3,H,W], as numpy copies."""
    s, d = net(torch.from_numpy(np.array(img))[None].to(DEV))
    return s[0, 0].cpu().numpy(), d[0].permute(1, 2, 0).contiguous().cpu().numpy()


@pytest.fixture(scope="module")
def nets():
    """(split net, its outputs on the coexistence image BEFORE any f16 net existed in this module, f16 net)."""
    split = _split()
    img = case(7, 61, 97)["img"]
    before = _run(split, img)
    return split, before, _f16()


@pytest.fixture(scope="module")
def net(nets):
    return nets[2]


@pytest.mark.parametrize("H,W", SHAPES)
def test_f16_against_reference_golden(net, H, W):
    v0, _ = synthetic.image_pair(0, H, W)
    score, desc = net(torch.from_numpy(v0)[None].to(DEV))
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 128, H, W)
    np.testing.assert_allclose(torch.linalg.norm(desc[0], dim=0).cpu().numpy(), 1.0, rtol=0, atol=1e-5)
    d = desc[0].permute(1, 2, 0).cpu().numpy()
    if H >= 480:
        d = d[::8, ::8]
    es, ed = errors(score[0, 0].cpu().numpy(), d, golden(H, W))
    print("r2d2 f16 %dx%d vs golden: max |score error| %.4g, max |desc error| %.4g" % (H, W, es, ed))
    assert es <= ATOL_F16_SCORE and ed <= ATOL_F16_DESC
    if (H, W) == (64, 96):
        assert es >= ENGAGED, "the f16 net's score error %.3g is the split path's: the mode is not engaged" % es


@pytest.mark.parametrize("H,W", SMALL_SHAPES)
def test_f16_error_is_capped_by_the_emulation_at_the_goldens(net, H, W):
    c = case(0, H, W)
    es, ed = errors(*_run(net, c["img"]), golden(H, W))
    ms, md = errors(*c["emu"], golden(H, W))
    print("r2d2 f16 %dx%d vs golden: score %.4g (emulation %.4g, ratio %.2f), desc %.4g (emulation %.4g, ratio %.2f)" % (H, W, es, ms, es / ms, ed, md, ed / md))
    assert es <= CAP * ms and ed <= CAP * md


@pytest.mark.parametrize("H,W", FORM_SHAPES)
def test_f16_at_shapes_where_the_forms_can_go_wrong(net, H, W):
    c = case(40 + H + W, H, W)
    score, desc = _run(net, c["img"])
    assert score.shape == (H, W) and desc.shape == (H, W, 128)
    np.testing.assert_allclose(np.sqrt((desc.astype(np.float64) ** 2).sum(-1)), 1.0, rtol=0, atol=1e-5)
    es, ed = errors(score, desc, c["exact"])
    if is_constant(c["exact"][0]):
        # every conv8 tap is padding: conv8's output is its bias, one value per channel, and no rounded operand reaches it -- the emulation's own error is fp32
        # representation (1e-8) and caps nothing; what is left on the device is the fp32 head: a 128-term sum and a few operations on values below 1
        assert max(H, W) <= 8
        assert is_constant(score) and constant_per_channel(desc.transpose(2, 0, 1)), "%dx%d: the maps are not constant" % (H, W)
        print("r2d2 f16 %dx%d (bias only) vs float64 chain: score %.3g, desc %.3g" % (H, W, es, ed))
        assert es <= 2e-6 and ed <= 2e-6
        return
    ms, md = errors(*c["emu"], c["exact"])
    dev_emu = errors(score, desc, c["emu"])
    print("r2d2 f16 %dx%d vs float64 chain: score %.4g (emulation %.4g, ratio %.2f), desc %.4g (emulation %.4g, ratio %.2f); device vs emulation %.3g / %.3g"
          % (H, W, es, ms, es / ms, ed, md, ed / md, dev_emu[0], dev_emu[1]))
    assert es <= CAP * ms and ed <= CAP * md


@pytest.mark.parametrize("B,H,W", [(3, 17, 33), (5, 17, 33), (9, 24, 40)])
def test_f16_batching_does_not_change_bits(net, B, H, W):
    imgs = np.stack([case(60 + i, H, W)["img"] for i in range(B)])
    s, d = net(torch.from_numpy(imgs).to(DEV))
    s, d = s.clone(), d.clone()
    for i in range(B):
        si, di = net(torch.from_numpy(imgs[i])[None].to(DEV))
        assert torch.equal(si[0], s[i]) and torch.equal(di[0], d[i]), "image %d of %d" % (i, B)


def test_f16_three_runs_are_bit_identical(net):
    v0, v1 = synthetic.image_pair(4, 128, 160)
    x = torch.from_numpy(np.stack([v0, v1])).to(DEV)
    s0, d0 = net(x)
    s0, d0 = s0.clone(), d0.clone()
    for _ in range(2):
        s, d = net(x)
        assert torch.equal(s, s0) and torch.equal(d, d0)


def test_split_and_f16_nets_coexist(nets):
    split, before, f16 = nets
    img = case(7, 61, 97)["img"]
    first = _run(f16, img)
    for _ in range(2):          # alternately, on the one context
        s, d = _run(split, img)
        assert np.array_equal(s.view(np.uint32), before[0].view(np.uint32)) and np.array_equal(d.view(np.uint32), before[1].view(np.uint32))
        fs, fd = _run(f16, img)
        assert np.array_equal(fs.view(np.uint32), first[0].view(np.uint32)) and np.array_equal(fd.view(np.uint32), first[1].view(np.uint32))
    assert not np.array_equal(first[0], before[0]) and not np.array_equal(first[1], before[1])
    assert split.matrix == "split" and f16.matrix == "f16"


def test_profile_names_tell_the_modes_apart(nets):
    from keypoint_bench_amd._lib import Context
    split, _, f16 = nets
    ctx = Context.get(torch.device(DEV))
    x = torch.from_numpy(np.array(case(7, 61, 97)["img"]))[None].to(DEV)
    layers = ["conv%d" % i for i in range(1, 9)]         # the split net's names, as they have always been
    ctx.prof_enable(True)
    try:
        ctx.prof_report()
        f16(x)
        rep = ctx.prof_report()
        print("f16:", sorted(rep))
        assert all("r2d2_" + n + "_h1" in rep and n not in rep and "r2d2_" + n not in rep for n in layers), sorted(rep)
        assert "r2d2_conv0" in rep and "r2d2_head" in rep and "r2d2_conv0_h1" not in rep
        split(x)
        rep = ctx.prof_report()
        print("split:", sorted(rep))
        assert all(n in rep for n in layers) and not [n for n in rep if n.endswith("_h1")], sorted(rep)
    finally:
        ctx.prof_enable(False)


def _child(code, env=None):
    """`code` in a fresh python (subprocess.run: KPB_FP32_MATRIX is read once per process, and a refused create is best seen in a process of its own)."""
    head = "import sys; sys.path[:0] = [%r, %r]\n" % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", head + code], cwd=ROOT, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-2000:]
    return p.stdout


def test_f16_is_refused_on_the_strict_fp32_build():
    out = _child("""
import torch
from keypoint_bench_amd.models.r2d2 import from_checkpoint
from r2d2_fixtures import checkpoint
net = from_checkpoint(checkpoint(), matrix="f16")
x = torch.zeros((1, 3, 24, 40), device="cuda:0")
try:
    net(x)
except NotImplementedError as e:
    assert "KPB_FP32_MATRIX" in str(e) and "kpb_net_create: R2D2" in str(e), str(e)
    print("REFUSED:", e)
else:
    raise SystemExit("the f16 net ran on the strict-fp32 build")
s, d = from_checkpoint(checkpoint())(x)       # the split net of the same process still runs
assert bool(torch.isfinite(s).all())
""", env={"KPB_FP32_MATRIX": "1"})
    assert "REFUSED:" in out


def test_other_archs_refuse_a_blob_that_asks_for_the_mode():
    out = _child("""
import ctypes
import numpy as np
import torch
from keypoint_bench_amd import weights
from keypoint_bench_amd._lib import Context, KpbError, c_void_p
from keypoint_bench_amd.models.SuperPoint import superpoint_random
from keypoint_bench_amd.models.disk import disk_random
ctx = Context.get(torch.device("cuda:0"))
for model in (superpoint_random(7), disk_random(5)):
    arch, t = weights.unpack(model._blob)
    assert arch != weights.ARCH_R2D2
    for value, refused in ((1.0, True), (0.0, False)):
        blob = weights.pack(dict(t, **{"matrix.mode": np.array([value], np.float32)}), arch)
        h = c_void_p()
        rc = ctx.lib.kpb_net_create(ctx.handle, arch, blob, len(blob), ctypes.byref(h))
        if refused:
            assert rc == -7 and not h.value, (arch, rc)
            msg = ctx.lib.kpb_last_error(ctx.handle).decode()
            assert msg.startswith("kpb_net_create:") and "matrix.mode" in msg, msg
            print("REFUSED arch %d: %s" % (arch, msg))
        else:
            assert rc == 0, (arch, rc)
            ctx.lib.kpb_net_destroy(h)
""")
    assert out.count("REFUSED arch") == 2


def test_f16_feeds_detection_like_the_oracle(net):
    import oracle
    from keypoint_bench_amd.utils.extracter import detection
    v0, _ = synthetic.image_pair(8, 128, 160)
    s0, _ = net(torch.from_numpy(v0)[None].to(DEV))
    ep = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
    k0 = detection(s0, ep)
    ok0, _ = oracle.detection(s0[0, 0].cpu().numpy(), ep)
    np.testing.assert_array_equal(k0.cpu().numpy().view(np.uint32), ok0.view(np.uint32))


def test_f16_pipeline_equals_single_pair_path(nets):
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import match_descriptors, sample_descriptors
    B, H, W = 4, 128, 160
    v = [synthetic.image_pair(20 + i, H, W) for i in range(B)]
    i0, i1 = np.stack([a for a, _ in v]), np.stack([b for _, b in v])
    images = torch.from_numpy(np.concatenate([i0, i1])).to(DEV)
    pipe = PairPipeline(_f16(), EP, BF, B, H, W, device=DEV)
    pipe.run(images)
    got = [pipe.pair(b) for b in range(B)]
    single = nets[2]
    for b in range(B):
        s0, d0 = single(torch.from_numpy(i0[b])[None].to(DEV))
        k0 = detection(s0, EP)
        f0 = sample_descriptors(k0, d0)
        s1, d1 = single(torch.from_numpy(i1[b])[None].to(DEV))
        k1 = detection(s1, EP)
        f1 = sample_descriptors(k1, d1)
        np.testing.assert_array_equal(got[b]["kps0"], k0.cpu().numpy())
        np.testing.assert_array_equal(got[b]["kps1"], k1.cpu().numpy())
        pairs, dist = match_descriptors(f0, f1, max_distance=5, cross_check=True, return_distance=True)
        np.testing.assert_array_equal(got[b]["pairs"], pairs.cpu().numpy())
        np.testing.assert_array_equal(got[b]["dist"], dist.cpu().numpy())
        assert got[b]["kps0"].shape[0] > 20
    # against the split net on the same pairs: reported, not gated
    ps = PairPipeline(nets[0], EP, BF, B, H, W, device=DEV)
    ps.run(images)
    for b in range(B):
        ref = ps.pair(b)
        xy = lambda k: set(map(tuple, np.asarray(k)[:, :2].tolist()))       # keypoints sit on pixel centres: the same floats in both modes
        k0s, k0f, k1s, k1f = ref["kps0"], got[b]["kps0"], ref["kps1"], got[b]["kps1"]
        ms = {(tuple(k0s[i, :2]), tuple(k1s[j, :2])) for i, j in np.asarray(ref["pairs"])[:, :2].astype(int)}
        mf = {(tuple(k0f[i, :2]), tuple(k1f[j, :2])) for i, j in np.asarray(got[b]["pairs"])[:, :2].astype(int)}
        print("pair %d: keypoints split %d / f16 %d, common %d; matches split %d / f16 %d, common %d"
              % (b, len(k0s), len(k0f), len(xy(k0s) & xy(k0f)), len(ms), len(mf), len(ms & mf)))
