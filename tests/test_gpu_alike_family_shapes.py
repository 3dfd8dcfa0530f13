"""GoodPoint, LETNet, EdgePoint (csrc/alike.hip) and ALIKE-l (csrc/alike_l.hip on the conv_layer.hip launchers) at shapes and batches their goldens never had.
The goldens are 32 x 32, 32 x 64, 64 x 96, 96 x 160 and 480 x 640 (ALIKE-l: 160 x 224), seed 0, never taller than wide, never one tile wide; the batches of the
per-net files are compared with their own solo runs or across launch regimes, never with a reference.  A swapped H and W, a pitch taken from the wrong side, or
a coarse map of 3 x 1 where 1 x 3 was meant would pass there.  ALIKE-t got such shapes in tests/test_gpu_alike.py; this file gives them to its four siblings.

Each test compares the FULL maps the forward returns (score; descriptor or tracking map at the net's own layout and divisor) with the net's reference
(alike_family_shapes.references: the fixtures' chains, oracle.alike_ref.alnet_forward for ALIKE-l) on one net object per architecture that goes through every
shape in turn.  tests/test_alike_family_shape_oracles_cpu.py shows without a GPU that the references are finite at these shapes and that two wrong variants per
net miss the bound used here at every sweep shape.

  shape sweep   (96, 32) and (160, 32): a tall column one tile wide, coarse maps 3 x 1 and 5 x 1; (32, 288): a strip whose width is a multiple of neither the
                64-wide (GP_TW, HP_BW) nor the 128-wide (SEG_TILES) unit; (224, 96) and (96, 224): odd multiples of 32 both ways, taller than wide, and the transpose
  batch sweep   B different images (different seeds, alternating views): 5 at 32 x 96, 17 at 32 x 64 (past the `batch >= 16` switch of the shared trunk), 3 at
                96 x 32; every image against the reference; images 0, B // 2 and B - 1 against their solo runs at the bar the net's own file uses for that:
                bit equality for GoodPoint, LETNet and EdgePoint, the score and descriptor bars for ALIKE-l
  strict fp32   both sweeps again in a child process under KPB_FP32_MATRIX=1

Bound; none is chosen here.  The per-net file's bars against the fp32 reference (alike_family_shapes.bars: ATOL_SCORE / ATOL_DESC of tests/test_gpu_goodpoint.py,
test_gpu_letnet.py and test_gpu_edgepoint.py; ALIKE-l's SCORE_ATOL and desc_bar, which scales with max(1, max |desc_ref|)); a comparison that misses by magnitude
is settled as tests/test_gpu_net_shapes.py settles it, max |device - ref64| <= 4 x max |ref32 - ref64|.  EdgePoint's score is a signed logit, compared unclamped.
Every figure is printed before it is asserted.  The measured errors of both arithmetics, and which (net, shape) pairs needed the float64 rule, are in the
docstring of tests/alike_family_shapes.py.  Wall time on an MI355X host: the whole file 7.9 s, 4.6 s of them the
strict-fp32 child; the slowest case 0.43 s (the first, which opens the device), every other under 0.1 s."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from alike_family_shapes import BATCHES, BITWISE, DESC, NETS, SHAPES, bars, images, references, rule, sid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32 = os.environ.get("KPB_FP32_MATRIX") == "1"
ARITH = "fp32" if FP32 else "split-f16"


@functools.lru_cache(maxsize=None)
def _net(name):
    """One net object per architecture for the whole file: it goes through every shape in turn, as a caller's would."""
    if name == "goodpoint":
        from goodpoint_fixtures import PARAM, checkpoint
        from keypoint_bench_amd.models.GoodPoint import GoodPoint
        net = GoodPoint(PARAM)
        net.load_state_dict(checkpoint())
    elif name == "letnet":
        from keypoint_bench_amd.models.LETNet import LETNet
        from letnet_fixtures import checkpoint
        net = LETNet(c1=8, c2=16, grayscale=False)
        net.load_state_dict(checkpoint())
    elif name == "edgepoint":
        from edgepoint_fixtures import PARAM, checkpoint
        from keypoint_bench_amd.models.EdgePoint import EdgePoint
        net = EdgePoint(PARAM)
        net.load_state_dict(checkpoint())
    else:
        from alike_l_fixtures import state_dict
        from keypoint_bench_amd.models.ALike import ALNet
        net = ALNet(dense_descriptors=True)
        net.load_state_dict(state_dict())
    return net.eval()


def _forward(name, imgs):
    """(score [B,1,H,W], map [B,C,H/div,W/div]) as GPU tensors of their own: a later forward of the same net does not write to them."""
    score, desc = _net(name)(torch.from_numpy(imgs).to(DEV))
    return score.clone(), desc.contiguous().clone()


def _check_images(name, B, shape, score, desc):
    """The maps of `images(B, shape)` against the references: shapes, finiteness, values."""
    H, W = shape
    C, div = DESC[name]
    tag = "%s %s%dx%d" % (name, "" if B == 1 else "%d at " % B, H, W)
    assert tuple(score.shape) == (B, 1, H, W) and tuple(desc.shape) == (B, C, H // div, W // div), (tag, tuple(score.shape), tuple(desc.shape))
    assert score.dtype == desc.dtype == torch.float32
    assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(desc).all()), tag + ": non-finite output"
    t0 = time.perf_counter()
    (s32, d32), (s64, d64) = references(name, B, shape)
    print("alike-family case %s %s: both references on the CPU took %.2f s" % (tag, ARITH, time.perf_counter() - t0))
    s, d = score[:, 0].cpu().numpy(), desc.cpu().numpy()
    failed = []
    for i in range(B):
        ti = tag if B == 1 else "%s image %d of %d" % (tag, i, B)
        for what, got, r32, r64, atol in zip(("score", "map"), (s[i], d[i]), (s32[i], d32[i]), (s64[i], d64[i]), bars(name, d32[i])):
            e32, e64, e_ref, holds = rule(got, r32, r64, atol)
            print("%s %s %s: max |gpu - ref32| = %.3g (bar %.3g: %s); max |gpu - ref64| = %.3g, e_ref = %.3g: ratio %.3f"
                  % (ti, ARITH, what, e32, atol, "holds" if e32 <= atol else "MISSED", e64, e_ref, e64 / max(e_ref, 1e-30)))
            if not holds:
                failed.append("%s %s: beyond %.3g of the fp32 reference (max %.3g) and beyond 4 x the reference's own fp32 error (%.3g > 4 x %.3g)"
                              % (ti, what, atol, e32, e64, e_ref))
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
@pytest.mark.parametrize("name", NETS)
def test_shape_sweep_against_the_reference(name, shape):
    score, desc = _forward(name, images(1, shape))
    _check_images(name, 1, shape, score, desc)


@pytest.mark.parametrize("B,shape", BATCHES, ids=sid)
@pytest.mark.parametrize("name", NETS)
def test_a_batch_of_different_images_equals_the_reference_and_the_single_images(name, B, shape):
    imgs = images(B, shape)
    sb, db = _forward(name, imgs)
    _check_images(name, B, shape, sb, db)
    for i in (0, B // 2, B - 1):
        s1, d1 = _forward(name, imgs[i:i + 1])
        es, ed = float((s1[0] - sb[i]).abs().max()), float((d1[0] - db[i]).abs().max())
        if name in BITWISE:
            assert torch.equal(s1[0], sb[i]), "%s: score of image %d of %d differs from the single-image run (max %.3g)" % (name, i, B, es)
            assert torch.equal(d1[0], db[i]), "%s: map of image %d of %d differs from the single-image run (max %.3g)" % (name, i, B, ed)
        else:
            bs, bd = bars(name, d1[0].cpu().numpy())
            print("%s %d at %dx%d image %d %s against its single-image run: max |score difference| %.3g (bar %.3g), max |map difference| %.3g (bar %.3g)"
                  % ((name, B) + shape + (i, ARITH, es, bs, ed, bd)))
            assert es <= bs and ed <= bd
    assert not torch.equal(sb[0], sb[B - 1])        # (different images)


@pytest.mark.timeout(600)
def test_strict_fp32_kernels_pass_both_sweeps():
    """KPB_FP32_MATRIX is read once per process: the shape and batch sweeps again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    tests = ["test_shape_sweep_against_the_reference", "test_a_batch_of_different_images_equals_the_reference_and_the_single_images"]
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"] + ["tests/test_gpu_alike_family_shapes.py::" + t for t in tests]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=500)
    out = p.stdout
    print("\n".join(l for l in out.splitlines() if " fp32 " in l or "passed" in l or "failed" in l))
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % "\n".join(out.splitlines()[-40:])
    n = len(NETS) * (len(SHAPES) + len(BATCHES))
    last = out.splitlines()[-1]
    assert "%d passed" % n in last and "skipped" not in last and "failed" not in last, last
    assert out.count(" fp32: both references") == n and " split-f16" not in out     # the fp32 tag once per case: every case of the child ran under the knob
