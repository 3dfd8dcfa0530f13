"""Key.Net (csrc/keynet.hip) at the shapes and batches its code depends on, against the float64 chain.  tests/test_gpu_keynet.py compares with goldens at
16 x 16, 30 x 50, 37 x 61, 96 x 160 and 480 x 640 (seed 0, H <= W) and one batch of 3 with its own solo runs; no shape there was steered at a tile edge, a
pyramid scale or a strip.  Here every FULL map is compared with keynet_fixtures.chain on the folded checkpoint, run by keynet_shapes.oracle in fp32 and, with
tensors and image cast, in float64, on one net object that goes through all shapes in turn.  tests/test_keynet_shape_oracles_cpu.py shows without a GPU that the
chains are finite at these shapes, that the level sizes are the literal table's, and that a chain with one edge rule wrong misses 16 x ref_err at every shape.

  shape sweep   nine shapes, one image each (keynet_shapes.LEVELS; the sweep test's docstring says what each is for)
  batch sweep   B different images (different seeds, alternating views): 5 at 21 x 40, 17 at 20 x 39, 3 at 47 x 78; every image against the float64 chain,
                images 0, B // 2 and B - 1 against the same net run on that image alone, bit for bit
  strict fp32   both sweeps again in a child process under KPB_FP32_MATRIX=1

Bound; none is chosen here.  max |device - chain64| <= M x ref_err with M_H16 / M_FP32 of keynet_fixtures, ref_err = max |chain32 - chain64| of the same pixels,
floored at one fp32 unit in the last place of the float64 map's maximum; the border ring (outermost 8 pixels) and the interior apart where the interior has at
least 256 pixels, else the whole map (keynet_shapes.regions).  The score is finite and non-negative.  Every figure is printed before it is asserted.

The measured ratios of both arithmetics are in the docstring of tests/keynet_shapes.py.  Largest: 2.121 (split-f16, 5 at 21 x 40) and 1.926 (strict
fp32, the same batch); no shape needed a multiplier of its own and none exposed a defect.  Wall time on an MI355X host: the whole file 6.8 s, 4.3 s of them the
strict-fp32 child; the slowest case 0.35 s (16 x 640, which also creates the net), every other under 0.15 s; both chains on the CPU take at most 0.04 s a case."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from keypoint_bench_amd import weights
from keynet_fixtures import PLAN, checkpoint
from keynet_shapes import BATCHES, BATCH_LEVELS, SHAPES, batch_images, check_levels, judge, multiplier, oracle, sid, sweep_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32 = os.environ.get("KPB_FP32_MATRIX") == "1"
ARITH = "fp32" if FP32 else "split-f16"


@pytest.fixture(scope="module")
def net():
    """One net object for the whole file: it goes through every shape in turn, as a caller's would."""
    from keypoint_bench_amd.models.KeyNet import KeyNet
    net = KeyNet(PLAN)
    net.load_state_dict(checkpoint())
    return net.eval()


def _check_images(imgs, score, tag):
    """score [B,1,H,W] (GPU tensor) of imgs [B,3,H,W] against the chains: shape, finiteness, sign, values."""
    B, _, H, W = imgs.shape
    assert tuple(score.shape) == (B, 1, H, W) and score.dtype == torch.float32, (tag, tuple(score.shape))
    s = score[:, 0].cpu().numpy()
    t0 = time.perf_counter()
    r32, r64 = oracle(imgs), oracle(imgs, double=True)
    print("keynet case %s %s: both chains on the CPU took %.2f s" % (tag, ARITH, time.perf_counter() - t0))
    assert np.isfinite(r32).all() and np.isfinite(r64).all(), tag + ": the oracle itself is not finite here"
    M = multiplier()[FP32]
    failed = []
    for i in range(B):
        ti = tag if B == 1 else "%s image %d of %d" % (tag, i, B)
        assert np.isfinite(s[i]).all() and float(s[i].min()) >= 0.0, ti + ": the score is not finite and non-negative"
        for name, err, ref in judge(s[i], r32[i], r64[i]):
            print("keynet %s %s %s: max |gpu - chain64| = %.4g, ref_err = %.4g (max score %.6g): ratio %.3f, M = %d" % (ti, ARITH, name, err, ref, float(r64[i].max()), err / ref, M))
            if err > M * ref:
                failed.append("%s, %s: %.4g > %d x %.4g (ratio %.3f)" % (ti, name, err, M, ref, err / ref))
    assert not failed, "the score is off: " + "; ".join(failed)


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_keynet_shape_sweep_against_the_float64_chain(net, shape):
    """16 x 640: a strip one tile high and twenty wide; levels of 13 and 10 rows are below one tile, 13 -> 10 is scale 1.3, the widest window keynet_pyrdown's
    28 x 28 staging is argued for.  640 x 16: the transpose -- one pair-column tile wide, forty high, 16 -> 13 -> 10 columns.  17 x 33: one past a tile both ways
    at level 0 (a second tile row of one pixel row, a second tile column of one pixel), odd H: the head's last thread pair is half a pair.  20 x 39: level 1 is
    exactly one 16 x 32 tile, 20 -> 16 is scale 1.25.  21 x 40: level 1 is 17 x 33 -- one past a tile, the last accumulator pair of keynet_conv5_h straddles
    the frame.  33 x 65: one past two tiles at level 0.  47 x 78: 78 -> 65 is scale 1.2 exactly, level 2 is exactly two tiles high.  31 x 97: one short of a tile
    edge in H, one past in W.  64 x 129: several tiles, one past 128."""
    H, W = shape
    check_levels(H, W)
    imgs = sweep_image(H, W)
    score, none = net(torch.from_numpy(imgs).to(DEV))
    assert none is None
    _check_images(imgs, score, "%dx%d" % shape)


@pytest.mark.parametrize("B,shape", BATCHES, ids=sid)
def test_a_batch_of_different_images_equals_the_chain_and_the_single_images(net, B, shape):
    """Every image of the batch against the float64 chain, and images 0, B // 2, B - 1 against the net run on that image alone, BIT FOR BIT: the batch is
    blockIdx.z in every kernel, and keynet_conv5_h scales a tile by that tile's own largest magnitude."""
    assert tuple(weights.keynet_level_sizes(*shape)[1:]) == BATCH_LEVELS[shape]
    imgs = batch_images(B, *shape)
    sb, none = net(torch.from_numpy(imgs).to(DEV))
    assert none is None
    sb = sb.clone()
    _check_images(imgs, sb, "%d at %dx%d" % ((B,) + shape))
    for i in (0, B // 2, B - 1):
        s1, _ = net(torch.from_numpy(imgs[i:i + 1]).to(DEV))
        assert torch.equal(s1[0], sb[i]), "score of image %d of %d differs from the single-image run (max %.3g)" % (i, B, float((s1[0] - sb[i]).abs().max()))
    assert not torch.equal(sb[0], sb[B - 1])        # (different images)


@pytest.mark.timeout(300)
def test_strict_fp32_kernels_pass_both_sweeps():
    """KPB_FP32_MATRIX is read once per process: the shape and batch sweeps again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    tests = ["test_keynet_shape_sweep_against_the_float64_chain", "test_a_batch_of_different_images_equals_the_chain_and_the_single_images"]
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"] + ["tests/test_gpu_keynet_shapes.py::" + t for t in tests]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=250)
    out = p.stdout
    print("\n".join(l for l in out.splitlines() if " fp32 " in l or "passed" in l or "failed" in l))
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % "\n".join(out.splitlines()[-40:])
    n = len(SHAPES) + len(BATCHES)
    last = out.splitlines()[-1]
    assert "%d passed" % n in last and "skipped" not in last and "failed" not in last, last
    assert out.count(" fp32: both chains") == n and " split-f16" not in out      # the fp32 tag once per case: every case of the child ran under the knob
