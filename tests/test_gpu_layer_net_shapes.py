"""Every image shape and batch kpb_net_forward accepts for R2D2, SFD2 and D2-Net -- the three nets whose launch_mfma forms (csrc/conv_layer.hip) no other net
runs: conv_mfma_h with dilation 2 and 4 (8-row tiles, a halo of 8), the tap-gathered gemm_h<2, 1, GE_PLAIN, false, 2>, the stride-2 forms on 8-row tiles,
gemm_h<.., GE_RES_RELU>, 1 x 1 layers of 65 and 3 output channels, the pool_out forms on maps half a tile high, a 512-channel head.  tests/test_gpu_net_shapes.py
is the same file for SuperPoint, DISK and XFeat; the per-net files compare with goldens at four or five fixed shapes and batches of 2 or 3.

Each test compares the FULL maps with the nets' torch.nn.functional chains (r2d2_fixtures / sfd2_fixtures / d2net_fixtures .chain, run by layer_net_shapes.oracle
in fp32 and, with tensors and image cast, in float64) on one net object per architecture: R2D2 with the fixture checkpoint, SFD2 and D2-Net with their seeded
stand-in state dicts.  tests/test_layer_net_shape_oracles_cpu.py shows without a GPU that the oracles are finite at all these shapes and that a chain with one
edge rule wrong falls outside the bounds used here.

  shape sweep   one parametrized test per net; its docstring says what each shape is for
  batch sweep   B different images (different seeds, alternating views): R2D2 3 and 5 at 17 x 33 and 9 at 24 x 40, SFD2 and D2-Net 3 and 5 at 24 x 40 and 17 at
                16 x 24; every image against the oracle, images 0, B // 2 and B - 1 against the same net run on that image alone, bit for bit
  refusals      the size limits: R2D2 a side of 32768 (and with it every H x W above 2^30: 32767^2 is below), SFD2 and D2-Net a side of 16392 and a batch of 8192
  strict fp32   the two sweeps again in a child process under KPB_FP32_MATRIX=1

Tolerances; none is chosen here.
  R2D2          ATOL_SCORE / ATOL_DESC of tests/test_gpu_r2d2.py against the fp32 chain; a comparison that misses by magnitude is settled by the float64 rule of
                tests/test_gpu_net_shapes.py with its factor 4: max |gpu - chain64| <= 4 max |chain32 - chain64|.  Descriptors are unit vectors to 1e-5.  With
                min(H, W) <= 8 every conv8 tap is padding: the maps must hold ONE value per channel (conv8's row is its bias at every pixel, and r2d2_head is
                the same arithmetic at every pixel), the score 0.185.
  SFD2, D2-Net  the per-net files' rule max |gpu - chain64| <= M ref_err with M_H16 / M_FP32 of the fixtures, ref_err = max |chain32 - chain64| at that
                shape, floored at one fp32 unit in the last place of the float64 map's largest magnitude (a smaller ref_err is an accident of rounding in the
                reference, not accuracy a correct fp32 result can reach).  SFD2's score leaves out the pixels whose two largest upsampled stability logits are
                closer than MARGIN in float64, at most 1 % of a shape.  Where D2-Net's oracle score is exactly constant the device must give its bits.

Measured on an MI355X, the largest max |gpu - chain64| / ref_err, score / descriptors (R2D2: e_ref for ref_err, and the largest max |gpu - chain32|):
                            split-f16, shape sweep             batch sweep                          strict fp32, shape sweep           batch sweep
  R2D2    ratio             1.925 (17x33) / 2.119 (9x9)        2.845 (9 at 24x40) / 1.829           3.055 (15x17) / 5.556 (9x9)        3.992 (9 at 24x40) / 3.486
          |gpu - chain32|   1.88e-6 (136x200) / 8.05e-7        (atol 6.92e-6 / 1e-4)                2.86e-6 / 1.13e-6 (9 at 24x40)
  SFD2    ratio             3.387 (24x40) / 2.066 (24x40)      4.192 (17 at 16x24) / 1.959          3.262 (8x264) / 2.430 (24x8)       5.459 (5 at 24x40) / 2.250
  D2-Net  ratio             5.714 (24x40) / 3.487 (120x160)    9.491 (17 at 16x24) / 3.454          7.240 (24x40) / 4.325 (264x328)    11.179 (17 at 16x24) / 4.187
R2D2 held ATOL_SCORE / ATOL_DESC everywhere: no comparison needed the float64 rule (its ratios are printed all the same).  The constant maps are constant on the
device too, score 0.185273141 as in the chain.  SFD2 stays under the fixtures' M_H16 = M_FP32 = 8; at most 5 of 960 pixels were unsure (0.52 %).

D2-Net's score at 16 x 24 exceeds the fixtures' M_H16 = 8 on two of the 17 images (8.968 and 9.491 on images 5 and 8, 7.685 on image 1; strict fp32 11.179,
8.059 and 7.154 on images 1, 5 and 12) with no defect: the descriptors of the same runs -- the conv4_3 map the score is computed from -- stay at 3.5 / 4.2, images
1 and 5 stand out in both arithmetics, and most other images of the same launch are at 1 - 3.  The map has six cells, each about 0.19 (one fp32 unit in the last place: 1.5e-8).  A cell is exp(x / m) over its
window's sum, divided by the image's sum, so it carries conv4_3's relative error (ten layers, K up to 4608, summed in the MFMA's order: about 1e-6) as an absolute
2 - 4e-7 -- what is measured.  ref_err there is 3.3 - 6.9e-8, two to five units in the last place: oneDNN's blocked sums happen to land that close on these six
values, and the largest of six is a small sample.  Torch's own fp32 convolution without oneDNN, the same chain in another order, is 2.3 to 32.7 x ref_err off
the float64 chain on these 17 images (measured on the CPU).  By the fixtures' rule (the smallest power of two that is at least twice the largest measured ratio,
never above 16) this file's D2-Net multiplier is layer_net_shapes.M_D2NET = 16 for both arithmetics -- the cap, not twice 11.179; d2net_fixtures and
tests/test_gpu_d2net.py keep theirs.  No test of this file failed for a defect in csrc.

The float64 and fp32 chains together take 0.32 s on the GPU host's CPU at the largest shape (D2-Net 264 x 328; R2D2 136 x 200 0.26 s); the whole file runs in
about 10 s, 6 s of them the strict-fp32 child."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from layer_net_shapes import (BATCHES, DESC, SHAPES, UNSURE_CAP, batch_images, constant_per_channel, image, is_constant, multiplier, oracle, r2d2_atols, r2d2_rule,
                              ratio_rule, sid, sweep_image)
from sfd2_fixtures import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KPB_E_INVALID = -1
FP32 = os.environ.get("KPB_FP32_MATRIX") == "1"
ARITH = "fp32" if FP32 else "split-f16"
NAME = {"r2d2": "R2D2", "sfd2": "SFD2", "d2net": "D2Net"}       # as the library's messages spell them


@functools.lru_cache(maxsize=None)
def _net(name):
    """One net object per architecture for the whole file: it goes through every shape in turn, as a caller's would."""
    if name == "r2d2":
        from keypoint_bench_amd.models.r2d2 import from_checkpoint
        from r2d2_fixtures import checkpoint
        return from_checkpoint(checkpoint())
    if name == "sfd2":
        from keypoint_bench_amd.models.sfd2 import ResSegNetV2
        from sfd2_fixtures import state_dict
        net = ResSegNetV2(outdim=128, require_stability=True)
        net.load_state_dict(state_dict(), strict=False)
        return net.eval()
    from d2net_fixtures import state_dict
    from keypoint_bench_amd.models.D2_Net import D2Net
    net = D2Net(use_cuda=True)
    net.load_state_dict(state_dict())
    return net.eval()


def _check_r2d2(tag, score, desc, o32, o64):
    H, W = score.shape
    np.testing.assert_allclose(np.sqrt((desc.astype(np.float64) ** 2).sum(0)), 1.0, rtol=0, atol=1e-5, err_msg=tag + ": descriptors are not unit vectors")
    if min(H, W) <= 8:
        print("%s: every conv8 tap is padding; score %.9g (chain %.9g)" % (tag, float(score.max()), float(o32[0].max())))
        assert is_constant(score) and constant_per_channel(desc), tag + ": the maps are not constant"
    for what, got, r32, r64, atol in zip(("score", "desc"), (score, desc), o32, o64, r2d2_atols()):
        e32, e64, e_ref, holds = r2d2_rule(got, r32, r64, atol)
        print("%s %s %s: max |gpu - chain32| = %.3g (atol %.3g: %s); max |gpu - chain64| = %.3g, e_ref = %.3g: ratio %.3f"
              % (tag, ARITH, what, e32, atol, "holds" if e32 <= atol else "MISSED", e64, e_ref, e64 / max(e_ref, 1e-30)))
        assert holds, "%s %s: beyond %g of the fp32 chain (max %.3g) and beyond 4 x the chain's own fp32 error (%.3g > 4 x %.3g)" % (tag, what, atol, e32, e64, e_ref)


def _check_ratio(name, tag, score, desc, o32, o64):
    M = multiplier(name)[FP32]
    np.testing.assert_allclose(np.sqrt((desc.astype(np.float64) ** 2).sum(0)), 1.0, rtol=0, atol=1e-5, err_msg=tag + ": descriptors are not unit vectors")
    assert float(score.min()) >= 0.0
    keep = None
    if name == "sfd2":
        keep = o64[2] >= MARGIN
        print("%s: %d of %d pixels unsure" % (tag, int((~keep).sum()), keep.size))
        assert float((~keep).mean()) <= UNSURE_CAP
    if name == "d2net" and is_constant(o32[0]) and is_constant(o64[0]):         # as the 8 x 8 golden: nothing to round
        assert np.array_equal(score.view(np.uint32), o32[0].view(np.uint32)), tag + ": the score is not the oracle's constant %r" % float(o32[0].max())
    for what, got, r32, r64, k in (("score", score, o32[0], o64[0], keep), ("desc", desc, o32[1], o64[1], None)):
        err, ref = ratio_rule(got, r32, r64, k)
        print("%s %s %s: max |gpu - chain64| = %.4g, ref_err = %.4g: ratio %.3f, M = %d" % (tag, ARITH, what, err, ref, err / ref, M))
        assert err <= M * ref, "%s: the %s is off: %.4g > %d x %.4g" % (tag, what, err, M, ref)


def _check_images(name, imgs, score, desc, tag):
    """score [B,1,H,W] and desc [B,C,H/div,W/div] (GPU tensors) of imgs [B,3,H,W] against the chains: shapes, finiteness, unit descriptors, values."""
    B, _, H, W = imgs.shape
    C, div = DESC[name]
    assert tuple(score.shape) == (B, 1, H, W) and tuple(desc.shape) == (B, C, H // div, W // div), (tag, tuple(score.shape), tuple(desc.shape))
    assert score.dtype == desc.dtype == torch.float32
    assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(desc).all()), tag + ": non-finite output"
    t0 = time.perf_counter()
    o32, o64 = oracle(name, imgs), oracle(name, imgs, double=True)
    print("%s: both chains on the CPU took %.2f s" % (tag, time.perf_counter() - t0))
    assert all(np.isfinite(m).all() for m in o32[:2] + o64[:2]), tag + ": the oracle itself is not finite here"
    s, d = score[:, 0].cpu().numpy(), desc.contiguous().cpu().numpy()
    for i in range(B):
        ti = tag if B == 1 else "%s image %d of %d" % (tag, i, B)
        a32, a64 = [None if m is None else m[i] for m in o32], [None if m is None else m[i] for m in o64]
        if name == "r2d2":
            _check_r2d2(ti, s[i], d[i], a32, a64)
        else:
            _check_ratio(name, ti, s[i], d[i], a32, a64)


def _sweep(name, shape):
    imgs = sweep_image(*shape)
    score, desc = _net(name)(torch.from_numpy(imgs).to(DEV))
    _check_images(name, imgs, score, desc, "%s %dx%d" % ((name,) + shape))


@pytest.mark.parametrize("shape", SHAPES["r2d2"], ids=sid)
def test_r2d2_shape_sweep_against_oracle(shape):
    """1 x 1: one pixel, one row of one wave in every layer.  7 x 200 / 130 x 6: strips no wider than conv8's reach of 8 -- no tap of conv8 is inside at any pixel,
    the maps are constant; 1400 rows are ten gemm_h workgroups of 128 and 120 rows, 780 six and 12.  9 x 9: conv8 has a tap inside at the four corner pixels only,
    conv5's 8-row tile and halo of 8 cover the map once and a row.  15 x 17, 16 x 16, 17 x 33: just around 16, the full width of conv8's taps and one 16 x 16 tile
    of conv3 / conv4; 17 rows are three dil-4 tiles.  33 x 129: 4257 rows, one column past eight tiles.  136 x 200: mid-size, both sides off the tiles."""
    _sweep("r2d2", shape)


@pytest.mark.parametrize("shape", SHAPES["sfd2"], ids=sid)
def test_sfd2_shape_sweep_against_oracle(shape):
    """8 x 136 / 200 x 8: strips one cell thick -- the 1/4 map is two rows or columns, sfd2_score's x 4 bilinear clamps both taps of one direction, the stride-2
    8-row tiles hold 4, 2 and 1 rows.  24 x 8: one cell wide, three high.  8 x 264: 66 columns at 1/4, five grouped-conv tiles across (sfd2_gconv_h: 16 x 16).
    136 x 24: 34 rows at 1/4, three tiles down.  24 x 40: odd cell counts.  120 x 160: odd one way.  264 x 328: mid-size, 66 x 82 at 1/4 and 33 x 41 cells: odd,
    no multiple of a tile, five by six grouped-conv tiles."""
    _sweep("sfd2", shape)


@pytest.mark.parametrize("shape", SHAPES["d2net"], ids=sid)
def test_d2net_shape_sweep_against_oracle(shape):
    """8 x 136 / 200 x 8: one cell thick -- d2_upsample's scale is 0 in ONE direction only (at 8 x 8 both are), conv1_2 / conv2_2 / conv3_3 pool maps of 8, 4 and 2
    rows out of 16-row tiles, six of a 3 x 3 window's nine values are the ones-padding.  24 x 8: one cell wide.  8 x 16: two cells.  136 x 24: 17 cell rows, one past
    a 16-row head tile.  24 x 40: odd cell counts.  120 x 160: 15 x 20 cells.  264 x 328: 33 x 41 cells -- three 16-wide head tiles both ways."""
    _sweep("d2net", shape)


@pytest.mark.parametrize("name,B,shape", [(n, b, s) for n in ("r2d2", "sfd2", "d2net") for b, s in BATCHES[n]], ids=sid)
def test_a_batch_of_different_images_equals_the_oracle_and_the_single_images(name, B, shape):
    """Every image of the batch against the oracle, and images 0, B // 2, B - 1 against the net run on that image alone, BIT FOR BIT: launch_mfma has no
    batch-size branch (the batch is blockIdx.z / nblk), sfd2_gconv_h folds it as blockIdx.z >> 3 and scales by its tile's own maximum, gemm_h by its wave's rows
    (one image's: a wave never spans two images, rows are counted per image), D2-Net's maximum and sum are per image in a fixed order."""
    imgs = batch_images(B, *shape)
    net = _net(name)
    sb, db = net(torch.from_numpy(imgs).to(DEV))
    _check_images(name, imgs, sb, db, "%s %dx%d" % ((name,) + shape))
    for i in (0, B // 2, B - 1):
        s1, d1 = net(torch.from_numpy(imgs[i:i + 1]).to(DEV))
        assert torch.equal(s1[0], sb[i]), "%s: score of image %d of %d differs from the single-image run (max %.3g)" % (name, i, B, float((s1[0] - sb[i]).abs().max()))
        assert torch.equal(d1[0], db[i]), "%s: descriptors of image %d of %d differ from the single-image run (max %.3g)" % (name, i, B, float((d1[0] - db[i]).abs().max()))
    assert not torch.equal(sb[0], sb[B - 1])        # (different images)


@pytest.mark.parametrize("name,B,H,W,good", [
    ("r2d2", 1, 32768, 8, (9, 9)), ("r2d2", 1, 8, 32768, (16, 16)), ("r2d2", 1, 32768, 32769, (15, 17)),
    ("sfd2", 1, 16392, 8, (24, 8)), ("sfd2", 1, 8, 16392, (8, 136)), ("sfd2", 8192, 24, 40, (24, 40)),
    ("d2net", 1, 16392, 8, (24, 8)), ("d2net", 1, 8, 16392, (8, 16)), ("d2net", 8192, 24, 40, (24, 40))], ids=sid)
def test_an_image_or_batch_past_the_size_limit_is_refused_before_any_launch(name, B, H, W, good):
    """KPB_E_INVALID with the documented message, outputs at their sentinel, and the same net then runs a sweep shape.  The limits are checked in front of kpb_carve
    and of every launch (R2d2Net / Sfd2Net / D2Net::forward: the first statements), so nothing is read through the image pointer and nothing of the caller's is
    written: one small image stands in for the large one.  R2D2 packs pixel coordinates as y << 16 | x (H, W <= 32767); a product above 2^30 needs a side above
    that, so the third case trips both conditions.  SFD2 and D2-Net take sides up to 16384 and batches up to 8191 (the grouped layer's blockIdx.z is batch x 8)."""
    from keypoint_bench_amd._lib import ptr
    net = _net(name)
    x = torch.from_numpy(image(5, 24, 40))[None].to(DEV)
    net._ensure(x.device)
    score, desc = torch.full((4096,), -7.0, device=DEV), torch.full((4096,), -7.0, device=DEV)
    rc = net._ctx.lib.kpb_net_forward(net._handle, ptr(x), B, H, W, ptr(score), ptr(desc))
    msg = net._ctx.lib.kpb_last_error(net._ctx.handle).decode()
    net._ctx.sync()
    torch.cuda.synchronize()
    want = "kpb_net_forward: %s image %dx%d%s too large" % (NAME[name], H, W, "" if name == "r2d2" else " x %d" % B)
    assert rc == KPB_E_INVALID and msg == want, (rc, msg, want)
    assert bool((score == -7.0).all()) and bool((desc == -7.0).all())
    _sweep(name, good)


@pytest.mark.timeout(600)
def test_strict_fp32_kernels_pass_both_sweeps():
    """KPB_FP32_MATRIX is read once per process: the shape and batch sweeps again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    tests = ["test_r2d2_shape_sweep_against_oracle", "test_sfd2_shape_sweep_against_oracle", "test_d2net_shape_sweep_against_oracle",
             "test_a_batch_of_different_images_equals_the_oracle_and_the_single_images"]
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"] + ["tests/test_gpu_layer_net_shapes.py::" + t for t in tests]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=500)
    out = p.stdout
    print("\n".join(l for l in out.splitlines() if " fp32 " in l or "passed" in l or "failed" in l))
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % "\n".join(out.splitlines()[-40:])
    n = sum(len(SHAPES[k]) + len(BATCHES[k]) for k in SHAPES)
    last = out.splitlines()[-1]
    assert "%d passed" % n in last and "skipped" not in last and "failed" not in last, last
    assert " fp32 score: " in out and " split-f16 " not in out          # every comparison of the child ran under the knob
