"""Every image shape and batch kpb_net_forward accepts for SuperPoint, DISK and XFeat, not only the multiples of 32 the other files run.

The three nets share conv_mfma_h / gemm_h / conv_valu_t (csrc/conv_mfma.h, launched by csrc/conv_layer.hip and csrc/convnet.hip) and accept H, W multiples of 8 (SuperPoint), 16 (DISK) and 32
(XFeat).  Heights that are not multiples of 16 end in half a workgroup tile (the generated-input form of SuperPoint's conv1b must treat the rows below the image
as conv1b's zero padding, not as relu(bias) of conv1a); DISK's lower levels are smaller than one 16 x 16 tile and its fused upsampling then stages a clamped
source tile that covers the whole source; XFeat at 32 x 32 has one pixel at 1/32 and fewer rows than a gemm_h workgroup.  Each test compares the FULL maps with
the torch-fp32 oracle restatements (oracle/*_ref.py) on the seeded weights of the per-net files, at their tolerances:

  shape sweep   SuperPoint (8,8) (8,136) (200,8) (40,24) (72,104) (120,160) (264,328);  DISK (16,32) (32,16) (16,272) (112,16) (48,80) (80,96) (208,336);
                XFeat (32,32) (32,288) (96,32) (160,224) (352,288): the smallest shape, a one-tile-high and a one-tile-wide strip whose long side is not a
                multiple of 128, odd multiples of the granularity both ways, an odd multiple one way and a multiple of 32 the other, one mid-size shape.
                The oracles are finite at every one of them (checked on the CPU before the first GPU run).
  batch sweep   B different images (different seeds, alternating views): 3 and 5 at an odd-multiple shape, 17 (DISK: 9) at 64 x 96; every image against the
                oracle, images 0, B // 2 and B - 1 against the same net run on that image alone.
  rejections    shapes off the granularity, DISK's 16 x 16 (a 1 x 1 bottleneck: the reference's InstanceNorm2d raises "Expected more than 1 spatial element" there,
                on nn.InstanceNorm2d in eval mode and on F.instance_norm alike, so the library refuses it), batch 0 and H = 0: KPB_E_INVALID, nothing written, net usable.

Tolerances: the per-net files' bounds (set at 480 x 640).  On maps of a few pixels an InstanceNorm or a one-cell softmax can be badly conditioned, so a comparison
that misses its bound BY MAGNITUDE is settled against the same oracle in float64: e_ref = max |oracle_fp32 - oracle_fp64| is the reference arithmetic's own error at
that shape, and the GPU passes if max |gpu - oracle_fp64| <= 4 e_ref (4: a summation order over K up to 2304 other than oneDNN's; a margin over the reference's
error, never over the GPU's).  The float64 oracle runs inside the test, no number is hard-coded.  Measured on an MI355X (split-f16 form and KPB_FP32_MATRIX=1):
no shape of either sweep needed the float64 rule -- every comparison holds its file's usual bound, so there is no (e_ref, error) pair to record.  The badly conditioned
case shows, inside the bound: DISK 16 x 32 (the instance statistics of a 1 x 2 bottleneck) is 5.9e-6 off the oracle's score against 1.0-1.6e-6 at every other shape
(bound 2e-5; strict fp32: 2.9e-6), its descriptors 5.9e-6 against 0.7-1.0e-6 (bound 1e-4); the oracle's own fp32 error at that shape is about 8e-7 / 5e-7.
The whole file runs in about 5 s (4.4 s of tests)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KPB_E_INVALID = -1

SHAPES = {
    "superpoint": [(8, 8), (8, 136), (200, 8), (40, 24), (72, 104), (120, 160), (264, 328)],
    "disk": [(16, 32), (32, 16), (16, 272), (112, 16), (48, 80), (80, 96), (208, 336)],
    "xfeat": [(32, 32), (32, 288), (96, 32), (160, 224), (352, 288)],
}
# (batch, shape): an odd-multiple shape of the sweep at 3 and 5 images, 64 x 96 at a batch that spreads over many workgroups
BATCHES = {
    "superpoint": [(3, (72, 104)), (5, (72, 104)), (17, (64, 96))],
    "disk": [(3, (48, 80)), (5, (48, 80)), (9, (64, 96))],
    "xfeat": [(3, (160, 224)), (5, (160, 224)), (17, (64, 96))],
}
# tests/test_gpu_superpoint.py, test_gpu_disk.py, test_gpu_xfeat.py, test_gpu_alike.py: (rtol, atol) of the score / heat-map, atol of the descriptors
TOL = {"superpoint": ((2e-3, 1e-6), 1e-4), "disk": ((0.0, 2e-5), 1e-4), "xfeat": ((2e-3, 1e-7), 1e-4), "alike": ((0.0, 7e-6), 1e-4)}
DESC = {"superpoint": (256, 8), "disk": (128, 1), "xfeat": (64, 8), "alike": (64, 1)}       # channels, H / div x W / div


@functools.lru_cache(maxsize=None)
def _net(name):
    """One net object per architecture for the whole file: it goes through every shape in turn, as a caller's would."""
    if name == "superpoint":
        from keypoint_bench_amd.models.SuperPoint import superpoint_random
        return superpoint_random(7).eval()
    if name == "disk":
        from keypoint_bench_amd.models.disk import disk_random
        return disk_random(5).eval()
    if name == "xfeat":
        from keypoint_bench_amd.models.XFeat import xfeat_random
        return xfeat_random(9).eval()
    from keypoint_bench_amd.models.ALike import alike_t
    return alike_t().eval()


@functools.lru_cache(maxsize=None)
def _tensors(name, double):
    if name == "superpoint":
        t = weights.random_superpoint(7)
    elif name == "disk":
        t = weights.tensors_disk(weights.random_disk_state_dict(5))
    elif name == "xfeat":
        t = weights.fold_xfeat(weights.random_xfeat_state_dict(9))
    else:
        t = weights.load_alike_t()
    return {k: torch.from_numpy(np.asarray(v)).double() if double else torch.from_numpy(np.asarray(v)) for k, v in t.items()}


def _oracle(name, img, double=False):
    """(score, desc) of one image [3,H,W] from the plain torch restatement, in fp32 or with image and weights cast to float64."""
    from oracle import alike_ref, disk_ref, superpoint_ref, xfeat_ref
    fwd = {"superpoint": superpoint_ref.superpoint_forward, "disk": disk_ref.disk_forward, "xfeat": xfeat_ref.xfeat_forward, "alike": alike_ref.alnet_forward}[name]
    x = torch.from_numpy(img)[None]
    with torch.no_grad():
        s, d = fwd(x.double() if double else x, _tensors(name, double))
    return s[0].numpy(), d[0].numpy()


def _image(seed, H, W, view=0):
    return synthetic.image_pair(seed, max(H, 64), max(W, 64))[view][:, :H, :W].copy()


def _close(what, got, ref32, ref64, rtol, atol):
    """The file's usual bound, or -- where that is missed by magnitude -- the float64 rule of the module docstring.  Prints its figures before it asserts."""
    err32 = float(np.abs(got - ref32).max())
    usual = bool(np.all(np.abs(got - ref32) <= atol + rtol * np.abs(ref32)))
    print("%s: max |gpu - oracle_fp32| = %.3g (rtol %g, atol %g: %s)" % (what, err32, rtol, atol, "holds" if usual else "MISSED"))
    if usual:
        return
    r64 = ref64()
    e_ref, err64 = float(np.abs(ref32.astype(np.float64) - r64).max()), float(np.abs(got.astype(np.float64) - r64).max())
    print("%s: float64 rule: e_ref = %.3g, max |gpu - oracle_fp64| = %.3g, 4 e_ref = %.3g" % (what, e_ref, err64, 4 * e_ref))
    assert err64 <= 4 * e_ref, "%s: beyond %g / %g of the fp32 oracle (max %.3g) and beyond 4 x the oracle's own fp32 error (%.3g > 4 x %.3g)" % (
        what, rtol, atol, err32, err64, e_ref)


def _check_image(name, img, score, desc, tag):
    """score [1,H,W] and desc [C,H/div,W/div] of one image (GPU tensors) against the oracle: shapes, finiteness, unit descriptors, values."""
    H, W = img.shape[1:]
    C, div = DESC[name]
    assert tuple(score.shape) == (1, H, W) and tuple(desc.shape) == (C, H // div, W // div), (tag, tuple(score.shape), tuple(desc.shape))
    assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(desc).all()), tag + ": non-finite output"
    if name in ("superpoint", "disk"):
        np.testing.assert_allclose(torch.linalg.norm(desc, dim=0).cpu().numpy(), 1.0, rtol=0, atol=1e-5, err_msg=tag + ": descriptors are not unit vectors")
    so, do = _oracle(name, img)
    assert np.isfinite(so).all() and np.isfinite(do).all(), tag + ": the oracle itself is not finite here"
    ref64 = functools.lru_cache(maxsize=None)(lambda: _oracle(name, img, double=True))
    (rtol, atol), atol_desc = TOL[name]
    _close(tag + " score", score.cpu().numpy(), so, lambda: ref64()[0], rtol, atol)
    _close(tag + " desc", desc.cpu().numpy(), do, lambda: ref64()[1], 0.0, atol_desc)


def _sweep(name, shape):
    H, W = shape
    img = _image(40 + H + W, H, W)
    score, desc = _net(name)(torch.from_numpy(img)[None].to(DEV))
    assert score.shape[0] == 1 and desc.shape[0] == 1
    _check_image(name, img, score[0], desc[0], "%s %dx%d" % (name, H, W))


@pytest.mark.parametrize("shape", SHAPES["superpoint"], ids=lambda s: "%dx%d" % s)
def test_superpoint_shape_sweep_against_oracle(shape):
    """8 x 8 is one cell (every convolution a single partial tile, a softmax and a pixel shuffle over one cell); 8 x 136 / 200 x 8 are strips one cell thick;
    40 x 24, 72 x 104 are odd multiples of 8 both ways (72 x 104 -> 36 x 52 -> 18 x 26 -> 9 x 13: 4.5 row tiles in conv1b, odd maps below); 120 x 160 is odd one
    way; 264 x 328 is mid-size and no multiple of 16."""
    _sweep("superpoint", shape)


@pytest.mark.parametrize("shape", SHAPES["disk"], ids=lambda s: "%dx%d" % s)
def test_disk_shape_sweep_against_oracle(shape):
    """16 x 32 / 32 x 16 have a 1 x 2 / 2 x 1 bottleneck (the instance statistics of two pixels); 16 x 272 / 112 x 16 are strips with a 1 x 17 / 7 x 1 bottleneck;
    48 x 80 (3 x 5 at the bottom) has three levels smaller than one 16 x 16 tile; 80 x 96 is odd one way; 208 x 336 mid-size, no multiple of 32."""
    _sweep("disk", shape)


@pytest.mark.parametrize("shape", SHAPES["xfeat"], ids=lambda s: "%dx%d" % s)
def test_xfeat_shape_sweep_against_oracle(shape):
    """32 x 32: one pixel at 1/32, 16 cells for gemm_h's 128-row workgroups and the in-place unfolded read of keypoint_head.0; 32 x 288 / 96 x 32 strips; 160 x 224 odd
    multiples of 32 both ways; 352 x 288 mid-size (XFeat accepts multiples of 32 only)."""
    _sweep("xfeat", shape)


@pytest.mark.parametrize("name,B,shape", [(n, b, s) for n in ("superpoint", "disk", "xfeat") for b, s in BATCHES[n]],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_a_batch_of_different_images_equals_the_oracle_and_the_single_images(name, B, shape):
    """Every image of the batch against the oracle, and images 0, B // 2, B - 1 against the net run on that image alone -- BIT FOR BIT, for all three nets.
    The launch plans choose their forms and tiles from the layer and from H, W only (launch_mfma of csrc/conv_layer.hip / launch_valu of csrc/convnet.hip have no batch-size branch; the
    batch is blockIdx.z / nblk or a grid dimension of its own), and everything per image is reduced per image in a fixed order: SuperPoint's pre_amax
    (plane_abs_max: one workgroup per image), XFeat's (mean, 1 / std) (gray_mean_stats: XF_STAT_BLOCKS partials per image, folded in block order), DISK's
    statistics and xf tables (chan_sums / up_chan_sums: SUM_BLOCKS partials per image, folded in block order by make_xf), gemm_h's per-wave operand scale (a
    wave's rows belong to one image).  So the arithmetic per output does not depend on the batch, and torch.equal replaces the atol 2e-6 / rtol 1e-5 of
    test_disk_full_size_and_batch / test_xfeat_full_size_batch_and_oracle (SuperPoint's test asserts torch.equal already)."""
    H, W = shape
    imgs = np.stack([_image(300 + 10 * B + i, H, W, view=i & 1) for i in range(B)])
    net = _net(name)
    sb, db = net(torch.from_numpy(imgs).to(DEV))
    assert sb.shape[0] == B and db.shape[0] == B
    for i in range(B):
        _check_image(name, imgs[i], sb[i], db[i], "%s %dx%d image %d of %d" % (name, H, W, i, B))
    for i in (0, B // 2, B - 1):
        s1, d1 = net(torch.from_numpy(imgs[i:i + 1]).to(DEV))
        assert torch.equal(s1[0], sb[i]), "%s: score of image %d of %d differs from the single-image run (max %.3g)" % (name, i, B, float((s1[0] - sb[i]).abs().max()))
        assert torch.equal(d1[0], db[i]), "%s: descriptors of image %d of %d differ from the single-image run (max %.3g)" % (name, i, B, float((d1[0] - db[i]).abs().max()))


def _raw_forward(name, x, B, H, W):
    """kpb_net_forward through ctypes on outputs filled with a sentinel: (return code, message, whether the outputs are untouched)."""
    from keypoint_bench_amd._lib import ptr
    net = _net(name)
    net._ensure(x.device)
    C, div = DESC[name]
    Hd, Wd = max(H, 8) // div, max(W, 8) // div
    score = torch.full((max(B, 1), 1, max(H, 8), max(W, 8)), -7.0, dtype=torch.float32, device=x.device)
    desc = torch.full((max(B, 1), Hd, Wd, C), -7.0, dtype=torch.float32, device=x.device)
    rc = net._ctx.lib.kpb_net_forward(net._handle, ptr(x), B, H, W, ptr(score), ptr(desc))
    msg = net._ctx.lib.kpb_last_error(net._ctx.handle).decode()
    net._ctx.sync()
    torch.cuda.synchronize()
    return rc, msg, bool((score == -7.0).all()) and bool((desc == -7.0).all())


@pytest.mark.parametrize("name,bad,gran,good", [
    ("superpoint", (36, 52), 8, (40, 24)), ("superpoint", (64, 100), 8, (72, 104)), ("disk", (24, 40), 16, (48, 80)), ("disk", (64, 104), 16, (16, 32)),
    ("xfeat", (48, 64), 32, (32, 32)), ("alike", (48, 64), 32, (64, 96))], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_a_shape_off_the_granularity_is_refused_and_the_net_stays_usable(name, bad, gran, good):
    """KPB_E_INVALID with the documented message, through the Python model and through the C ABI; nothing is launched (the outputs keep their sentinel); the same
    net object then runs an accepted shape and matches the oracle."""
    from keypoint_bench_amd._lib import KpbError
    net = _net(name)
    H, W = bad
    x = torch.from_numpy(_image(5, H, W))[None].to(DEV)
    with pytest.raises(KpbError, match=r"needs H and W multiples of %d \(got %dx%d\)" % (gran, H, W)) as e:
        net(x)
    assert e.value.code == KPB_E_INVALID
    rc, msg, untouched = _raw_forward(name, x, 1, H, W)
    assert rc == KPB_E_INVALID and "needs H and W multiples of %d" % gran in msg and untouched, (rc, msg, untouched)
    _sweep(name, good)


def test_disk_refuses_the_16x16_image_whose_bottleneck_is_one_pixel():
    """The reference cannot run it: nn.InstanceNorm2d / F.instance_norm raise "Expected more than 1 spatial element" on the 64 x 1 x 1 map in front of down_4 (the
    oracle restatement raises the same error, asserted here).  The library names the 1x1 bottleneck, launches nothing, and runs 16 x 32 afterwards."""
    from keypoint_bench_amd._lib import KpbError
    img = _image(6, 16, 16)
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        _oracle("disk", img)
    net = _net("disk")
    x = torch.from_numpy(img)[None].to(DEV)
    with pytest.raises(KpbError, match="1x1 bottleneck") as e:
        net(x)
    assert e.value.code == KPB_E_INVALID
    rc, msg, untouched = _raw_forward("disk", x, 1, 16, 16)
    assert rc == KPB_E_INVALID and "1x1 bottleneck" in msg and untouched, (rc, msg, untouched)
    x3 = torch.from_numpy(np.stack([img] * 3)).to(DEV)          # refused at every batch size: each image has its own statistics
    rc, msg, untouched = _raw_forward("disk", x3, 3, 16, 16)
    assert rc == KPB_E_INVALID and "1x1 bottleneck" in msg and untouched, (rc, msg, untouched)
    _sweep("disk", (16, 32))


@pytest.mark.parametrize("name", ["superpoint", "disk", "xfeat", "alike"])
def test_an_empty_batch_or_image_is_refused_before_any_launch(name):
    """kpb_net_forward with batch 0, H = 0, W = 0 or a negative batch: KPB_E_INVALID ("bad argument", csrc/net_api.hip), outputs untouched, net usable."""
    net = _net(name)
    x = torch.from_numpy(_image(8, 64, 96))[None].to(DEV)
    for B, H, W in ((0, 64, 96), (1, 0, 96), (1, 64, 0), (-1, 64, 96)):
        rc, msg, untouched = _raw_forward(name, x, B, H, W)
        assert rc == KPB_E_INVALID and "kpb_net_forward: bad argument" in msg and untouched, (B, H, W, rc, msg, untouched)
    null = ctypes.c_void_p(0)
    net._ensure(x.device)
    assert net._ctx.lib.kpb_net_forward(net._handle, null, 1, 64, 96, null, null) == KPB_E_INVALID
    _sweep(name, (64, 96))
