"""KPB_OPT_ALIKE_COARSE_FUSED: from 16 images on, conv2 of ALIKE's blocks 3 and 4 finishes the block in its epilogue (CmForm::tail in
csrc/conv_mfma.h: aggregation, score and head shares and block 3's max-pool from the output tile in LDS; x3 / x4 never written, four launches
instead of seven).  Nothing in it reorders arithmetic, so option 1 (the default) and option 0 (the separate kernels) must give the SAME BITS:
the score map, the dense descriptor map, and the descriptors alike_desc_at reads from a3 / a4 in the keypoint-only mode.

Shapes: the smallest at which the tiling can go wrong -- 32 x 32 (a 4 x 4 map: one partial tile; block 4 a single pixel), 96 x 160 (12 x 20:
partial tiles in both directions, two tile rows; block 4's 3 x 5 map smaller than one tile), 64 x 96 (8 x 12: a partial tile in x only).
Batches 16 and 17: the first that take the batch path, one of them odd; every slot its own seeded image."""

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic
from keypoint_bench_amd._lib import Context, KpbError, ptr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(32, 32), (96, 160), (64, 96)]
NPTS = 50
KPB_E_INVALID = -1


@pytest.fixture(scope="module")
def nets():
    from keypoint_bench_amd.models.ALike import alike_t
    out = {}
    for dense in (True, False):
        net = alike_t(dense_descriptors=dense).eval()
        net._ensure(DEV)
        out[dense] = net
    yield out
    Context.get(DEV).set_option(Context.OPT_ALIKE_COARSE_FUSED, 1)


@pytest.fixture(scope="module")
def images():
    """17 seeded images per shape, computed once; a batch of 16 is the first 16 of them."""
    return {(H, W): torch.from_numpy(np.stack([synthetic.image_pair(300 + 7 * H + i, H, W)[i & 1] for i in range(17)])).to(DEV) for H, W in SHAPES}


def _forward(net, imgs, option, pts=None):
    """One forward with KPB_OPT_ALIKE_COARSE_FUSED = option, on the shared context: (score, dense map or the rows of alike_desc_at at pts)."""
    ctx = Context.get(DEV)
    ctx.set_option(Context.OPT_ALIKE_COARSE_FUSED, option)
    B, _, H, W = imgs.shape
    score = torch.full((B, 1, H, W), float("nan"), device=DEV)
    if net.dense_descriptors:
        out = torch.full((B, H, W, 64), float("nan"), device=DEV)
        ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(imgs), B, H, W, ptr(score), ptr(out)))
    else:
        out = torch.full((B, NPTS, 64), float("nan"), device=DEV)
        n = torch.full((B,), NPTS, dtype=torch.int32, device=DEV)
        ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(imgs), B, H, W, ptr(score), ptr(None)))
        ctx.check(ctx.lib.kpb_net_desc_at(net._handle, ptr(pts), 2, NPTS, ptr(n), ptr(out)))
    ctx.sync()
    return score, out


def _points(B, seed):
    return torch.from_numpy(np.random.default_rng(seed).random((B, NPTS, 2)).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "keypoint-only"])
@pytest.mark.parametrize("batch", [16, 17])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_fused_tail_gives_the_bits_of_the_separate_kernels(nets, images, shape, batch, dense):
    net, imgs = nets[dense], images[shape][:batch].contiguous()
    pts = None if dense else _points(batch, 1000 * batch + shape[0])
    s1, d1 = _forward(net, imgs, 1, pts)
    s0, d0 = _forward(net, imgs, 0, pts)
    assert torch.isfinite(s1).all() and torch.isfinite(d1).all() and torch.isfinite(s0).all() and torch.isfinite(d0).all()
    assert torch.equal(s1, s0), "score maps differ: max |d| = %g" % (s1 - s0).abs().max().item()
    assert torch.equal(d1, d0), "descriptors differ: max |d| = %g" % (d1 - d0).abs().max().item()


def test_the_fused_tail_is_deterministic(nets, images):
    imgs = images[(96, 160)]
    sa, da = _forward(nets[True], imgs, 1)
    sb, db = _forward(nets[True], imgs, 1)
    assert torch.equal(sa, sb) and torch.equal(da, db)


@pytest.mark.parametrize("bad", [2, -1])
def test_an_unknown_value_is_refused_and_leaves_the_net_usable(nets, images, bad):
    ctx = Context.get(DEV)
    imgs = images[(64, 96)][:16].contiguous()
    want = _forward(nets[True], imgs, 1)
    assert ctx.lib.kpb_ctx_set_option(ctx.handle, Context.OPT_ALIKE_COARSE_FUSED, bad) == KPB_E_INVALID
    with pytest.raises(KpbError):
        ctx.set_option(Context.OPT_ALIKE_COARSE_FUSED, bad)
    B, _, H, W = imgs.shape
    score, desc = torch.empty((B, 1, H, W), device=DEV), torch.empty((B, H, W, 64), device=DEV)
    ctx.check(ctx.lib.kpb_net_forward(nets[True]._handle, ptr(imgs), B, H, W, ptr(score), ptr(desc)))      # the option stayed at 1
    ctx.sync()
    assert torch.equal(score, want[0]) and torch.equal(desc, want[1])
