"""GPU checks of N13 (Harris: csrc/harris.hip through the C ABI).  The response is defined as the correctly rounded value of the formula cv2.cornerHarris
approximates, every step before its last line an integer, so the device must equal the numpy oracle of tests/harris_fixtures.py
BIT FOR BIT: at the smallest accepted shape, below and around one 32 x 64 tile, across several tiles and at 480 x 640, on maps whose gray cast wraps, on
maps where nothing wraps, on a constant image (exactly +0.0 everywhere), on the byte ramp, on negative sums and on an image of squares whose response is half negative; alone and in a batch; then detection on the
device's map against the signed-detection oracle on the oracle's map (identical keypoints: nothing is left out, the maps are bit-equal), the refusals at
the ABI, and the pipelines and the runner against the single-pair path."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from keypoint_bench_amd import synthetic, weights
from keypoint_bench_amd._lib import Context, KpbError, c_void_p, ptr
from harris_fixtures import BLOCK_SIZES, CONFIG_PLAN, KINDS, KS, LARGE, SMALL, harris_oracle, image, stripes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KPB_E_INVALID, KPB_E_WEIGHTS, KPB_E_UNSUPPORTED = -1, -6, -7
PARAMS = dict(block_size=CONFIG_PLAN[0], ksize=CONFIG_PLAN[1], k=CONFIG_PLAN[2])
EP = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
BF = dict(metric="euclidean", max_distance=float("inf"), cross_check=True)
OF = dict(distance=0, win_size=7, levels=2, interation=20, gray=False)      # distance 0: the tracker's drawn start angles cannot matter


def _net(**kw):
    from keypoint_bench_amd.models.Harris import Harris
    return Harris(dict(PARAMS, **kw)).eval()


@pytest.fixture(scope="module")
def net():
    return _net()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _homo(hm, H, W):
    return dict(mode="homo", homography_matrix=hm, width=np.int64(W), height=np.int64(H))


def _check(n, img, b, k, what):
    score, none = n(_t(img)[None])
    H, W = img.shape[1:]
    assert none is None and score.shape == (1, 1, H, W) and score.dtype == torch.float32 and score.device == torch.device(DEV)
    got, want = score[0, 0].cpu().numpy(), harris_oracle(img, b, k)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d of %d pixels differ, first at %s: device %r, oracle %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])
    return got


# ------------------------------------------------------------------------------------------------ 1. bit equality with the oracle
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SMALL)
def test_harris_equals_the_oracle_bit_for_bit(net, H, W, kind):
    got = _check(net, image(kind, H, W, seed=H), CONFIG_PLAN[0], CONFIG_PLAN[2], "%s %dx%d" % (kind, H, W))
    if kind == "constant":
        assert not _bits(got).any()                 # exactly +0.0: no sign bit either
    else:
        assert _bits(got).any()
        if kind == "blocks" and H >= 31:
            assert (got < 0).mean() > 0.2 and (got > 0).mean() > 0.2       # a signed response: edges below zero, corners above


@pytest.mark.parametrize("b", BLOCK_SIZES)
@pytest.mark.parametrize("k", KS)
def test_every_block_size_and_k_at_an_odd_shape(b, k):
    H, W = 37, 61
    n = _net(block_size=b, k=k)
    for kind in ("frames", "thirds"):
        _check(n, image(kind, H, W, seed=b), b, k, "%s block_size %d k %g" % (kind, b, k))
    if b == 6:      # the largest integer terms there are: A (C) at its bound b^2 1 040 400
        for tr in (False, True):
            _check(n, stripes(H, W, transpose=tr), b, k, "stripes transposed %d" % tr)


def test_harris_at_480x640(net):
    _check(net, image("frames", *LARGE, seed=0), CONFIG_PLAN[0], CONFIG_PLAN[2], "frames 480x640")


# ------------------------------------------------------------------------------------------------ 2. batch equals solo
def test_harris_batch_equals_solo_bit_for_bit_and_a_map_pointer_is_not_written_through(net):
    H, W = 37, 61
    imgs = np.stack([image("frames", H, W, seed=500 + i) for i in range(3)])
    x = _t(imgs)
    s, d = net._run(x, want_desc=False)         # desc_out_dev = NULL
    s = s.clone()
    assert d is None and net.dim == 0 and net.desc_div == 1
    for i in range(3):                          # alone, and against the oracle: a pixel's bits depend on neither tile nor batch nor position
        si, _ = net._run(x[i:i + 1].contiguous(), want_desc=False)
        assert torch.equal(si[0], s[i])
        assert np.array_equal(_bits(s[i, 0].cpu().numpy()), _bits(harris_oracle(imgs[i], CONFIG_PLAN[0], CONFIG_PLAN[2])))
    assert not torch.equal(s[0], s[2])          # (different images)
    sentinel = torch.full((3, H, W, 8), 7.0, device=DEV)
    score = torch.empty((3, 1, H, W), device=DEV)
    ctx = net._ctx
    ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(x), 3, H, W, ptr(score), ptr(sentinel)))
    ctx.sync()
    assert torch.equal(score, s) and bool((sentinel == 7.0).all())
    assert ctx.lib.kpb_net_desc_dim(net._handle) == 0 and ctx.lib.kpb_net_desc_div(net._handle) == 1
    with pytest.raises(KpbError):               # no descriptor map, so nothing to sample inside the net either
        ctx.check(ctx.lib.kpb_net_desc_at(net._handle, ptr(torch.zeros((4, 2), device=DEV)), 2, 4, ptr(None), ptr(torch.zeros((4, 8), device=DEV))))


# ------------------------------------------------------------------------------------------------ 3. detection
@pytest.mark.parametrize("H,W", [(96, 160), LARGE])
@pytest.mark.parametrize("nms_dist", [4, 6])
@pytest.mark.parametrize("kind", ["frames", "blocks"])      # all corners (the wrapped noise), and half the map below zero
def test_signed_detection_on_the_device_map_equals_the_oracle_keypoints(net, H, W, nms_dist, kind):
    from keypoint_bench_amd.utils.extracter import detection
    img = image(kind, H, W, seed=7)
    prm = dict(nms_dist=nms_dist, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)      # the configs' extractor_params
    score, _ = net(_t(img)[None])
    got = detection(score, prm, signed=True).cpu().numpy()
    want, _ = oracle.detection(harris_oracle(img, CONFIG_PLAN[0], CONFIG_PLAN[2]), prm)
    print("harris detect %s %dx%d nms_dist %d: %d keypoints (oracle %d)" % (kind, H, W, nms_dist, got.shape[0], want.shape[0]))
    assert got.shape == want.shape and want.shape[0] > 50
    assert np.array_equal(_bits(got), _bits(np.ascontiguousarray(want, np.float32)))


# ------------------------------------------------------------------------------------------------ 4. refusals at the ABI
def _create(arch, tensors, blob_arch=None):
    ctx = Context.get(torch.device(DEV))
    blob = weights.pack(tensors, arch if blob_arch is None else blob_arch)
    h = c_void_p()
    rc = ctx.lib.kpb_net_create(ctx.handle, arch, blob, len(blob), ctypes.byref(h))
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    if h.value:
        ctx.lib.kpb_net_destroy(h)
    return rc, msg, bool(h.value)


def test_create_refuses_foreign_missing_misshaped_and_unsupported_plans(net):
    HA, K = weights.ARCH_HARRIS, weights.ARCH_KEYNET
    t = weights.harris_plan(PARAMS)
    plan = lambda *v: {"harris.plan": np.array(v, np.float32)}
    for arch, blob_arch in ((HA, K), (K, HA)):          # a wrong arch id over the blob
        rc, msg, made = _create(arch, t, blob_arch)
        assert rc == KPB_E_WEIGHTS and not made and msg, (arch, msg)
    rc, msg, made = _create(K, t)                       # the plan under another net's id and arch
    assert rc == KPB_E_WEIGHTS and not made and "KeyNet" in msg, msg
    for tensors in ({}, {"harris.plam": t["harris.plan"]}, plan(5, 3), plan(5, 3, 0.04, 0), {"harris.plan": np.zeros((1, 3), np.float32)}):
        rc, msg, made = _create(HA, tensors)
        assert rc == KPB_E_WEIGHTS and not made and "harris.plan" in msg, msg
    for tensors, word in ((plan(5, 5, 0.04), "ksize"), (plan(7, 3, 0.04), "block_size"), (plan(1, 3, 0.04), "block_size"), (plan(2.5, 3, 0.04), "block_size"),
                          (plan(5, 3, np.inf), "k"), (plan(5, 3, np.nan), "k")):
        rc, msg, made = _create(HA, tensors)
        assert rc == KPB_E_UNSUPPORTED and not made and "Harris" in msg and word in msg, msg
    rc, msg, made = _create(HA, t)                      # the intact one is created on the same context
    assert rc == 0 and made, msg


@pytest.mark.parametrize("H,W", [(7, 64), (64, 7)])
def test_a_shape_below_8_is_refused_and_the_net_stays_usable(net, H, W):
    x = _t(image("frames", 32, 64))[None]
    s = net._run(x, want_desc=False)[0].clone()
    bad = _t(np.full((1, 3, H, W), 0.25, np.float32))
    score = torch.full((1, 1, H, W), 7.0, device=DEV)
    ctx = net._ctx
    rc = ctx.lib.kpb_net_forward(net._handle, ptr(bad), 1, H, W, ptr(score), ptr(None))
    assert rc == KPB_E_INVALID
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    assert "Harris" in msg and "%dx%d" % (H, W) in msg, msg
    ctx.sync()
    assert bool((score == 7.0).all())           # nothing written
    with pytest.raises(KpbError):
        net(bad)
    assert torch.equal(net._run(x, want_desc=False)[0], s)


# ------------------------------------------------------------------------------------------------ 5. pipelines and runner
def _pair_items(n, H, W):
    ds = []
    for v0, v1, hm in [synthetic.warped_pair(1 + i, H, W, strength=1.0) for i in range(n)]:
        ds.append({"image0": v0, "image1": v1, "dataset": "HPatches", "warp01_params": _homo(hm, H, W),
                   "warp10_params": _homo(np.linalg.inv(hm).astype(np.float32), H, W)})
    return ds


def _config(task, **kw):
    return dict({"model_type": "Harris", "task_type": task, "Harris_params": dict(PARAMS), "extractor_params": EP,
                 "matcher_params": {"type": "optical_flow", "optical_flow_params": OF, "brute_force_params": BF}}, **kw)


def test_repeatability_batched_pipeline_equals_the_single_pair_path():
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.models.Harris import Harris
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    B, H, W = 3, 96, 160
    ds = _pair_items(B, H, W)
    images = _t(np.concatenate([np.stack([d["image0"] for d in ds]), np.stack([d["image1"] for d in ds])]))
    pipe = PairPipeline(_net(), EP, BF, B, H, W, device=DEV, match=False)
    assert pipe.desc is None and pipe.C == 0
    pipe.run(images)
    solo = _net()
    n = pipe.n.cpu().numpy()
    for j in range(2 * B):                      # every view: net(x), then detection(..., signed=True)
        want = detection(solo(images[j:j + 1])[0], EP, signed=True).cpu().numpy()
        assert n[j] == want.shape[0] > 20
        assert np.array_equal(_bits(pipe.kps[j, :n[j]].cpu().numpy()), _bits(want)), j
    prm = _config("repeatability", repeatability_params={"th": 3})
    rows = np.array(runner._batched_repeatability(pipe, ds, prm), np.float64)
    single = runner.PairRunner(prm, device=DEV, batch=1)
    assert isinstance(single.model, Harris) and single.model.dim == 0 and single.model.signed_scores
    _, rows1 = single.run(ds)
    assert single.batched_pairs == 0
    batched = runner.PairRunner(prm, device=DEV, batch=4)
    agg, rowsb = batched.run(ds)
    assert batched.batched_pairs == B
    assert np.array_equal(_bits(rows1), _bits(rowsb)), (rows1[:, :3], rowsb[:, :3])
    assert np.array_equal(_bits(rows1[:, :3]), _bits(rows[:, :3])), (rows1[:, :3], rows)
    print("harris repeatability rows [num_feat, repeatability, mean_error]: %s" % rowsb[:, :3].tolist())
    assert rowsb[:, 0].min() > 20 and np.isfinite(agg["repeatability"])


def test_runner_tracks_harris_keypoints_on_the_frames_batched_equal_single():
    from keypoint_bench_amd import runner
    H, W = 96, 160
    rng = np.random.default_rng(9)
    frames = [synthetic.image_pair(40, H, W)[0], synthetic.image_pair(40, H, W)[1], synthetic.image_pair(41, H, W)[0]]
    seq = [{"image0": fr.copy(), "fundamental": torch.from_numpy(rng.normal(size=(3, 3)).astype(np.float32)), "dataset": "TartanAir"} for fr in frames]
    prm = _config("FundamentalMatrix", FundamentalMatrix_params={"th": 3.0})
    single = runner.PairRunner(prm, device=DEV, batch=1)
    _, rows1 = single.run(seq)
    assert single.batched_pairs == 0 and rows1.shape[0] == 3
    batched = runner.PairRunner(prm, device=DEV, batch=4)
    _, rowsb = batched.run(seq)
    assert batched.batched_pairs == 3
    assert np.array_equal(_bits(rows1), _bits(rowsb)), (rows1[:, :3], rowsb[:, :3])
    assert rowsb[:, 2].min() >= 0 and np.isfinite(rowsb[:, :3]).all()
    pairs = _pair_items(2, H, W) + [dict(_pair_items(1, H, W)[0], image1=synthetic.image_pair(1, H, W)[1])]
    prm = _config("VisualizeTrackingError")
    single = runner.PairRunner(prm, device=DEV, batch=1)
    agg1, rows1 = single.run(pairs)
    assert single.batched_pairs == 0
    batched = runner.PairRunner(prm, device=DEV, batch=4)
    agg, rowsb = batched.run(pairs)
    assert batched.batched_pairs == 3
    assert np.array_equal(_bits(rows1), _bits(rowsb)), (rows1[:, :2], rowsb[:, :2])
    print("harris VisualizeTrackingError rows [track_error, tracked]: %s" % rowsb[:, :2].tolist())
    assert rowsb[:, 1].min() > 20 and np.isfinite(rowsb[:, :2]).all() and agg == agg1


def test_everything_that_matches_descriptors_refuses_harris_in_key_nets_words():
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.pipeline import PairPipeline, SequencePipeline
    H, W = 64, 96
    with pytest.raises(ValueError, match="Harris has no descriptors"):
        PairPipeline(_net(), EP, BF, 2, H, W, device=DEV)
    with pytest.raises(ValueError, match="Harris has no descriptors"):
        SequencePipeline(_net(), EP, BF, 2, H, W, device=DEV)
    item = _pair_items(1, H, W)[0]
    for task in ("MHA", "AUC", "match_stats", "FundamentalMatrixRansac"):
        r = runner.PairRunner(_config(task, matcher_params={"type": "brute_force", "brute_force_params": dict(BF, max_distance=5)}), device=DEV, batch=1)
        with pytest.raises(ValueError, match="Harris has no descriptors"):
            r.test_step(item, 0)
    seq = [{"image0": item["image0"], "fundamental": torch.eye(3), "dataset": "TartanAir"}]
    r = runner.PairRunner(_config("FundamentalMatrix", matcher_params={"type": "brute_force", "brute_force_params": dict(BF, max_distance=5)},
                                  FundamentalMatrix_params={"th": 3.0}), device=DEV, batch=1)
    with pytest.raises(ValueError, match="Harris has no descriptors"):
        r.run(seq)
