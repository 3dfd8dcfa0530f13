"""kpb_lk_track_batch (csrc/lk.hip): the Lucas-Kanade tracker for a batch of pairs on maps of any strides, and what is built on it --
utils/matcher.optical_flow_batch, SequencePipeline(track=...) and the runner's batched optical_flow branch.

The entry's contract needs no new reference: every pair's rows equal, BIT FOR BIT, what kpb_lk_track returns for that pair's maps made
planar-contiguous with the same points, units and parameters.  Tests 1-4 check that through the C ABI; 5 ties the chain GoodPoint map -> tracker to
the reference's own tracker on the reference's maps (tests/golden/goodpoint_track.npz), within test_gpu_lk.ATOL_PX on the points the reference itself
reproduces (`stable`, 198 of 200 in both sets; cap 5 %); 6 and 7 check the sequence pipeline and the runner against the single-pair path, bit for bit.

Measured on an MI355X, test 5: the device's maps differ from the reference's by 4.8e-7; on stable points the device chain is within 5.3e-5 px
(error column 3.2e-5) of the reference with the class defaults and 1.1e-5 px (8.6e-6) with config_fund.yaml's set, against ATOL_PX = 1e-3."""
import ctypes

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic
from keypoint_bench_amd._lib import Context, LkParams, ptr
from goodpoint_fixtures import CAP_PERCENT, PARAM, TRACK_SETS, checkpoint, load_parts, track_params
from test_gpu_lk import ATOL_PX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KPB_OK, KPB_E_INVALID, KPB_E_UNSUPPORTED = 0, -1, -7
SENTINEL = np.float32(-7.5)
DEFAULTS = dict(distance=3, win_size=3, levels=1, interation=40)
FUND = dict(distance=10, win_size=21, levels=3, interation=40)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lp(prm):
    return LkParams(float(prm["distance"]), int(prm["win_size"]), int(prm["levels"]), int(prm["interation"]))


def _maps(n, C, H, W, seed=40):
    """n + 1 consecutive maps [n+1, C, H, W]: a seeded smooth canvas sliding by (2, 1) px a step, plus a little noise."""
    rng = np.random.default_rng(seed)
    canvas = rng.random((C, H + 2 * n + 8, W + 2 * n + 8))
    blur = sum(canvas[:, i:i + H + 2 * n + 4, j:j + W + 2 * n + 4] for i in range(5) for j in range(5)) / 25.0
    blur = (blur - blur.min()) / (blur.max() - blur.min())
    return np.stack([blur[:, i:i + H, 2 * i:2 * i + W] + rng.normal(0, 0.01, (C, H, W)) for i in range(n + 1)]).astype(np.float32)


def _points(B, K, seed=41):
    rng = np.random.default_rng(seed)
    pts1 = rng.uniform(0.0, 1.0, (B, K, 2)).astype(np.float32)
    pts1[:, :4] = [(0, 0), (1, 1), (0, 1), (1, 0)]         # the corners: zero padding of every stage and the start clamp
    pts2 = np.clip(pts1 + rng.normal(0, 0.02, (B, K, 2)), 0, 1).astype(np.float32)
    ang = rng.normal(size=(B, K)) * 6.28
    return pts1, pts2, np.stack([np.cos(ang), np.sin(ang)], 2).astype(np.float32)


def single(m1, m2, pts1, pts2, unit, prm):
    """kpb_lk_track on one pair's planar maps [C, H, W] (numpy): (out [n, 2], err [n])."""
    ctx = Context.get(torch.device(DEV))
    C, H, W = m1.shape
    n = pts1.shape[0]
    out, err = torch.empty((n, 2), device=DEV), torch.empty((n,), device=DEV)
    bufs = [_t(m1), _t(m2), _t(pts1), _t(pts2), _t(unit)]
    rc = ctx.lib.kpb_lk_track(ctx.handle, ptr(bufs[0]), ptr(bufs[1]), C, H, W, ptr(bufs[2]), ptr(bufs[3]), pts1.shape[1], ptr(bufs[4]), n,
                              ctypes.byref(_lp(prm)), ptr(out), ptr(err))
    assert rc == KPB_OK, ctx.lib.kpb_last_error(ctx.handle).decode()
    ctx.sync()
    return out.cpu().numpy(), err.cpu().numpy()


def batch(maps1, maps2, pts1, pts2, unit, n, prm, B=None, K=None, C=None, H=None, W=None, strides=None, stride=None, null=False):
    """kpb_lk_track_batch on device tensors maps1 / maps2 [B, C, H, W] of any strides: (rc, out [B, K, 2], err [B, K]) with sentinels where nothing
    was written.  The keyword overrides feed the refusal test."""
    ctx = Context.get(torch.device(DEV))
    b, c, h, w = maps1.shape
    k = pts1.shape[1]
    out = torch.full((b, k, 2), float(SENTINEL), device=DEV)
    err = torch.full((b, k), float(SENTINEL), device=DEV)
    sb, sc, sh, sw = strides or maps1.stride()
    pick = lambda v, d: d if v is None else v
    bufs = [None] * 5 if null else [pts1, pts2, unit, out, err]
    rc = ctx.lib.kpb_lk_track_batch(ctx.handle, ptr(maps1), ptr(maps2), pick(B, b), pick(C, c), pick(H, h), pick(W, w), sb, sc, sh, sw, ptr(bufs[0]),
                                    ptr(bufs[1]), pick(stride, pts1.shape[2]), ptr(bufs[2]), pick(K, k), ptr(n), ctypes.byref(_lp(prm)), ptr(bufs[3]),
                                    ptr(bufs[4]))
    ctx.sync()
    return rc, out.cpu().numpy(), err.cpu().numpy()


def assert_pairs_equal_single(maps1, maps2, pts1, pts2, unit, counts, prm, out, err):
    """maps*, pts*, unit: numpy, planar; counts: rows tracked per pair."""
    for j, nj in enumerate(counts):
        if nj:
            o, e = single(maps1[j], maps2[j], pts1[j, :nj], pts2[j, :nj], unit[j, :nj], prm)
            assert np.array_equal(_bits(out[j, :nj]), _bits(o)), (j, np.abs(out[j, :nj] - o).max())
            assert np.array_equal(_bits(err[j, :nj]), _bits(e)), j
        assert (out[j, nj:] == SENTINEL).all() and (err[j, nj:] == SENTINEL).all(), j


# ------------------------------------------------------------------------------------------------ 1. batch equals single
@pytest.mark.parametrize("C", [3, 1])
def test_batch_equals_single_with_counts_and_without(C):
    K, counts = 9, (0, 5, 9)
    m = _maps(5, C, 32, 48)
    m1, m2 = m[:3], m[3:6]                 # three unrelated pairs, held apart
    pts1, pts2, unit = _points(3, K)
    prm = dict(DEFAULTS, win_size=5, levels=2, interation=10)
    args = (_t(m1), _t(m2), _t(pts1), _t(pts2), _t(unit))
    rc, out, err = batch(*args, _t(np.array(counts, np.int32)), prm)
    assert rc == KPB_OK
    assert_pairs_equal_single(m1, m2, pts1, pts2, unit, counts, prm, out, err)
    rc, out, err = batch(*args, None, prm)                      # n_dev = NULL: max_n rows of every pair
    assert rc == KPB_OK and np.isfinite(out).all()
    assert_pairs_equal_single(m1, m2, pts1, pts2, unit, (K, K, K), prm, out, err)


# ------------------------------------------------------------------------------------------------ 2. strides
def test_strides_overlapping_maps_and_separate_second_points():
    K = 9
    m = _maps(3, 3, 32, 48)                 # four consecutive maps: three pairs (j, j + 1)
    pts1, pts2, unit = _points(3, K)
    prm = dict(DEFAULTS, win_size=7, levels=2, interation=20)
    n = _t(np.array([7, 9, 4], np.int32))
    p1, p2, u = _t(pts1), _t(pts2), _t(unit)
    planar = _t(m)
    rc, want, want_err = batch(_t(m[:3]), _t(m[1:]), p1, p2, u, n, prm)     # the pairs held apart, planar
    assert rc == KPB_OK
    assert_pairs_equal_single(m[:3], m[1:], pts1, pts2, unit, (7, 9, 4), prm, want, want_err)
    rc, out, err = batch(planar[:3], planar[1:], p1, p2, u, n, prm)         # map2 = map1 + sb
    assert rc == KPB_OK and planar[1:].data_ptr() == planar.data_ptr() + 4 * planar.stride(0)
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(err), _bits(want_err))
    last = _t(m.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2)                  # channels-last storage, [B, C, H, W] view
    assert last.stride() == (32 * 48 * 3, 1, 48 * 3, 3) and torch.equal(last, planar)
    rc, out, err = batch(last[:3], last[1:], p1, p2, u, n, prm)
    assert rc == KPB_OK
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(err), _bits(want_err))
    rc, same, _ = batch(planar[:3], planar[1:], p1, p1, u, n, prm)          # pts2 = pts1 (one buffer) is another track
    assert rc == KPB_OK and not np.array_equal(_bits(same), _bits(want))
    assert_pairs_equal_single(m[:3], m[1:], pts1, pts1, unit, (7, 9, 4), prm, same, _)
    wide = np.concatenate([pts1, np.full((3, K, 1), np.nan, np.float32)], 2)                    # pts_stride 3
    wide2 = np.concatenate([pts2, np.full((3, K, 1), np.nan, np.float32)], 2)
    rc, out, err = batch(planar[:3], planar[1:], _t(wide), _t(wide2), u, n, prm)
    assert rc == KPB_OK and np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(err), _bits(want_err))


# ------------------------------------------------------------------------------------------------ 3. parameter sets
@pytest.mark.parametrize("prm", [DEFAULTS, dict(distance=3, win_size=7, levels=2, interation=20), FUND], ids=["defaults", "3-7-2-20", "config_fund"])
def test_parameter_sets_at_64x96(prm):
    K = 12
    m = _maps(2, 3, 64, 96, seed=50)
    pts1, pts2, unit = _points(2, K, seed=51)
    last = _t(m.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2)
    rc, out, err = batch(last[:2], last[1:], _t(pts1), _t(pts2), _t(unit), _t(np.array([K, 10], np.int32)), prm)
    assert rc == KPB_OK
    assert_pairs_equal_single(m[:2], m[1:], pts1, pts2, unit, (K, 10), prm, out, err)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_write_nothing_and_leave_the_context_usable():
    K = 9
    m = _maps(2, 3, 32, 48)
    pts1, pts2, unit = _points(2, K)
    a = (_t(m[:2]), _t(m[1:]), _t(pts1), _t(pts2), _t(unit), None)
    prm = dict(DEFAULTS)
    rc, want, want_err = batch(*a, prm)
    assert rc == KPB_OK
    five = torch.zeros((2, 5, 32, 48), device=DEV)
    refused = [(KPB_E_INVALID, dict(B=0), {}), (KPB_E_INVALID, dict(B=-1), {}), (KPB_E_INVALID, dict(K=-1), {}), (KPB_E_INVALID, dict(H=20), {}),
               (KPB_E_INVALID, dict(W=20), {}), (KPB_E_INVALID, dict(C=0), {}), (KPB_E_INVALID, dict(stride=1), {}),
               (KPB_E_INVALID, dict(strides=(0, 32 * 48, 48, 1)), {}), (KPB_E_INVALID, dict(strides=(3 * 32 * 48, 0, 48, 1)), {}),
               (KPB_E_INVALID, dict(strides=(3 * 32 * 48, 32 * 48, -48, 1)), {}), (KPB_E_INVALID, dict(strides=(3 * 32 * 48, 32 * 48, 48, 0)), {}),
               (KPB_E_UNSUPPORTED, {}, dict(win_size=4)), (KPB_E_UNSUPPORTED, {}, dict(win_size=33)), (KPB_E_UNSUPPORTED, {}, dict(levels=0)),
               (KPB_E_UNSUPPORTED, {}, dict(levels=5)), (KPB_E_UNSUPPORTED, {}, dict(interation=-1)), (KPB_E_UNSUPPORTED, dict(B=65536), {})]
    ctx = Context.get(torch.device(DEV))
    for code, kw, pk in refused:
        assert ctx.lib.kpb_ctx_set_option(ctx.handle, 9999, 0) == KPB_E_INVALID       # another entry point's message first
        rc, out, err = batch(*a, dict(prm, **pk), **kw)
        msg = ctx.lib.kpb_last_error(ctx.handle).decode()
        assert rc == code, (kw, pk, rc, msg)
        assert msg.startswith("kpb_lk_track_batch:"), (kw, pk, msg)
        assert (out == SENTINEL).all() and (err == SENTINEL).all(), (kw, pk)
    rc, out, err = batch(five, five, *a[2:], dict(prm, win_size=31))                  # 4 * 5 * 31^2 floats: over the LDS bound
    assert rc == KPB_E_UNSUPPORTED and (out == SENTINEL).all() and ctx.lib.kpb_last_error(ctx.handle).decode().startswith("kpb_lk_track_batch:")
    rc, _, _ = batch(*a, prm, K=0, null=True)
    assert rc == KPB_OK
    rc, _, _ = batch(*a, prm, null=True)
    assert rc == KPB_E_INVALID
    rc, out, err = batch(*a, prm)
    assert rc == KPB_OK and np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(err), _bits(want_err))


# ------------------------------------------------------------------------------------------------ 5. the chain, from the reference
def _goodpoint():
    from keypoint_bench_amd.models.GoodPoint import GoodPoint
    net = GoodPoint(PARAM)
    net.load_state_dict(checkpoint())
    return net.eval()


@pytest.mark.parametrize("name", TRACK_SETS)
def test_goodpoint_maps_tracked_like_the_reference_tracks_its_own(name):
    from keypoint_bench_amd.utils.matcher import optical_flow_batch
    g = load_parts("goodpoint_track")
    seed, H, W = (int(v) for v in g["image_pair"])
    v0, v1 = synthetic.image_pair(seed, H, W)
    _, maps = _goodpoint()(_t(np.stack([v0, v1])))               # [2, 3, H, W] view over channels-last storage
    assert maps.stride() == (H * W * 3, 1, W * 3, 3)
    print("goodpoint maps vs the reference's: %.3g" % float(np.abs(maps.cpu().numpy() - np.stack([g["map0"], g["map1"]])).max()))
    kps = _t(g["kps"])[None]
    out, err = optical_flow_batch(maps[:1], maps[1:], kps, kps, None, track_params(g, name), random_angle=_t(g[name + "_angle"])[None])
    out, err, stable = out[0].cpu().numpy(), err[0].cpu().numpy(), g[name + "_stable"]
    assert 100 * int((~stable).sum()) <= CAP_PERCENT * stable.size
    dp, de = np.abs(out - g[name + "_out"])[stable].max(), np.abs(err - g[name + "_err"])[stable].max()
    print("%s stable %d/%d: device chain vs reference %.3g px (err %.3g); ATOL_PX %g" % (name, stable.sum(), stable.size, dp, de, ATOL_PX))
    np.testing.assert_allclose(out[stable], g[name + "_out"][stable], rtol=0, atol=ATOL_PX)
    np.testing.assert_allclose(err[stable], g[name + "_err"][stable], rtol=0, atol=ATOL_PX)


# ------------------------------------------------------------------------------------------------ 6. SequencePipeline(track=...)
EP = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)


def sequence_frames(n, h=96, w=128):
    canvas, _ = synthetic.image_pair(300, h + 40, w + 40)
    return np.stack([canvas[:, i:i + h, 2 * i:2 * i + w] for i in range(n)]).astype(np.float32)


def _alike():
    from keypoint_bench_amd.models.ALike import alike_t
    return alike_t()


@pytest.mark.parametrize("make", [_goodpoint, _alike], ids=["GoodPoint-maps", "ALIKE-frames"])
def test_sequence_pipeline_tracks_like_the_single_pair_tracker(make):
    from keypoint_bench_amd.pipeline import SequencePipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import OpticalFlow
    F, H, W = 2, 96, 128
    frames = _t(sequence_frames(5, H, W))
    prm = dict(distance=3, win_size=7, levels=2, interation=20, gray=False)
    net, solo = make(), make()
    pipe = SequencePipeline(net, EP, None, F, H, W, device=DEV, track=prm)
    K = pipe.top_k
    angles = _t((np.random.default_rng(60).normal(size=(5, K)) * 6.28).astype(np.float32))
    prev = None
    for c0 in range(0, 5, F):               # chunks of 2, 2, 1: the carried slot is used twice
        f = min(F, 5 - c0)
        pipe.run(frames[c0:c0 + f].contiguous(), first=(c0 == 0), angles=angles[c0:c0 + f])
        n, tracked, terr, kps = pipe.n.cpu().numpy(), pipe.tracked.cpu().numpy(), pipe.track_err.cpu().numpy(), pipe.kps.cpu().numpy()
        assert np.array_equal(pipe.k[:f].cpu().numpy(), n[:f])
        for j in range(f):
            i = c0 + j
            s, d = solo(frames[i:i + 1])
            cur = dict(kps=detection(s, EP), map=(d if net.tracked_maps else frames[i:i + 1]).clone())
            if prev is None:
                prev = cur                  # frame 0 is paired with itself
            k = prev["kps"]
            assert n[j] == k.shape[0] > 20 and np.array_equal(kps[j, :n[j]], k.cpu().numpy())
            assert prev["map"].shape == (1, 3, H, W)
            o, e = OpticalFlow(prm)(prev["map"], cur["map"], k, k, random_angle=angles[i, :n[j]])
            assert np.array_equal(_bits(tracked[j, :n[j]]), _bits(o[0].cpu().numpy())), (i, np.abs(tracked[j, :n[j]] - o[0].cpu().numpy()).max())
            assert np.array_equal(_bits(terr[j, :n[j]]), _bits(e[0].cpu().numpy())), i
            if i == 0:                      # tracked from a map into itself: every point comes back to within the tracker's own convergence
                assert float(e.max()) < 8.0
            prev = cur


# ------------------------------------------------------------------------------------------------ 7. the runner
def test_runner_batches_optical_flow_and_hands_goodpoint_maps_to_the_tracker(tmp_path, monkeypatch):
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.utils import matcher
    path = str(tmp_path / "goodpoint.pth")
    torch.save(checkpoint(), path)
    rng = np.random.default_rng(9)
    ds = [{"image0": fr.copy(), "fundamental": torch.from_numpy(rng.normal(size=(3, 3)).astype(np.float32)), "dataset": "TartanAir"}
          for fr in sequence_frames(5)]
    prm = {"model_type": "GoodPoint", "task_type": "FundamentalMatrix", "GoodPoint_params": dict(PARAM, weight=path), "extractor_params": EP,
           "matcher_params": {"type": "optical_flow", "optical_flow_params": dict(distance=0, win_size=7, levels=2, interation=20, gray=False)},
           "FundamentalMatrix_params": {"th": 3.0}}
    seen = []
    real = matcher.optical_flow_tensor

    def recorder(pts0, pts1, img0, img1, params=None):
        seen.append((img0.clone(), img1.clone()))
        return real(pts0, pts1, img0, img1, params)

    monkeypatch.setattr(matcher, "optical_flow_tensor", recorder)
    single = runner.PairRunner(prm, device=DEV, batch=1)
    _, rows1 = single.run(ds)
    assert single.batched_pairs == 0 and rows1.shape[0] == 5 and len(seen) == 5
    net = single.model
    for i, (m0, m1) in enumerate(seen):             # the descriptor maps, not the frames
        assert m0.shape == m1.shape == (1, 3, 96, 128)
        want0 = net(_t(ds[max(i - 1, 0)]["image0"])[None])[1].clone()
        want1 = net(_t(ds[i]["image0"])[None])[1].clone()
        assert torch.equal(m0, want0) and torch.equal(m1, want1), i
        assert not torch.equal(m1, _t(ds[i]["image0"])[None])
    seen.clear()
    batched = runner.PairRunner(prm, device=DEV, batch=4)
    _, rowsb = batched.run(ds)
    assert batched.batched_pairs == 5 and not seen
    assert np.array_equal(rows1.view(np.uint64), rowsb.view(np.uint64)), (rows1, rowsb)
    assert rowsb[:, 2].min() >= 0 and np.isfinite(rowsb[:, :3]).all()
    vo = dict(prm, task_type="visual_odometer")     # cv2's tracker stays refused
    with pytest.raises(NotImplementedError):
        runner.PairRunner(vo, device=DEV, batch=4).run([dict(d, pose=np.eye(4, dtype=np.float32)) for d in ds])
