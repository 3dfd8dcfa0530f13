"""GPU parity of N12 (D2-Net: csrc/d2net.hip through the C ABI) against the reference class's own fp32 CPU maps with the seeded stand-in weights
(tests/golden/d2net*.npz), at five shapes: 8 x 8 (one cell: its 3 x 3 window is all padding, the upsampling scale 0), 16 x 24 (2 x 3 cells), 40 x 56 (odd cell
counts), 136 x 200 (17 x 25 at 1/8: one row and one column past a 16-wide tile) and 480 x 640; batch against solo; the per-image normalisation; detection on the
device's map against the reference's keypoints; refusals; the pipelines and the runner against the single-pair path, bit for bit.

Tolerance.  Per shape, `ref_err_score` / `ref_err_desc` = the reference's own max |fp32 run - the same model in .double()|.  The device must stay within
M x ref_err for the score and the descriptors alike; at 8 x 8 ref_err_score is 0 and the score must be exactly 1.0f.  Measured on an MI355X,
max |device - reference| / ref_err per shape (score / descriptors):
    split-f16 MFMA triples            8 x 8 - / 1.548, 16 x 24 2.264 / 2.324, 40 x 56 3.786 / 3.237, 136 x 200 3.340 / 3.091, 480 x 640 3.464 / 3.879
    strict fp32 (KPB_FP32_MATRIX=1)   8 x 8 - / 1.935, 16 x 24 2.264 / 2.188, 40 x 56 3.786 / 3.699, 136 x 200 3.712 / 3.572, 480 x 640 5.406 / 3.233
largest: split-f16 3.786 / 3.879, strict fp32 5.406 / 3.699, so M_H16 = 8 and M_FP32 = 16.  (ref_err_score is one to two units in the last place of the map's
maximum, 1e-6 of it at most: the ratios count single roundings.)  Detection on the device map found exactly the reference's keypoints on all six cases (1148 /
409 / 100 at 96 x 160, 95 / 29 / 95 at 40 x 56).
M_H16 and M_FP32 (d2net_fixtures.py) are the smallest powers of two that are at least twice the largest ratio of their arithmetic; M_FP32 stays under the 16
above which the strict kernels would count as defective."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights
from keypoint_bench_amd._lib import Context, KpbError, c_void_p, ptr
from d2net_fixtures import (DETECT_CAP_PERCENT, DETECT_CASES, DETECT_SHAPES, M_FP32, M_H16, SHAPES, chain, detect_params, load_parts, state_dict)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KPB_E_INVALID, KPB_E_WEIGHTS = -1, -6
EP = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
BF = dict(metric="euclidean", max_distance=5, cross_check=True)
FP32 = os.environ.get("KPB_FP32_MATRIX") == "1"
ARITH = "fp32" if FP32 else "split-f16"
M = M_FP32 if FP32 else M_H16


def _net():
    from keypoint_bench_amd.models.D2_Net import D2Net
    net = D2Net(use_cuda=True)
    net.load_state_dict(state_dict())
    return net.eval()


@pytest.fixture(scope="module")
def net():
    return _net()


@pytest.fixture(scope="module")
def gold():
    return load_parts("d2net")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _homo(hm, H, W):
    return dict(mode="homo", homography_matrix=hm, width=np.int64(W), height=np.int64(H))


def _digest(score, desc):
    """A checksum of the two maps' bit patterns."""
    import hashlib
    return hashlib.sha256(score.cpu().numpy().tobytes() + desc.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def _pixels(kps, H, W):
    """The set of (column, row) of detection's ((column + 0.5) / W, (row + 0.5) / H, score) rows."""
    return set(map(tuple, np.rint(np.asarray(kps, np.float64)[:, :2] * np.array([W, H]) - 0.5).astype(np.int64).tolist()))


def _batch3():
    return _t(np.stack([synthetic.image_pair(500 + i, 40, 56)[i & 1] for i in range(3)]))


# ------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("H,W", SHAPES)
def test_d2net_against_reference_golden(net, gold, H, W):
    tag = "%dx%d" % (H, W)
    v0, _ = synthetic.image_pair(0, H, W)
    assert synthetic.checksum(v0) == str(gold[tag + ".img.sum"])
    score, desc = net(_t(v0)[None])
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 512, H // 8, W // 8) and score.dtype == desc.dtype == torch.float32
    s, d = score[0, 0].cpu().numpy(), desc[0].cpu().numpy()
    r_s, r_d = float(gold[tag + ".ref_err_score"]), float(gold[tag + ".ref_err_desc"])
    e_s = float(np.abs(s.astype(np.float64) - gold[tag + ".score"]).max())
    dd = d if (H, W) != (480, 640) else d[:, ::4, ::4]
    e_d = float(np.abs(dd.astype(np.float64) - gold[tag + ".desc"]).max())
    norm = np.sqrt((d.astype(np.float64) ** 2).sum(0))
    print("d2net %s %s: max |error| score %.4g desc %.4g; ref_err %.4g / %.4g: ratios %s / %.3f, M = %d"
          % (tag, ARITH, e_s, e_d, r_s, r_d, "%.3f" % (e_s / r_s) if r_s > 0 else "-", e_d / r_d, M))
    assert np.isfinite(s).all() and float(s.min()) >= 0.0 and np.isfinite(d).all()
    assert float(np.abs(norm - 1.0).max()) <= 1e-5
    if (H, W) == (8, 8):
        assert r_s == 0.0 and np.array_equal(_bits(s), _bits(np.ones((8, 8), np.float32))), "the 8 x 8 score is not exactly 1.0f"
    else:
        assert e_s <= M * r_s, "the score is off: %.4g > %d x %.4g" % (e_s, M, r_s)
    assert e_d <= M * r_d, "the descriptors are off: %.4g > %d x %.4g" % (e_d, M, r_d)


# ------------------------------------------------------------------------------------------------ 2. batch equals solo
def test_d2net_batch_equals_solo_bit_for_bit(net):
    x = _batch3()
    s, d = net(x)
    s, d = s.clone(), d.clone()
    assert net.dim == 512 and net.desc_div == 8
    s2, d2 = net(x)
    assert torch.equal(s, s2) and torch.equal(d, d2)           # the sum is a fixed tree, the maximum order-independent
    for i in range(3):                          # alone: a pixel's bits depend on neither tile nor batch, an image's maximum and sum on no other image
        si, di = net(x[i:i + 1].contiguous())
        assert torch.equal(si[0], s[i]), "score of image %d: max |d| = %g" % (i, (si[0] - s[i]).abs().max().item())
        assert torch.equal(di[0], d[i]), "descriptors of image %d: max |d| = %g" % (i, (di[0] - d[i]).abs().max().item())
    assert not torch.equal(s[0], s[2])          # (different images)
    print("d2net bits 40x56 %s: %s" % (ARITH, _digest(s, d)))


# ------------------------------------------------------------------------------------------------ 3. strict fp32
@pytest.mark.timeout(300)
def test_d2net_strict_fp32_kernels_pass_the_goldens():
    """KPB_FP32_MATRIX is read once per process: tests 1 and 2 again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_d2net.py::test_d2net_against_reference_golden", "tests/test_gpu_d2net.py::test_d2net_batch_equals_solo_bit_for_bit"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=250)
    tail = "\n".join(p.stdout.splitlines()[-30:])
    print(tail)
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % tail
    assert "6 passed" in tail and "skipped" not in tail.split("passed")[-1], tail
    assert tail.count(" fp32: ") == 6, tail     # five goldens and the batch test, all under the knob
    # the child really ran other kernels: its maps of the batch test's input are not this process's split-f16 maps, bit for bit
    theirs = tail.split("d2net bits 40x56 fp32: ")[1].split()[0]
    s, d = _net()(_batch3())
    mine = _digest(s, d)
    print("d2net bits 40x56: split-f16 %s, strict fp32 %s" % (mine, theirs))
    assert len(theirs) == 16 and theirs != mine


# ------------------------------------------------------------------------------------------------ 4. per-image normalisation
def test_the_normalisation_is_per_image(net, gold):
    """Image 1 is image 0 x 0.25: another maximum, another sum.  Image 0's maps are those of image 0 alone, and each map sums to what the reference's does.  (At
    40 x 56 the coarse map is 5 x 7 and its nodes sit at multiples of 39 / 4 and 55 / 6: no stride of the fine map lands on them, so the sums are compared.)"""
    H, W = 40, 56
    v0, _ = synthetic.image_pair(0, H, W)
    x = _t(np.stack([v0, 0.25 * v0]).astype(np.float32))
    s, d = net(x)
    s, d = s.clone(), d.clone()
    s0, d0 = net(x[:1].contiguous())
    assert torch.equal(s0[0], s[0]) and torch.equal(d0[0], d[0])
    s1, d1 = net(x[1:].contiguous())
    assert torch.equal(s1[0], s[1]) and torch.equal(d1[0], d[1])
    assert not torch.equal(s[0], s[1])
    with torch.no_grad():
        ref1 = chain(weights.fold_d2net(state_dict()), x[1:].cpu())[0][0, 0].numpy()        # the reference's arithmetic on the CPU (tests/test_d2net_cpu.py)
    r_s = float(gold["40x56.ref_err_score"])
    for i, ref in enumerate((gold["40x56.score"], ref1)):
        got, want = float(s[i].cpu().numpy().astype(np.float64).sum()), float(ref.astype(np.float64).sum())
        print("d2net per-image sum %s, image %d: %.9g (reference %.9g), |difference| %.3g, bound %.3g" % (ARITH, i, got, want, abs(got - want), M * r_s * H * W))
        assert abs(got - want) <= M * r_s * H * W


# ------------------------------------------------------------------------------------------------ 5. / 6. detection
@pytest.mark.parametrize("H,W", DETECT_SHAPES)
@pytest.mark.parametrize("nms_dist,top_k", DETECT_CASES)
def test_detection_on_the_device_map_finds_the_reference_keypoints(net, H, W, nms_dist, top_k):
    from keypoint_bench_amd.utils.extracter import detection
    want = load_parts("d2net_detect")["%dx%d.nd%d.k%d" % (H, W, nms_dist, top_k)]
    score, _ = net(_t(synthetic.image_pair(0, H, W)[0])[None])
    kps = detection(score, detect_params(nms_dist, top_k)).cpu().numpy()
    a, b = _pixels(kps, H, W), _pixels(want, H, W)
    diff = len(a ^ b)
    print("d2net detect %dx%d nms_dist %d top_k %d: %d keypoints (reference %d), symmetric difference %d" % (H, W, nms_dist, top_k, len(a), len(b), diff))
    assert len(b) == want.shape[0] and len(a) == kps.shape[0]
    assert 100 * diff <= DETECT_CAP_PERCENT * len(b)


@pytest.mark.parametrize("H,W", DETECT_SHAPES)
@pytest.mark.parametrize("nms_dist,top_k", DETECT_CASES)
def test_detection_on_the_reference_map_equals_the_reference_keypoints(H, W, nms_dist, top_k):
    from keypoint_bench_amd.utils.extracter import detection
    det = load_parts("d2net_detect")
    want = det["%dx%d.nd%d.k%d" % (H, W, nms_dist, top_k)]
    kps = detection(_t(det["%dx%d.score" % (H, W)])[None, None], detect_params(nms_dist, top_k)).cpu().numpy()
    assert kps.shape == want.shape and kps.dtype == want.dtype == np.float32
    rows = lambda k: sorted(map(tuple, _bits(k).tolist()))
    assert rows(kps) == rows(want)
    if want.shape[0] == top_k:                  # cut by top_k: the reference's descending order too
        assert np.array_equal(_bits(kps), _bits(want))


# ------------------------------------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("H,W", [(12, 16), (16, 12), (4, 8)])
def test_a_shape_that_is_no_multiple_of_8_is_refused_and_the_net_stays_usable(net, H, W):
    x = _t(synthetic.image_pair(0, 32, 64)[0])[None]
    s, d = net(x)
    s, d = s.clone(), d.clone()
    bad = _t(synthetic.image_pair(0, 16, 16)[0][:, :H, :W])[None]
    score = torch.full((1, 1, H, W), 7.0, device=DEV)
    desc = torch.full((1, 2, 2, 512), 7.0, device=DEV)
    ctx = net._ctx
    rc = ctx.lib.kpb_net_forward(net._handle, ptr(bad), 1, H, W, ptr(score), ptr(desc))
    assert rc == KPB_E_INVALID
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    assert "D2Net" in msg and "%dx%d" % (H, W) in msg, msg
    ctx.sync()
    assert bool((score == 7.0).all()) and bool((desc == 7.0).all())         # nothing written
    with pytest.raises(KpbError):
        net(bad)
    s2, d2 = net(x)
    assert torch.equal(s, s2) and torch.equal(d, d2)


def test_a_null_descriptor_pointer_is_refused(net):
    H, W = 32, 64
    x = _t(synthetic.image_pair(0, H, W)[0])[None]
    s, d = net(x)
    s = s.clone()
    score = torch.full((1, 1, H, W), 7.0, device=DEV)
    ctx = net._ctx
    rc = ctx.lib.kpb_net_forward(net._handle, ptr(x), 1, H, W, ptr(score), ptr(None))
    assert rc == KPB_E_INVALID
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    assert "D2Net" in msg and "desc_out_dev" in msg, msg
    ctx.sync()
    assert bool((score == 7.0).all())
    assert torch.equal(net(x)[0], s)


def _create(arch, tensors, blob_arch=None, cut=None):
    ctx = Context.get(torch.device(DEV))
    blob = weights.pack(tensors, arch if blob_arch is None else blob_arch)
    if cut is not None:
        blob = blob[:cut]
    h = c_void_p()
    rc = ctx.lib.kpb_net_create(ctx.handle, arch, blob, len(blob), ctypes.byref(h))
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    if h.value:
        ctx.lib.kpb_net_destroy(h)
    return rc, msg, bool(h.value)


def test_create_refuses_truncated_misshaped_missing_and_foreign_blobs(net):
    from sfd2_fixtures import state_dict as sfd2_state_dict
    D, A, S = weights.ARCH_D2NET, weights.ARCH_ALIKE, weights.ARCH_SFD2
    t = weights.fold_d2net(state_dict())
    x = _t(synthetic.image_pair(0, 32, 64)[0])[None]
    s, d = net(x)
    s, d = s.clone(), d.clone()
    whole = len(weights.pack(t, D))
    for cut in (8, 100, whole // 2, whole - 4):
        rc, msg, made = _create(D, t, cut=cut)
        assert rc == KPB_E_WEIGHTS and not made and "malformed" in msg, (cut, msg)
    for name in ("conv1_1.w", "conv1_1.b", "conv3_2.w", "conv3_2.b", "conv4_3.w", "conv4_3.b"):      # the first, a middle and the last layer
        rc, msg, made = _create(D, {k: v for k, v in t.items() if k != name})
        assert rc == KPB_E_WEIGHTS and not made and name in msg and "D2Net" in msg, msg
    for name, wrong in (("conv1_1.w", t["conv1_1.w"][:, :1]), ("conv3_2.w", t["conv3_2.w"][:, :, 0, 0]), ("conv4_1.w", np.zeros((512, 512, 3, 3), np.float32)),
                        ("conv4_3.w", t["conv4_3.w"][:256]), ("conv4_3.b", t["conv4_3.b"][:256])):
        rc, msg, made = _create(D, dict(t, **{name: wrong}))
        assert rc == KPB_E_WEIGHTS and not made and name in msg and "D2Net" in msg, msg
    alike, sfd2 = weights.load_alike_t(), weights.fold_sfd2(sfd2_state_dict())
    for arch, tensors, names in ((D, alike, ("conv1_1.w", "D2Net")), (D, sfd2, ("conv1_1.w", "D2Net")), (A, t, ("b1c1.w",)), (S, t, ("conv1a.w", "SFD2"))):
        rc, msg, made = _create(arch, tensors)
        assert rc == KPB_E_WEIGHTS and not made and all(n in msg for n in names), (arch, msg)
    for blob_arch, arch, tensors in ((A, D, alike), (D, A, t), (D, S, t), (S, D, sfd2)):       # a blob under another net's arch id
        rc, msg, made = _create(arch, tensors, blob_arch)
        assert rc == KPB_E_WEIGHTS and not made, (blob_arch, arch, msg)
    rc, msg, made = _create(D, t)               # the intact one is created on the same context
    assert rc == 0 and made, msg
    s2, d2 = net(x)
    assert torch.equal(s2, s) and torch.equal(d2, d)


# ------------------------------------------------------------------------------------------------ 8. pipelines
def test_pair_pipeline_with_matching_equals_the_single_pair_path():
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import match_descriptors, sample_descriptors
    B, H, W = 2, 96, 128
    v = [synthetic.image_pair(20 + i, H, W) for i in range(B)]
    i0, i1 = np.stack([a for a, _ in v]), np.stack([b for _, b in v])
    net = _net()
    assert net.dense_descriptors is True        # D2-Net always writes its map: there is no keypoint-only path to run as well
    pipe = PairPipeline(net, EP, BF, B, H, W, device=DEV)
    assert pipe.div == 8 and pipe.C == 512 and (pipe.Hd, pipe.Wd) == (12, 16) and pipe.desc.shape == (2 * B, 12, 16, 512)
    pipe.run(_t(np.concatenate([i0, i1])))
    single = _net()
    most = 0
    for b in range(B):
        got = pipe.pair(b)
        s0, d0 = single(_t(i0[b])[None])
        k0 = detection(s0, EP)
        f0 = sample_descriptors(k0, d0)
        s1, d1 = single(_t(i1[b])[None])
        k1 = detection(s1, EP)
        f1 = sample_descriptors(k1, d1)
        assert f0.shape == (k0.shape[0], 512)
        np.testing.assert_array_equal(_bits(got["kps0"]), _bits(k0.cpu().numpy()))
        np.testing.assert_array_equal(_bits(got["kps1"]), _bits(k1.cpu().numpy()))
        np.testing.assert_array_equal(_bits(pipe.sdesc[b, :k0.shape[0]].cpu().numpy()), _bits(f0.cpu().numpy()))        # sampled from the 1/8-resolution map
        np.testing.assert_array_equal(_bits(pipe.sdesc[B + b, :k1.shape[0]].cpu().numpy()), _bits(f1.cpu().numpy()))
        pairs, dist = match_descriptors(f0, f1, max_distance=5, cross_check=True, return_distance=True)      # 512 channels: the exact match_tile path, no prefilter
        np.testing.assert_array_equal(got["pairs"], pairs.cpu().numpy())
        np.testing.assert_array_equal(_bits(got["dist"]), _bits(dist.cpu().numpy()))
        most = max(most, got["pairs"].shape[0])
    print("d2net pipeline: most matches of a pair %d" % most)
    assert most > 5
    # SequencePipeline on the same net: pair 1 of a two-frame chunk is (frame 0, frame 1), matched from the same 1/8-resolution maps
    from keypoint_bench_amd.pipeline import SequencePipeline
    seq = SequencePipeline(_net(), EP, BF, 2, H, W, device=DEV)
    assert seq.div == 8 and seq.desc.shape == (2, 12, 16, 512)
    seq.run(_t(np.stack([i0[0], i1[0]])), first=True)
    want = pipe.pair(0)
    k = int(seq.k[1])
    np.testing.assert_array_equal(_bits(seq.kps[1, :int(seq.n[1])].cpu().numpy()), _bits(want["kps0"]))
    np.testing.assert_array_equal(_bits(seq.kps[2, :int(seq.n[2])].cpu().numpy()), _bits(want["kps1"]))
    np.testing.assert_array_equal(seq.pairs[1, :k].cpu().numpy(), want["pairs"])
    np.testing.assert_array_equal(_bits(seq.dist[1, :k].cpu().numpy()), _bits(want["dist"]))


# ------------------------------------------------------------------------------------------------ 9. runner
@pytest.mark.parametrize("task", ["repeatability", "MHA"])
def test_runner_rows_batched_equal_single(tmp_path, task):
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.models.D2_Net import D2Net
    path = str(tmp_path / "d2_tf.pth")
    torch.save({"model": state_dict()}, path)
    H, W = 96, 128
    ds = []
    for i in range(3):
        v0, v1, hm = synthetic.warped_pair(1 + i, H, W, strength=1.0)
        ds.append({"image0": v0, "image1": v1, "dataset": "HPatches", "warp01_params": _homo(hm, H, W),
                   "warp10_params": _homo(np.linalg.inv(hm).astype(np.float32), H, W)})
    prm = {"model_type": "D2Net", "task_type": task, "D2Net_params": dict(weight=path), "extractor_params": EP,
           "matcher_params": {"type": "brute_force", "brute_force_params": BF}, "repeatability_params": {"th": 3}, "MHA_params": {"th": [3, 5, 7]}}
    single = runner.PairRunner(prm, device=DEV, batch=1)
    assert isinstance(single.model, D2Net) and single.model.dim == 512 and single.model.desc_div == 8
    _, rows1 = single.run(ds)
    assert single.batched_pairs == 0
    batched = runner.PairRunner(prm, device=DEV, batch=4)
    agg, rowsb = batched.run(ds)
    assert batched.batched_pairs == 3
    assert np.array_equal(rows1.view(np.uint64), rowsb.view(np.uint64)), (rows1, rowsb)
    print("runner %s rows: %s" % (task, rowsb[:, :4].tolist()))
    if task == "repeatability":
        assert np.isfinite(agg["repeatability"])
    else:
        assert len(agg["MHA"]) == 3 and all(np.isfinite(a) for a in agg["MHA"])
