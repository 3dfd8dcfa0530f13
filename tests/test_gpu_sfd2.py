"""GPU parity of N11 (SFD2: csrc/sfd2.hip through the C ABI) against the reference class's own fp32 CPU maps with the seeded stand-in weights
(tests/golden/sfd2*.npz), at five shapes: 8 x 8 (one cell, out4 2 x 2), 16 x 24, 40 x 56 (odd cell counts), 72 x 104 (18 x 26 at 1/4: a 16-row tile plus two rows)
and 480 x 640; batch against solo; the grouped layer alone; detection on the device's map against the reference's keypoints; refusals; the pipelines and the
runner against the single-pair path, bit for bit.

Tolerance.  Per shape, `ref_err_score` / `ref_err_desc` = the reference's own max |fp32 run - the same model in .double()|.  The stability factor is a step
function (0.1 / 0.5 / 1.0 by the argmax of three upsampled logits): pixels whose two largest logits lie closer than 1e-3 in float64 (`margin`, at most 1 % of a
shape by the generator's condition (b); 0.27 % at most here) are left out of the score check, everywhere else a wrong class is a factor >= 2 and fails.  The device
must stay within M x ref_err for the score and the descriptors alike.  Measured on an MI355X, largest max |device - reference| / ref_err over the five shapes
(score / descriptors):
    split-f16 MFMA triples   2.246 (40 x 56) / 2.232 (72 x 104)      strict fp32 (KPB_FP32_MATRIX=1)   2.968 (40 x 56) / 2.401 (72 x 104)
per shape, split-f16: 8 x 8 1.873 / 1.532, 16 x 24 1.915 / 1.446, 40 x 56 2.246 / 1.693, 72 x 104 1.853 / 2.232, 480 x 640 1.968 / 1.353; strict fp32:
2.809 / 2.065, 2.804 / 1.675, 2.968 / 1.971, 2.100 / 2.401, 1.689 / 1.504.  M_H16 = 8 and M_FP32 = 8 (sfd2_fixtures.py) are the smallest powers of two that are at
least twice the largest ratio of their arithmetic; M_FP32 stays under the 16 above which the strict kernels would count as defective.  Detection on the device
map found exactly the reference's keypoints on all six cases (724 / 180 / 100 at 96 x 160, 64 / 15 / 64 at 40 x 56)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights
from keypoint_bench_amd._lib import Context, KpbError, c_void_p, ptr
from sfd2_fixtures import (DETECT_CAP_PERCENT, DETECT_CASES, DETECT_SHAPES, M_FP32, M_H16, MARGIN, SHAPES, detect_params, load_parts, state_dict)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KPB_E_INVALID, KPB_E_WEIGHTS = -1, -6
EP = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
BF = dict(metric="euclidean", max_distance=5, cross_check=True)


def _net():
    from keypoint_bench_amd.models.sfd2 import ResSegNetV2
    net = ResSegNetV2(outdim=128, require_stability=True)
    net.load_state_dict(state_dict(), strict=False)
    return net.eval()


@pytest.fixture(scope="module")
def net():
    return _net()


@pytest.fixture(scope="module")
def gold():
    return load_parts("sfd2")


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


# ------------------------------------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("H,W", SHAPES)
def test_sfd2_against_reference_golden(net, gold, H, W):
    tag = "%dx%d" % (H, W)
    v0, _ = synthetic.image_pair(0, H, W)
    assert synthetic.checksum(v0) == str(gold[tag + ".img.sum"])
    score, desc = net(_t(v0)[None])
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 128, H // 4, W // 4) and score.dtype == desc.dtype == torch.float32
    s, d = score[0, 0].cpu().numpy(), desc[0].cpu().numpy()
    sure = gold[tag + ".margin"] >= MARGIN
    assert float((~sure).mean()) <= 0.01
    r_s, r_d = float(gold[tag + ".ref_err_score"]), float(gold[tag + ".ref_err_desc"])
    e_s = float(np.abs(s.astype(np.float64) - gold[tag + ".score"])[sure].max())
    dd = d if (H, W) != (480, 640) else d[:, ::4, ::4]
    e_d = float(np.abs(dd.astype(np.float64) - gold[tag + ".desc"]).max())
    norm = np.sqrt((d.astype(np.float64) ** 2).sum(0))
    fp32 = os.environ.get("KPB_FP32_MATRIX") == "1"
    M = M_FP32 if fp32 else M_H16
    print("sfd2 %s %s: max |error| score %.4g desc %.4g; ref_err %.4g / %.4g: ratios %.3f / %.3f, M = %d; %d of %d pixels unsure"
          % (tag, "fp32" if fp32 else "split-f16", e_s, e_d, r_s, r_d, e_s / r_s, e_d / r_d, M, int((~sure).sum()), H * W))
    assert np.isfinite(s).all() and float(s.min()) >= 0.0 and np.isfinite(d).all()
    assert float(np.abs(norm - 1.0).max()) <= 1e-5
    assert e_s <= M * r_s, "the score is off: %.4g > %d x %.4g" % (e_s, M, r_s)
    assert e_d <= M * r_d, "the descriptors are off: %.4g > %d x %.4g" % (e_d, M, r_d)


# ------------------------------------------------------------------------------------------------ 2. batch equals solo
def test_sfd2_batch_equals_solo_bit_for_bit(net):
    H, W = 40, 56
    x = _t(np.stack([synthetic.image_pair(500 + i, H, W)[i & 1] for i in range(3)]))
    s, d = net(x)
    s, d = s.clone(), d.clone()
    assert net.dim == 128 and net.desc_div == 4
    s2, d2 = net(x)
    assert torch.equal(s, s2) and torch.equal(d, d2)
    for i in range(3):                          # alone: a pixel's bits depend on neither tile nor batch
        si, di = net(x[i:i + 1].contiguous())
        assert torch.equal(si[0], s[i]), "score of image %d: max |d| = %g" % (i, (si[0] - s[i]).abs().max().item())
        assert torch.equal(di[0], d[i]), "descriptors of image %d: max |d| = %g" % (i, (di[0] - d[i]).abs().max().item())
    assert not torch.equal(s[0], s[2])          # (different images)
    print("sfd2 bits 40x56 %s: %s" % ("fp32" if os.environ.get("KPB_FP32_MATRIX") == "1" else "split-f16", _digest(s, d)))


# ------------------------------------------------------------------------------------------------ 3. strict fp32
@pytest.mark.timeout(300)
def test_sfd2_strict_fp32_kernels_pass_the_goldens():
    """KPB_FP32_MATRIX is read once per process: tests 1, 2 and 4 again in a fresh CHILD python (subprocess.run, never an exec of this process)."""
    env = dict(os.environ, KPB_FP32_MATRIX="1")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_sfd2.py::test_sfd2_against_reference_golden", "tests/test_gpu_sfd2.py::test_sfd2_batch_equals_solo_bit_for_bit",
           "tests/test_gpu_sfd2.py::test_groups_do_not_leak"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=250)
    tail = "\n".join(p.stdout.splitlines()[-30:])
    print(tail)
    assert p.returncode == 0, "child pytest with KPB_FP32_MATRIX=1 failed:\n%s" % tail
    assert "9 passed" in tail and "skipped" not in tail.split("passed")[-1], tail
    assert tail.count(" fp32: ") == 6, tail     # five goldens and the batch test, all under the knob
    # the child really ran other kernels: its maps of the batch test's input are not this process's split-f16 maps, bit for bit
    theirs = tail.split("sfd2 bits 40x56 fp32: ")[1].split()[0]
    x = _t(np.stack([synthetic.image_pair(500 + i, 40, 56)[i & 1] for i in range(3)]))
    s, d = _net()(x)
    mine = _digest(s, d)
    print("sfd2 bits 40x56: split-f16 %s, strict fp32 %s" % (mine, theirs))
    assert len(theirs) == 16 and theirs != mine


# ------------------------------------------------------------------------------------------------ 4. the grouped layer alone
@pytest.mark.parametrize("group", [0, 13, 31])
def test_groups_do_not_leak(group):
    """KPB_OPT_SFD2_PROBE hands out the output of conv4.0's grouped 3 x 3 (+ folded BatchNorm + ReLU).  With random weights in ONE group and zero in the 31 others,
    every channel outside that group must be ReLU(bias) exactly, at every pixel -- borders and tile seams included (18 x 26 at 1/4: two tile rows, two tile columns)."""
    from keypoint_bench_amd.models.sfd2 import ResSegNetV2
    H, W = 72, 104
    sd = {k: v.clone() for k, v in state_dict().items()}
    w = sd["conv4.0.conv2.weight"]
    keep = w[8 * group:8 * group + 8].clone()
    w.zero_()
    w[8 * group:8 * group + 8] = keep
    t = weights.fold_sfd2(sd)
    net = ResSegNetV2(outdim=128, require_stability=True)
    net.load_packed(weights.pack(t, weights.ARCH_SFD2))
    x = _t(synthetic.image_pair(3, H, W)[0])[None]
    ctx = Context.get(torch.device(DEV))
    halves = []
    try:
        for half in (1, 2):
            ctx.set_option(ctx.OPT_SFD2_PROBE, half)
            _, d = net(x)
            halves.append(d[0].clone())
    finally:
        ctx.set_option(ctx.OPT_SFD2_PROBE, 0)
    out = torch.cat(halves, 0).cpu().numpy()            # [256, H/4, W/4]
    assert out.shape == (256, H // 4, W // 4)
    bias = np.maximum(t["res0.c2.b"], 0.0)
    inside = np.zeros(256, bool)
    inside[8 * group:8 * group + 8] = True
    want = np.broadcast_to(bias[:, None, None], out.shape)
    assert np.array_equal(_bits(out[~inside]), _bits(np.ascontiguousarray(want[~inside]))), "channels outside group %d are not ReLU(bias)" % group
    live = out[inside]
    assert np.isfinite(live).all() and float(live.std()) > 1e-3 and not np.array_equal(live, want[inside])      # the group itself computes something
    with pytest.raises(KpbError):
        ctx.set_option(ctx.OPT_SFD2_PROBE, 3)
    s, d = net(x)                                       # the hook is off again: a whole forward
    assert float(np.abs(np.sqrt((d[0].cpu().numpy().astype(np.float64) ** 2).sum(0)) - 1.0).max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ 5. detection
@pytest.mark.parametrize("H,W", DETECT_SHAPES)
@pytest.mark.parametrize("nms_dist,top_k", DETECT_CASES)
def test_detection_on_the_device_map_finds_the_reference_keypoints(net, H, W, nms_dist, top_k):
    from keypoint_bench_amd.utils.extracter import detection
    want = load_parts("sfd2_detect")["%dx%d.nd%d.k%d" % (H, W, nms_dist, top_k)]
    score, _ = net(_t(synthetic.image_pair(0, H, W)[0])[None])
    kps = detection(score, detect_params(nms_dist, top_k)).cpu().numpy()
    a, b = _pixels(kps, H, W), _pixels(want, H, W)
    diff = len(a ^ b)
    print("sfd2 detect %dx%d nms_dist %d top_k %d: %d keypoints (reference %d), symmetric difference %d" % (H, W, nms_dist, top_k, len(a), len(b), diff))
    assert len(b) == want.shape[0] and len(a) == kps.shape[0]
    assert 100 * diff <= DETECT_CAP_PERCENT * len(b)


@pytest.mark.parametrize("H,W", DETECT_SHAPES)
@pytest.mark.parametrize("nms_dist,top_k", DETECT_CASES)
def test_detection_on_the_reference_map_equals_the_reference_keypoints(H, W, nms_dist, top_k):
    from keypoint_bench_amd.utils.extracter import detection
    det = load_parts("sfd2_detect")
    want = det["%dx%d.nd%d.k%d" % (H, W, nms_dist, top_k)]
    kps = detection(_t(det["%dx%d.score" % (H, W)])[None, None], detect_params(nms_dist, top_k)).cpu().numpy()
    assert kps.shape == want.shape and kps.dtype == want.dtype == np.float32
    rows = lambda k: sorted(map(tuple, _bits(k).tolist()))
    assert rows(kps) == rows(want)
    if want.shape[0] == top_k:                  # cut by top_k: the reference's descending order too
        assert np.array_equal(_bits(kps), _bits(want))


# ------------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("H,W", [(12, 16), (16, 12)])
def test_a_shape_that_is_no_multiple_of_8_is_refused_and_the_net_stays_usable(net, H, W):
    x = _t(synthetic.image_pair(0, 32, 64)[0])[None]
    s, d = net(x)
    s, d = s.clone(), d.clone()
    bad = _t(synthetic.image_pair(0, H, W)[0])[None]
    score = torch.full((1, 1, H, W), 7.0, device=DEV)
    desc = torch.full((1, H // 4, W // 4, 128), 7.0, device=DEV)
    ctx = net._ctx
    rc = ctx.lib.kpb_net_forward(net._handle, ptr(bad), 1, H, W, ptr(score), ptr(desc))
    assert rc == KPB_E_INVALID
    msg = ctx.lib.kpb_last_error(ctx.handle).decode()
    assert "SFD2" in msg and "%dx%d" % (H, W) in msg, msg
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
    assert "SFD2" in msg and "desc_out_dev" in msg, msg
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
    from keynet_fixtures import checkpoint as keynet_checkpoint
    S, A, K = weights.ARCH_SFD2, weights.ARCH_ALIKE, weights.ARCH_KEYNET
    t = weights.fold_sfd2(state_dict())
    x = _t(synthetic.image_pair(0, 32, 64)[0])[None]
    s, d = net(x)
    s, d = s.clone(), d.clone()
    whole = len(weights.pack(t, S))
    for cut in (8, 100, whole // 2, whole - 4):
        rc, msg, made = _create(S, t, cut=cut)
        assert rc == KPB_E_WEIGHTS and not made and "malformed" in msg, (cut, msg)
    for name in ("conv1a.w", "conv2b.b", "res0.c2.w", "res2.c3.b", "convPa3.w", "convPb.b", "convDb.w", "sta.w", "sta.b"):
        rc, msg, made = _create(S, {k: v for k, v in t.items() if k != name})
        assert rc == KPB_E_WEIGHTS and not made and name in msg and "SFD2" in msg, msg
    for name, wrong in (("conv1a.w", t["conv1a.w"][:, :1]), ("res1.c2.w", np.zeros((256, 256, 3, 3), np.float32)), ("res0.c1.w", t["res0.c1.w"][:, :, 0, 0]),
                        ("convPb.w", t["convPb.w"][:64]), ("convDb.b", t["convDb.b"][:64]), ("sta.w", t["sta.w"][:2])):
        rc, msg, made = _create(S, dict(t, **{name: wrong}))
        assert rc == KPB_E_WEIGHTS and not made and name in msg and "SFD2" in msg, msg
    alike, key = weights.load_alike_t(), weights.fold_keynet(keynet_checkpoint())
    for arch, tensors, names in ((S, alike, ("conv1a.w", "SFD2")), (S, key, ("conv1a.w", "SFD2")), (A, t, ("b1c1.w",)), (K, t, ("KeyNet",))):
        rc, msg, made = _create(arch, tensors)
        assert rc == KPB_E_WEIGHTS and not made and all(n in msg for n in names), (arch, msg)
    for blob_arch, arch, tensors in ((A, S, alike), (S, A, t), (S, K, t), (K, S, key)):       # a blob under another net's arch id
        rc, msg, made = _create(arch, tensors, blob_arch)
        assert rc == KPB_E_WEIGHTS and not made, (blob_arch, arch, msg)
    rc, msg, made = _create(S, t)               # the intact one is created on the same context
    assert rc == 0 and made, msg
    s2, d2 = net(x)
    assert torch.equal(s2, s) and torch.equal(d2, d)


# ------------------------------------------------------------------------------------------------ 7. pipelines
def test_pair_pipeline_with_matching_equals_the_single_pair_path():
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import match_descriptors, sample_descriptors
    B, H, W = 2, 96, 128
    v = [synthetic.image_pair(20 + i, H, W) for i in range(B)]
    i0, i1 = np.stack([a for a, _ in v]), np.stack([b for _, b in v])
    net = _net()
    assert net.dense_descriptors is True        # SFD2 always writes its map: there is no keypoint-only path to run as well
    pipe = PairPipeline(net, EP, BF, B, H, W, device=DEV)
    assert pipe.div == 4 and pipe.C == 128 and (pipe.Hd, pipe.Wd) == (H // 4, W // 4) and pipe.desc.shape == (2 * B, H // 4, W // 4, 128)
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
        assert f0.shape == (k0.shape[0], 128)
        np.testing.assert_array_equal(_bits(got["kps0"]), _bits(k0.cpu().numpy()))
        np.testing.assert_array_equal(_bits(got["kps1"]), _bits(k1.cpu().numpy()))
        np.testing.assert_array_equal(_bits(pipe.sdesc[b, :k0.shape[0]].cpu().numpy()), _bits(f0.cpu().numpy()))        # sampled from the 1/4-resolution map
        np.testing.assert_array_equal(_bits(pipe.sdesc[B + b, :k1.shape[0]].cpu().numpy()), _bits(f1.cpu().numpy()))
        pairs, dist = match_descriptors(f0, f1, max_distance=5, cross_check=True, return_distance=True)
        np.testing.assert_array_equal(got["pairs"], pairs.cpu().numpy())
        np.testing.assert_array_equal(_bits(got["dist"]), _bits(dist.cpu().numpy()))
        most = max(most, got["pairs"].shape[0])
    assert most > 5
    # SequencePipeline on the same net: pair 1 of a two-frame chunk is (frame 0, frame 1), matched from the same 1/4-resolution maps
    from keypoint_bench_amd.pipeline import SequencePipeline
    seq = SequencePipeline(_net(), EP, BF, 2, H, W, device=DEV)
    assert seq.div == 4 and seq.desc.shape == (2, H // 4, W // 4, 128)
    seq.run(_t(np.stack([i0[0], i1[0]])), first=True)
    want = pipe.pair(0)
    k = int(seq.k[1])
    np.testing.assert_array_equal(_bits(seq.kps[1, :int(seq.n[1])].cpu().numpy()), _bits(want["kps0"]))
    np.testing.assert_array_equal(_bits(seq.kps[2, :int(seq.n[2])].cpu().numpy()), _bits(want["kps1"]))
    np.testing.assert_array_equal(seq.pairs[1, :k].cpu().numpy(), want["pairs"])
    np.testing.assert_array_equal(_bits(seq.dist[1, :k].cpu().numpy()), _bits(want["dist"]))


@pytest.mark.parametrize("task", ["repeatability", "MHA"])
def test_runner_rows_batched_equal_single(tmp_path, task):
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.models.sfd2 import ResSegNetV2
    path = str(tmp_path / "sfd2.pth")
    torch.save({"model": state_dict()}, path)
    H, W = 96, 128
    ds = []
    for i in range(3):
        v0, v1, hm = synthetic.warped_pair(1 + i, H, W, strength=1.0)
        ds.append({"image0": v0, "image1": v1, "dataset": "HPatches", "warp01_params": _homo(hm, H, W),
                   "warp10_params": _homo(np.linalg.inv(hm).astype(np.float32), H, W)})
    prm = {"model_type": "sfd2", "task_type": task, "sfd2_params": dict(weight=path), "extractor_params": EP,
           "matcher_params": {"type": "brute_force", "brute_force_params": BF}, "repeatability_params": {"th": 3}, "MHA_params": {"th": [3, 5, 7]}}
    single = runner.PairRunner(prm, device=DEV, batch=1)
    assert isinstance(single.model, ResSegNetV2) and single.model.dim == 128 and single.model.desc_div == 4
    _, rows1 = single.run(ds)
    assert single.batched_pairs == 0
    batched = runner.PairRunner(prm, device=DEV, batch=4)
    agg, rowsb = batched.run(ds)
    assert batched.batched_pairs == 3
    assert np.array_equal(rows1.view(np.uint64), rowsb.view(np.uint64)), (rows1, rowsb)
    print("runner %s rows: %s" % (task, rowsb[:, :4].tolist()))
    if task == "repeatability":
        assert rowsb[:, 0].min() > 20 and np.isfinite(agg["repeatability"])
    else:
        assert len(agg["MHA"]) == 3 and all(np.isfinite(a) for a in agg["MHA"])
