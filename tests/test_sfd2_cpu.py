"""SFD2 without a GPU: the fixtures are whole, the folded tensors of the seeded stand-in pushed through a plain torch.nn.functional chain
(sfd2_fixtures.chain: conv2d with groups=32 for the ResBlocks' 3 x 3, the head as the reference states it) reproduce the reference class's own score and
descriptor maps (tests/golden/sfd2*.npz), and the Python surface keeps its contract.  That pins the BatchNorm folding (affine and not, with and without a
convolution bias), the tensor names and layouts csrc/sfd2.hip reads, and the head's order of operations.

Tolerance of the chain: 8 x ref_err per shape on the pixels whose stability class is sure (margin >= 1e-3), ref_err being the reference's own
max |fp32 - float64| stored with each golden.  The chain is the same fp32 arithmetic in torch with the BatchNorm folded in float64."""
import os
import re

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights
from sfd2_fixtures import (CPU_SHAPES, DETECT_CASES, DETECT_SHAPES, M_CPU, M_FP32, M_H16, MARGIN, SEED, SHAPES, chain, load_parts, state_dict)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def folded():
    return weights.fold_sfd2(state_dict())


def test_fixtures_are_intact(folded):
    g = load_parts("sfd2")
    wsum = synthetic.checksum(np.concatenate([np.asarray(v, np.float32).ravel() for k, v in sorted(folded.items())]))
    for H, W in SHAPES:
        tag = "%dx%d" % (H, W)
        assert synthetic.checksum(synthetic.image_pair(0, H, W)[0]) == str(g[tag + ".img.sum"])
        assert wsum == str(g[tag + ".w.sum"]), "the goldens were made from other weights than random_sfd2_state_dict(%d)" % SEED
        s, d, m, c = g[tag + ".score"], g[tag + ".desc"], g[tag + ".margin"], g[tag + ".cls"]
        assert s.shape == m.shape == c.shape == (H, W) and s.dtype == m.dtype == np.float32 and c.dtype == np.uint8
        assert d.shape == ((128, H // 4, W // 4) if (H, W) != (480, 640) else (128, 30, 40)) and d.dtype == np.float32
        assert np.isfinite(s).all() and float(s.min()) >= 0.0 and float(s.max()) < 1.0
        assert float((m < MARGIN).mean()) <= 0.01                           # condition (b) of the generator
        if (H, W) != (8, 8):
            assert set(np.unique(c).tolist()) == {0, 1, 2}                  # condition (c)
        assert 1e-10 < float(g[tag + ".ref_err_score"]) < 1e-4 and 1e-8 < float(g[tag + ".ref_err_desc"]) < 1e-5
    d = load_parts("sfd2_detect")
    assert sorted(d) == sorted(["%dx%d.nd%d.k%d" % (H, W, nd, k) for H, W in DETECT_SHAPES for nd, k in DETECT_CASES] + ["%dx%d.score" % s for s in DETECT_SHAPES])
    for key, kps in d.items():
        if key.endswith(".score"):
            continue
        k = int(key.rsplit(".k", 1)[1])
        assert kps.ndim == 2 and kps.shape[1] == 3 and 10 < kps.shape[0] <= k and kps.dtype == np.float32
    assert M_FP32 <= 16 and M_H16 & (M_H16 - 1) == 0 and M_FP32 & (M_FP32 - 1) == 0


def test_fold_pack_unpack_round_trip(folded):
    t = folded
    names = ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b"] + ["res%d.c%d" % (i, j) for i in range(3) for j in (1, 2, 3)] + [
        "convPa0", "convPa3", "convPb", "convDa0", "convDa3", "convDb", "sta"]
    assert list(t) == [n + s for n in names for s in (".w", ".b")]
    assert t["conv1a.w"].shape == (64, 3, 3, 3) and t["res1.c2.w"].shape == (256, 8, 3, 3) and t["res2.c3.w"].shape == (256, 256, 1, 1)
    assert t["convPb.w"].shape == (65, 256, 1, 1) and t["convDb.w"].shape == (128, 256, 1, 1) and t["sta.w"].shape == (3, 256, 1, 1) and t["sta.b"].shape == (3,)
    arch, back = weights.unpack(weights.pack(t, weights.ARCH_SFD2))
    assert arch == weights.ARCH_SFD2 and list(back) == list(t)
    for k in t:
        assert back[k].dtype == np.float32 and back[k].shape == t[k].shape and np.array_equal(back[k], t[k]), k
    sd = {k: v.double().numpy() for k, v in state_dict().items()}
    # BatchNorm(affine=False) behind a convolution with a bias, on one channel by hand
    s = 1.0 / np.sqrt(sd["bn1b.0.running_var"][5] + 1e-5)
    np.testing.assert_allclose(t["conv1b.w"][5], sd["conv1b.0.weight"][5] * s, rtol=1e-6)
    np.testing.assert_allclose(t["conv1b.b"][5], (sd["conv1b.0.bias"][5] - sd["bn1b.0.running_mean"][5]) * s, rtol=1e-6, atol=1e-9)
    # affine BatchNorm behind the bias-free grouped convolution
    s = sd["conv4.1.bn2.weight"][77] / np.sqrt(sd["conv4.1.bn2.running_var"][77] + 1e-5)
    np.testing.assert_allclose(t["res1.c2.w"][77], sd["conv4.1.conv2.weight"][77] * s, rtol=1e-6)
    np.testing.assert_allclose(t["res1.c2.b"][77], sd["conv4.1.bn2.bias"][77] - sd["conv4.1.bn2.running_mean"][77] * s, rtol=1e-6, atol=1e-9)
    # affine BatchNorm behind a convolution with a bias
    s = sd["convDa.1.weight"][3] / np.sqrt(sd["convDa.1.running_var"][3] + 1e-5)
    np.testing.assert_allclose(t["convDa0.b"][3], (sd["convDa.0.bias"][3] - sd["convDa.1.running_mean"][3]) * s + sd["convDa.1.bias"][3], rtol=1e-6, atol=1e-9)
    assert np.array_equal(t["convPb.w"], state_dict()["convPb.weight"].numpy()) and np.array_equal(t["sta.b"], state_dict()["ConvSta.bias"].numpy())


def test_random_state_dict_follows_the_recipe():
    sd = weights.random_sfd2_state_dict(SEED)
    again = weights.random_sfd2_state_dict(SEED)
    assert list(sd) == list(again) and all(np.array_equal(sd[k], again[k]) for k in sd)
    assert not np.array_equal(sd["conv1a.0.weight"], weights.random_sfd2_state_dict(SEED + 1)["conv1a.0.weight"])
    w = sd["conv3b.0.weight"]
    assert abs(float(w.std()) / np.sqrt(2.0 / (256 * 9)) - 1.0) < 0.02 and abs(float(sd["conv4.0.conv2.weight"].std()) / np.sqrt(2.0 / 72) - 1.0) < 0.02
    assert 0.75 <= float(sd["conv4.2.bn3.weight"].min()) and float(sd["bn3b.0.running_var"].max()) <= 1.25
    assert "conv1a.1.weight" not in sd and "bn2b.0.bias" not in sd            # affine=False
    assert "conv4.0.conv1.bias" not in sd                                    # the ResBlocks' convolutions have no bias


@pytest.mark.parametrize("H,W", CPU_SHAPES)
def test_folded_chain_reproduces_the_reference_goldens(folded, H, W):
    g = load_parts("sfd2")
    tag = "%dx%d" % (H, W)
    v0, _ = synthetic.image_pair(0, H, W)
    with torch.no_grad():
        score, desc = chain(folded, torch.from_numpy(v0)[None])
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 128, H // 4, W // 4)
    sure = g[tag + ".margin"] >= MARGIN
    e_s = float(np.abs(score[0, 0].numpy().astype(np.float64) - g[tag + ".score"])[sure].max())
    e_d = float(np.abs(desc[0].numpy().astype(np.float64) - g[tag + ".desc"]).max())
    r_s, r_d = float(g[tag + ".ref_err_score"]), float(g[tag + ".ref_err_desc"])
    print("sfd2 folded chain %s: max |score error| %.3g = %.2f x ref_err, max |desc error| %.3g = %.2f x ref_err" % (tag, e_s, e_s / r_s, e_d, e_d / r_d))
    assert e_s <= M_CPU * r_s and e_d <= M_CPU * r_d


def test_misshaped_missing_and_foreign_state_dicts_are_refused():
    sd = state_dict()
    for name in ("conv1a.0.weight", "bn1b.0.running_var", "conv4.1.conv2.weight", "conv4.2.bn3.bias", "convPa.3.bias", "ConvSta.weight"):
        with pytest.raises(ValueError, match=re.escape(name)):
            weights.fold_sfd2({k: v for k, v in sd.items() if k != name})
    bad = dict(sd)
    bad["conv4.0.conv2.weight"] = torch.zeros(256, 256, 3, 3)      # not grouped
    with pytest.raises(ValueError, match="conv4.0.conv2.weight"):
        weights.fold_sfd2(bad)
    bad = dict(sd)
    bad["convDb.weight"] = torch.zeros(256, 256, 1, 1)             # outdim 256
    with pytest.raises(ValueError, match="convDb.weight"):
        weights.fold_sfd2(bad)
    with pytest.raises(ValueError, match="SFD2 state_dict"):       # the whole checkpoint instead of its 'model' entry
        weights.fold_sfd2({"model": sd})
    let = {k: torch.from_numpy(v) for k, v in load_parts("letnet_state_dict").items()}
    with pytest.raises(ValueError, match="SFD2 state_dict"):
        weights.fold_sfd2(let)
    extra = dict(sd, **{"convSeg.weight": torch.zeros(4, 256, 1, 1), "conv1a.1.num_batches_tracked": torch.tensor(7)})     # strict=False: unused keys are ignored
    t0, t1 = weights.fold_sfd2(sd), weights.fold_sfd2(extra)
    assert list(t0) == list(t1) and all(np.array_equal(t0[k], t1[k]) for k in t0)


def test_model_class_contract():
    from keypoint_bench_amd.models.sfd2 import ResSegNetV2, sfd2_random
    assert ResSegNetV2.dense_descriptors is True and ResSegNetV2.tracked_maps is False and ResSegNetV2.signed_scores is False
    assert ResSegNetV2.ARCH == weights.ARCH_SFD2 == 11
    text = open(os.path.join(ROOT, "include", "kpb.h")).read()
    m = re.search(r"#define\s+KPB_ARCH_SFD2\s+(\d+)\s+/\*(.*?)\*/", text)
    assert m and int(m.group(1)) == weights.ARCH_SFD2
    assert "multiples of 8" in m.group(2) and "dim 128" in m.group(2) and "desc_div 4" in m.group(2)
    with pytest.raises(NotImplementedError):
        ResSegNetV2(outdim=256, require_stability=True)
    with pytest.raises(NotImplementedError):
        ResSegNetV2(outdim=128)                                     # require_stability=False: the reference itself fails there
    net = ResSegNetV2(outdim=128, require_feature=False, require_stability=True, ms_detector=True)
    assert net.load_state_dict(state_dict(), strict=False) == "<All keys matched successfully>"       # (no device is touched before the first forward)
    assert net._handle is None and net._ctx is None
    assert net.dim == 128 and net.desc_div == 4 and net.eval() is net
    assert weights.unpack(net._blob)[0] == weights.ARCH_SFD2
    assert weights.unpack(sfd2_random(SEED)._blob)[1].keys() == weights.unpack(net._blob)[1].keys()
    assert np.array_equal(weights.unpack(sfd2_random(SEED)._blob)[1]["res0.c2.w"], weights.unpack(net._blob)[1]["res0.c2.w"])
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        net(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match="convPb.bias"):
        net.load_state_dict({k: v for k, v in state_dict().items() if k != "convPb.bias"}, strict=False)


def test_runner_builds_sfd2_from_the_model_entry_of_a_saved_checkpoint(tmp_path):
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.models.sfd2 import ResSegNetV2
    with pytest.raises(FileNotFoundError, match="sfd2") as e:
        runner.build_model({"model_type": "sfd2", "sfd2_params": {"weight": "/nonexistent/sfd2.pth"}})
    assert "not shipped" in str(e.value)
    with pytest.raises(NotImplementedError, match="sfd2") as e:
        runner.build_model({"model_type": "Harris"})
    assert "Harris" in str(e.value) and "KeyNet" in str(e.value)
    path = str(tmp_path / "sfd2.pth")
    torch.save({"model": state_dict(), "epoch": 3}, path)
    net = runner.build_model({"model_type": "sfd2", "sfd2_params": {"weight": path}})
    assert isinstance(net, ResSegNetV2) and net.dim == 128 and net.desc_div == 4
    want = weights.fold_sfd2(state_dict())
    got = weights.unpack(net._blob)
    assert got[0] == weights.ARCH_SFD2 and all(np.array_equal(got[1][k], want[k]) for k in want)
