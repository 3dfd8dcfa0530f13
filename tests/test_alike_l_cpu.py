"""ALIKE-l (the reference's default ALNet(): c1..c4 = 32, 64, 128, 128, dim = 128) without a GPU.

1. The drop-in class accepts exactly two plans -- ALIKE-t (8, 16, 32, 64, 64) and ALIKE-l, `param=None` included -- reports the plan's dim and refuses every
   other plan (ALIKE-n, ALIKE-s, an arbitrary one) with a NotImplementedError whose text names both.
2. weights.fold_alike of the fixture state dict (tests/golden/alike_l_state_dict*.npz: seeded stand-in weights with non-trivial BatchNorm statistics), pushed
   through oracle.alike_ref.alnet_forward, reproduces the outputs the REFERENCE class wrote (tests/golden/alike_l*.npz) at all five shapes within the bars the
   GPU tests hold the kernels to: score 7e-6, descriptors 1e-4 x max(1, max |desc_ref|).  That ties the fold, the oracle and the reference together.
3. The runner builds the default plan from Alike_params and refuses to put the packaged ALIKE-t checkpoint into it.
"""
import os
import re

import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic, weights
from alike_l_fixtures import FULL_DESC, PARAM, SCORE_ATOL, SHAPES, desc_bar, desc_of, load_parts, state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def folded():
    return weights.fold_alike(state_dict())


def test_default_and_l_plan_construct_with_dim_128():
    from keypoint_bench_amd.models.ALike import ALNet
    for net in (ALNet(), ALNet(None), ALNet(dict(PARAM)), ALNet(dict(PARAM, weight="weights/alike-l.pth")), ALNet(dense_descriptors=False)):
        assert net.dim == 128 and net.desc_div == 1 and net.param == PARAM and net.ARCH == weights.ARCH_ALIKE
    t = ALNet({"c1": 8, "c2": 16, "c3": 32, "c4": 64, "dim": 64})
    assert t.dim == 64 and t.desc_div == 1


@pytest.mark.parametrize("plan", [(16, 32, 64, 128, 128), (8, 16, 48, 96, 96), (32, 64, 128, 128, 64), (8, 16, 32, 64, 128), (24, 40, 56, 72, 88)],
                         ids=["alike-n", "alike-s", "l-trunk-dim-64", "t-trunk-dim-128", "arbitrary"])
def test_every_other_plan_is_refused_and_the_message_names_both(plan):
    from keypoint_bench_amd.models.ALike import ALNet
    with pytest.raises(NotImplementedError) as e:
        ALNet(dict(zip(("c1", "c2", "c3", "c4", "dim"), plan)))
    assert "8,16,32,64, dim = 64" in str(e.value) and "32,64,128,128, dim = 128" in str(e.value)


def test_fold_is_plan_agnostic_and_round_trips(folded):
    t = folded
    assert list(t)[:2] == ["b1c1.w", "b1c1.b"]
    want = {"b1c1.w": (32, 3, 3, 3), "b1c2.w": (32, 32, 3, 3), "b2c1.w": (64, 32, 3, 3), "b2c2.w": (64, 64, 3, 3), "b2ds.w": (64, 32), "b2ds.b": (64,),
            "b3c1.w": (128, 64, 3, 3), "b3c2.w": (128, 128, 3, 3), "b3ds.w": (128, 64), "b4c1.w": (128, 128, 3, 3), "b4c2.w": (128, 128, 3, 3), "b4ds.w": (128, 128),
            "agg1.w": (32, 32), "agg2.w": (32, 64), "agg3.w": (32, 128), "agg4.w": (32, 128), "head.w": (129, 128)}
    assert {k: t[k].shape for k in want} == want
    arch, back = weights.unpack(weights.pack(t, weights.ARCH_ALIKE))
    assert arch == weights.ARCH_ALIKE and list(back) == list(t)
    assert all(back[k].dtype == np.float32 and np.array_equal(back[k], t[k]) for k in t)
    # the BatchNorm folding, on one channel by hand -- and the statistics are not the trivial ones a fresh BatchNorm has
    sd = {k: v.double().numpy() for k, v in state_dict().items()}
    assert sd["block4.bn2.running_var"].std() > 0.1 and np.abs(sd["block4.bn2.running_mean"]).max() > 0.1 and np.abs(sd["block4.bn2.bias"]).max() > 0.3
    s = sd["block4.bn2.weight"][77] / np.sqrt(sd["block4.bn2.running_var"][77] + 1e-5)
    np.testing.assert_allclose(t["b4c2.w"][77], sd["block4.conv2.weight"][77] * s, rtol=1e-6)
    np.testing.assert_allclose(t["b4c2.b"][77], sd["block4.bn2.bias"][77] - sd["block4.bn2.running_mean"][77] * s, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("H,W", SHAPES)
def test_fold_and_oracle_reproduce_the_reference_fixtures(folded, H, W):
    from oracle.alike_ref import alnet_forward
    g = load_parts("alike_l")
    v0, _ = synthetic.image_pair(0, H, W)
    assert synthetic.checksum(v0) == str(g["%dx%d.img.sum" % (H, W)])
    with torch.no_grad():
        score, desc = alnet_forward(torch.from_numpy(v0)[None], {k: torch.from_numpy(v) for k, v in folded.items()})
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 128, H, W)
    ref_s, ref_d = g["%dx%d.score" % (H, W)], g["%dx%d.desc" % (H, W)]
    assert ref_d.shape == ((H, W, 128) if SHAPES.index((H, W)) < FULL_DESC else ((H + 7) // 8, (W + 7) // 8, 128))
    es = float(np.abs(score[0, 0].numpy() - ref_s).max())
    ed = float(np.abs(desc_of(g, (H, W), desc[0].permute(1, 2, 0).numpy()) - ref_d).max())
    print("alike_l fold + oracle %dx%d: max |score error| %.3g (bar %.3g), max |desc error| %.3g (bar %.3g), max |desc| %.3g"
          % (H, W, es, SCORE_ATOL, ed, desc_bar(ref_d), float(np.abs(ref_d).max())))
    assert es <= SCORE_ATOL and ed <= desc_bar(ref_d)


@pytest.mark.parametrize("H,W", SHAPES)
def test_fixture_scores_are_not_saturated_and_descriptors_are_of_order_one(H, W):
    g = load_parts("alike_l")
    s, d = g["%dx%d.score" % (H, W)], g["%dx%d.desc" % (H, W)]
    assert ((s < 1e-3) | (s > 1 - 1e-3)).mean() == 0.0 and s.max() - s.min() > 0.1
    assert 1.0 <= np.abs(d).max() <= 10.0


def test_load_state_dict_checks_the_plan():
    from keypoint_bench_amd.models.ALike import ALNet
    net = ALNet()
    assert net.load_state_dict(state_dict()) == "<All keys matched successfully>"       # (no device is touched before the first forward)
    arch, t = weights.unpack(net._blob)
    assert arch == weights.ARCH_ALIKE and t["head.w"].shape == (129, 128)
    with pytest.raises(ValueError, match="b1c1.w"):
        ALNet({"c1": 8, "c2": 16, "c3": 32, "c4": 64, "dim": 64}).load_state_dict(state_dict())
    alike_t = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(ROOT, "tests", "golden", "alike_t_state_dict.npz")).items()}
    with pytest.raises(ValueError, match="b1c1.w"):
        ALNet().load_state_dict(alike_t)


def test_runner_builds_the_default_plan_and_wants_its_checkpoint(tmp_path):
    from keypoint_bench_amd import runner
    from keypoint_bench_amd.models.ALike import ALNet
    path = str(tmp_path / "alike-l.pth")
    torch.save(state_dict(), path)
    for p in (dict(PARAM, weight=path), {"weight": path}):         # Alike_params with the -l plan, and without plan keys: the reference's ALNet(None)
        net = runner.build_model({"model_type": "Alike", "Alike_params": p})
        assert isinstance(net, ALNet) and net.dim == 128 and weights.unpack(net._blob)[1]["head.w"].shape == (129, 128)
    with pytest.raises(FileNotFoundError, match="ALIKE-l"):         # the packaged checkpoint is ALIKE-t's
        runner.build_model({"model_type": "Alike", "Alike_params": dict(PARAM, weight="/nonexistent/alike-l.pth")})
    t = runner.build_model({"model_type": "Alike", "Alike_params": {"c1": 8, "c2": 16, "c3": 32, "c4": 64, "dim": 64, "weight": "/nonexistent/alike-t.pth"}})
    assert t.dim == 64          # ALIKE-t still falls back on the packaged checkpoint


def test_header_names_both_plans():
    text = open(os.path.join(ROOT, "include", "kpb.h")).read()
    m = re.search(r"#define\s+KPB_ARCH_ALIKE\s+(\d+)(.*)", text)
    assert m and int(m.group(1)) == weights.ARCH_ALIKE == 1
    assert "ALIKE-t" in text and "ALIKE-l" in text
