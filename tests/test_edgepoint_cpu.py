"""EdgePoint without a GPU: the folded tensors of the reference checkpoint, pushed through a plain torch.nn.functional chain that uses the
closed forms of the head's strided and transposed layers, reproduce the reference's own outputs (tests/golden/edgepoint*.npz, written by the
reference class).  That pins the BatchNorm folding, the tensor layouts and the closed forms the kernels of csrc/alike.hip are built on:

    score = conv_score(relu(conv1(x1)))                       raw logit, full resolution
    d1    = conv_8 (1 x 1, stride 8) == its weights on a1[..., ::8, ::8]
    d2    = conv_4 (1 x 1, stride 4) == its weights on a2[..., ::4, ::4]
    d4    = conv_transpose_4 (4 x 4, stride 4): out[:, :, y, x] = b + sum_ci a4[ci, y // 4, x // 4] w[ci, :, y % 4, x % 4]
    desc  = convhead2(cat[d1, d2, a3, d4])                    H/8 x W/8, not normalised

Tolerances: the reference's own fp32 forward differs from its fp64 forward by 2.7e-5 (score) and 7.6e-7 (descriptor) at 480 x 640; the chain
(edgepoint_fixtures.chain) is the same fp32 arithmetic with the BatchNorm division folded into the weights, so it gets five times that yardstick: 1.4e-4 / 4e-6."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from keypoint_bench_amd import synthetic, weights
from edgepoint_fixtures import PARAM, SHAPES, chain, checkpoint, load_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL_SCORE, ATOL_DESC = 1.4e-4, 4e-6


@pytest.fixture(scope="module")
def folded():
    return weights.fold_edgepoint(checkpoint())


def test_fold_pack_unpack_round_trip(folded):
    t = folded
    assert list(t)[:2] == ["b1c1.w", "b1c1.b"] and t["head.w"].shape == (64, 64)
    assert {k: t[k].shape for k in ("score.w", "score.b", "d8.w", "d8.b", "d4.w", "d4.b", "ct4.w", "ct4.b")} == {
        "score.w": (16,), "score.b": (1,), "d8.w": (16, 16), "d8.b": (16,), "d4.w": (16, 16), "d4.b": (16,), "ct4.w": (16, 16, 4, 4), "ct4.b": (16,)}
    arch, back = weights.unpack(weights.pack(t, weights.ARCH_EDGEPOINT))
    assert arch == weights.ARCH_EDGEPOINT and list(back) == list(t)
    for k in t:
        assert back[k].dtype == np.float32 and np.array_equal(back[k], t[k]), k
    # the trunk is fold_alike's, tensor for tensor
    fa = weights.fold_alike(checkpoint())
    assert all(np.array_equal(fa[k], t[k]) for k in fa) and set(t) - set(fa) == {"score.w", "score.b", "d8.w", "d8.b", "d4.w", "d4.b", "ct4.w", "ct4.b"}
    # the BatchNorm folding, on one channel by hand: block 3 conv 2, channel 5
    sd = {k: v.double().numpy() for k, v in checkpoint().items()}
    s = sd["block3.bn2.weight"][5] / np.sqrt(sd["block3.bn2.running_var"][5] + 1e-5)
    np.testing.assert_allclose(t["b3c2.w"][5], sd["block3.conv2.weight"][5] * s, rtol=1e-6)
    np.testing.assert_allclose(t["b3c2.b"][5], sd["block3.bn2.bias"][5] - sd["block3.bn2.running_mean"][5] * s, rtol=1e-6, atol=1e-9)


def test_ct4_keeps_the_state_dicts_layout(folded):
    """ct4.w is [in][out][ky][kx]: one output pixel of the transposed convolution by hand against F.conv_transpose2d."""
    sd = checkpoint()
    assert np.array_equal(folded["ct4.w"], sd["conv_transpose_4.weight"].numpy())
    a4 = torch.from_numpy(np.random.default_rng(3).random((1, 16, 2, 3)).astype(np.float32))
    ref = F.conv_transpose2d(a4, sd["conv_transpose_4.weight"], sd["conv_transpose_4.bias"], stride=4)
    assert ref.shape == (1, 16, 8, 12)
    y, x, co = 6, 9, 11
    by_hand = float(folded["ct4.b"][co]) + sum(float(a4[0, ci, y // 4, x // 4]) * float(folded["ct4.w"][ci, co, y % 4, x % 4]) for ci in range(16))
    assert abs(by_hand - float(ref[0, co, y, x])) < 1e-5
    swapped = float(folded["ct4.b"][co]) + sum(float(a4[0, ci, y // 4, x // 4]) * float(folded["ct4.w"][co, ci, y % 4, x % 4]) for ci in range(16))
    assert abs(swapped - float(ref[0, co, y, x])) > 1e-3            # [out][in] would not have passed


@pytest.mark.parametrize("H,W", SHAPES[:4])
def test_folded_chain_reproduces_the_reference_goldens(folded, H, W):
    g = load_parts("edgepoint")
    v0, _ = synthetic.image_pair(0, H, W)
    assert synthetic.checksum(v0) == str(g["%dx%d.img.sum" % (H, W)])
    with torch.no_grad():
        score, desc = chain(folded, torch.from_numpy(v0)[None])
    assert score.shape == (1, 1, H, W) and desc.shape == (1, 64, H // 8, W // 8)
    es = float(np.abs(score[0, 0].numpy() - g["%dx%d.score" % (H, W)]).max())
    ed = float(np.abs(desc[0].permute(1, 2, 0).numpy() - g["%dx%d.desc" % (H, W)]).max())
    print("edgepoint folded chain %dx%d: max |score error| %.3g, max |desc error| %.3g" % (H, W, es, ed))
    assert es <= ATOL_SCORE and ed <= ATOL_DESC


def test_misshaped_missing_and_foreign_state_dicts_are_refused():
    sd = checkpoint()
    bad = dict(sd)
    bad["conv_transpose_4.weight"] = bad["conv_transpose_4.weight"][:, :, :3, :3]
    with pytest.raises(ValueError, match="conv_transpose_4.weight"):
        weights.fold_edgepoint(bad)
    with pytest.raises(ValueError, match="conv_8.bias"):
        weights.fold_edgepoint({k: v for k, v in sd.items() if k != "conv_8.bias"})
    with pytest.raises(ValueError, match="block3.bn1.running_var"):
        weights.fold_edgepoint({k: v for k, v in sd.items() if k != "block3.bn1.running_var"})
    foreign = dict(sd)                  # another plan: c1 = 32
    foreign["block1.conv1.weight"] = torch.zeros(32, 3, 3, 3)
    with pytest.raises(ValueError, match="block1.conv1.weight"):
        weights.fold_edgepoint(foreign)
    alike = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(ROOT, "tests", "golden", "alike_t_state_dict.npz")).items()}
    with pytest.raises(ValueError, match="convhead2.weight|conv_score.weight"):       # ALIKE-t's state_dict: a 65-row head, no score layer
        weights.fold_edgepoint(alike)


def test_model_class_contract():
    from keypoint_bench_amd.models.EdgePoint import EdgePoint
    from keypoint_bench_amd.models._base import HipNet
    assert EdgePoint.signed_scores is True and HipNet.signed_scores is False and EdgePoint.ARCH == weights.ARCH_EDGEPOINT
    with pytest.raises(NotImplementedError):
        EdgePoint(None)                 # the reference's default plan, 32/64/128/128/128
    with pytest.raises(NotImplementedError):
        EdgePoint(dict(PARAM, c1=32))
    with pytest.raises(NotImplementedError):
        EdgePoint(PARAM, trainable=True)
    net = EdgePoint(dict(PARAM, weight="weights/EdgePoint.pt"))         # EdgePoint_params of the configs carry the path too
    assert net.load_state_dict(checkpoint()) == "<All keys matched successfully>"           # (no device is touched before the first forward)
    assert net.dim == 64 and net.desc_div == 8 and net.eval() is net
    assert weights.unpack(net._blob)[0] == weights.ARCH_EDGEPOINT


def test_runner_refuses_a_missing_checkpoint_file_and_lists_the_type():
    from keypoint_bench_amd import runner
    with pytest.raises(FileNotFoundError):
        runner.build_model({"model_type": "EdgePoint", "EdgePoint_params": dict(PARAM, weight="/nonexistent/EdgePoint.pt")})
    with pytest.raises(NotImplementedError, match="EdgePoint"):
        runner.build_model({"model_type": "Harris"})


def test_header_and_python_agree_on_the_arch_id():
    text = open(os.path.join(ROOT, "include", "kpb.h")).read()
    m = re.search(r"#define\s+KPB_ARCH_EDGEPOINT\s+(\d+)", text)
    assert m and int(m.group(1)) == weights.ARCH_EDGEPOINT == 7


@pytest.mark.parametrize("H,W", SHAPES)
def test_premise_the_score_map_is_mostly_negative(H, W):
    """Why this net needs signed detection: at least three pixels in four of every golden score map are negative (measured 0.79-0.86), and the
    reference's detection on the map and on the map clamped at zero -- what a non-negative contract could serve -- both return rows."""
    import oracle
    s = load_parts("edgepoint")["%dx%d.score" % (H, W)]
    assert (s < 0).mean() >= 0.75 and s.max() > 0
    ep = dict(nms_dist=2, threshold=0.0, border_dist=4, top_k=1000, min_score=0.0)
    raw, _ = oracle.detection(s, ep)
    clamped, _ = oracle.detection(np.maximum(s, 0), ep)
    assert raw.shape[0] > 0 and clamped.shape[0] > 0 and raw.shape[1] == 3
