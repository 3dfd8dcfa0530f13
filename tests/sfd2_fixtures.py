"""The SFD2 fixtures of tests/golden/make_golden_sfd2.py: the shapes of sfd2*.npz, the seeded stand-in state dict, the detection cases, the net restated as a
few lines of torch.nn.functional over the folded tensors (for the test that needs no GPU), and the tolerance multipliers the GPU test holds the kernels to."""
import numpy as np

from r2d2_fixtures import load_parts  # noqa: F401  (stem-generic: load_parts("sfd2"), load_parts("sfd2_detect"))

SEED = 17                       # weights.random_sfd2_state_dict(SEED): the first seed from 11 on that passes all five conditions of the generator (11 .. 16 lack a
                                # stability class at 16 x 24)
# 8 x 8: one cell, out4 2 x 2; 16 x 24; 40 x 56: odd cell counts; 72 x 104: 18 x 26 at 1/4 -- a 16-row tile plus two rows; 480 x 640: the benchmark's shape
SHAPES = ((8, 8), (16, 24), (40, 56), (72, 104), (480, 640))
CPU_SHAPES = SHAPES[:3]
DETECT_SHAPES = ((96, 160), (40, 56))
# (nms_dist, top_k) of every detection case; border_dist 8, threshold 0, min_score 0
DETECT_CASES = ((2, 5000), (4, 5000), (2, 100))
DETECT_CAP_PERCENT = 2          # the device map's keypoints may differ from the reference's by at most this share of the reference count (as a set of pixels)
MARGIN = 1e-3                   # pixels whose two largest upsampled stability logits lie closer than this (fp64) are left out of the score check (at most 1 % per shape)
M_CPU = 8                       # the folded chain on the CPU: within 8 x ref_err

# max |device - reference| <= M x ref_err per golden shape, for the score (pixels with margin >= MARGIN) and the descriptors alike (ref_err_score / ref_err_desc:
# the reference's own fp32-against-fp64 differences, stored per shape).  The multipliers are the smallest powers of two that are at least twice the largest ratio
# measured on an MI355X over the five shapes (tests/test_gpu_sfd2.py has the ratios); the strict-fp32 kernels do the reference's arithmetic in another order, so
# M_FP32 above 16 would be a defect, not a tolerance.
M_H16 = 8       # measured 2.246 (score, 40 x 56); descriptors 2.232 (72 x 104)
M_FP32 = 8      # measured 2.968 (score, 40 x 56); descriptors 2.401 (72 x 104)
assert M_FP32 <= 16


def state_dict():
    """{name: torch tensor}: the stand-in for checkpoint['model'] of the reference's weights/sfd2.pth."""
    import torch
    from keypoint_bench_amd import weights
    return {k: torch.from_numpy(np.asarray(v)) for k, v in weights.random_sfd2_state_dict(SEED).items()}


def detect_params(nms_dist, top_k):
    return dict(nms_dist=int(nms_dist), threshold=0.0, border_dist=8, top_k=int(top_k), min_score=0.0)


def chain(t, img, margin=False):
    """(score [B,1,H,W], desc [B,128,H/4,W/4]) from the folded tensors `t` (weights.fold_sfd2): sfd2.py:144-182 with every BatchNorm already in its convolution.
    margin=True: a third result [B,H,W], the difference between the two largest upsampled stability logits per pixel (MARGIN is meant for the float64 chain's)."""
    import torch
    import torch.nn.functional as F
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))

    def conv(x, name, stride=1, relu=True, groups=1):
        w = tt(t[name + ".w"])
        y = F.conv2d(x, w, tt(t[name + ".b"]), stride=stride, padding=w.shape[-1] // 2, groups=groups)
        return F.relu(y) if relu else y

    x = conv(conv(img, "conv1a"), "conv1b", stride=2)
    x = conv(conv(x, "conv2a"), "conv2b", stride=2)
    x = conv(conv(x, "conv3a"), "conv3b")
    for i in range(3):
        y = conv(conv(x, "res%d.c1" % i), "res%d.c2" % i, groups=32)
        x = F.relu(conv(y, "res%d.c3" % i, relu=False) + x)
    semi = torch.exp(conv(conv(conv(x, "convPa0", stride=2), "convPa3", relu=False), "convPb", relu=False))       # no maximum subtracted
    semi = semi / (semi.sum(1, keepdim=True) + 1e-5)
    B, _, Hc, Wc = semi.shape
    score = semi[:, :-1].permute(0, 2, 3, 1).reshape(B, Hc, Wc, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, 1, Hc * 8, Wc * 8)
    desc = F.normalize(conv(conv(conv(x, "convDa0"), "convDa3", relu=False), "convDb", relu=False), dim=1)
    logits = F.interpolate(conv(x, "sta", relu=False), size=img.shape[2:], mode="bilinear", align_corners=False)
    stab = torch.tensor([0.1, 0.5, 1.0])[logits.argmax(1, keepdim=True)]
    if margin:
        top2 = torch.topk(logits, 2, dim=1).values
        return score * stab, desc, top2[:, 0] - top2[:, 1]
    return score * stab, desc
