"""CPU emulation of R2D2's single-f16 matrix mode (Quad_L2Net_ConfCFS(matrix="f16"), csrc/conv_mfma.h CmForm::h1), and the references it is held against.

The definition (one MFMA a_hi * b_hi per product): before each of conv1 .. conv8 both operands are rounded to f16 at a power-of-two scale -- the activations with
max |x| brought into [2^14, 2^15), the weights into [2^12, 2^13) -- as (x s).half().float() / s; the convolution of the rounded operands is evaluated in float64
and cast to fp32, bias and ReLU as always.  conv0 (vector ALU, fp32) and the head are left alone.  Rounding to f16 at a power-of-two scale does not depend on
the scale while the scaled value is a normal f16, so the per-tensor scales here and the per-workgroup, per-slab scales of the device give the same hi halves
(they can differ only around 2^-29 of a slab's maximum and below)."""
import functools

import numpy as np

from r2d2_fixtures import chain, load_parts

SMALL_SHAPES = ((64, 96), (61, 97), (24, 40))       # the golden shapes an emulation takes well under a second at


@functools.lru_cache(maxsize=None)
def folded():
    """The reference checkpoint's folded tensors (weights.fold_r2d2), fp32."""
    from keypoint_bench_amd import weights
    from r2d2_fixtures import checkpoint
    return weights.fold_r2d2(checkpoint()["state_dict"])


def round_f16(x, top):
    """x (torch fp32) rounded to f16, to nearest even, at the power-of-two scale that puts max |x| into [2^(top - 1), 2^top); all-zero stays zero."""
    import torch
    m = float(x.abs().max())
    if not m > 0.0:
        return x.clone()
    s = 2.0 ** (top - (int(np.floor(np.log2(m))) + 1))
    return ((x * s).half().float() / s).to(torch.float32)


def emulate(img, rounded=True):
    """(score [B,1,H,W], desc [B,128,H,W]) of fp32 image `img` [B,3,H,W] (numpy) by the plan table: every layer's convolution in float64 on fp32 operands, cast to fp32;
    with `rounded`, conv1 .. conv8 on operands rounded by round_f16 (activations top 15, weights top 13).  rounded=False is the same chain without the rounding."""
    import torch
    import torch.nn.functional as F
    from keypoint_bench_amd import weights
    t = folded()
    x = torch.from_numpy(np.array(img, np.float32))
    for name, cin, cout, k, dil, bn, relu in weights.R2D2_PLAN:
        w, b = torch.from_numpy(t[name + ".w"]), torch.from_numpy(t[name + ".b"])
        if rounded and name != "conv0":
            x, w = round_f16(x, 15), round_f16(w, 13)
        x = F.conv2d(x.double(), w.double(), b.double(), padding=(k - 1) * dil // 2, dilation=dil).float()
        if relu:
            x = F.relu(x)
    x = x.double()
    sq = x * x
    clf = F.conv2d(sq, torch.from_numpy(t["clf.w"]).double()[:, :, None, None], torch.from_numpy(t["clf.b"]).double())
    sal = F.softplus(F.conv2d(sq, torch.from_numpy(t["sal.w"]).double()[:, :, None, None], torch.from_numpy(t["sal.b"]).double()))
    score = sal / (1 + sal) * F.softmax(clf, dim=1)[:, 1:2]
    desc = x / torch.linalg.norm(x, dim=1, keepdim=True).clamp_min(1e-12)
    return score.float().numpy(), desc.float().numpy()


@functools.lru_cache(maxsize=None)
def case(seed, H, W):
    """One seeded image with its three maps, computed once and shared (read-only): {"img" [3,H,W], "exact": (score [H,W], desc [H,W,128]) of the float64 chain,
    "emu": the same of the emulation}."""
    import torch
    from keypoint_bench_amd import synthetic
    img = synthetic.image_pair(seed, max(H, 24), max(W, 40))[0][:, :H, :W].copy()       # (the generator's smallest scene; the golden shapes are taken whole)
    t64 = {k: v.astype(np.float64) for k, v in folded().items()}
    s, d = chain(t64, torch.from_numpy(img.astype(np.float64))[None])
    es, ed = emulate(img[None])
    out = {"img": img, "exact": (s[0, 0].numpy(), d[0].permute(1, 2, 0).numpy()), "emu": (es[0, 0], np.ascontiguousarray(ed[0].transpose(1, 2, 0)))}
    for v in out.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return out


def golden(H, W):
    """The reference's own fp32 CPU outputs at a golden shape: (score [H,W], desc [H,W,128]; every eighth pixel at 480 x 640)."""
    g = load_parts("r2d2")
    return g["%dx%d.score" % (H, W)], g["%dx%d.desc" % (H, W)]


def errors(score, desc, ref):
    """(max |score error|, max |desc error|) of maps [H,W] / [H,W,128] against ref = (score, desc)."""
    return float(np.abs(np.asarray(score, np.float64) - ref[0]).max()), float(np.abs(np.asarray(desc, np.float64) - ref[1]).max())
