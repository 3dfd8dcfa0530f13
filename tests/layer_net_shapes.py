"""What tests/test_gpu_layer_net_shapes.py and tests/test_layer_net_shape_oracles_cpu.py share: the shapes and batches of R2D2, SFD2 and D2-Net, their images,
the three nets' torch.nn.functional chains at any shape in fp32 and float64, the bounds of the GPU test as functions of the two chains alone, and the
deliberately wrong chains that show those bounds can fail.

The wrong chains are the fixtures' chains themselves with ONE primitive of torch.nn.functional replaced while they run (`wrong(kind)`), so a variant
differs from the oracle in the named respect and in nothing else:
  tap          a 2 x 2 convolution ignores the last row and column of its input: the bound `y < H` of a gathered tap read as `y < H - 1`
  replicate    a dilated 3 x 3 convolution pads by replicating the border instead of with zeros
  align        F.interpolate with the align_corners flag flipped (SFD2's stability logits, D2-Net's score map)
  zeros        F.pad fills with 0 where the caller asked for another value (D2-Net pads exp() with ones in front of its 3 x 3 mean)"""
import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

from keypoint_bench_amd import synthetic, weights

NETS = ("r2d2", "sfd2", "d2net")
SHAPES = {
    "r2d2": [(1, 1), (7, 200), (130, 6), (9, 9), (15, 17), (16, 16), (17, 33), (33, 129), (136, 200)],
    "sfd2": [(8, 136), (200, 8), (24, 8), (8, 264), (136, 24), (24, 40), (120, 160), (264, 328)],
    "d2net": [(8, 136), (200, 8), (24, 8), (8, 16), (136, 24), (24, 40), (120, 160), (264, 328)],
}
BATCHES = {
    "r2d2": [(3, (17, 33)), (5, (17, 33)), (9, (24, 40))],
    "sfd2": [(3, (24, 40)), (5, (24, 40)), (17, (16, 24))],
    "d2net": [(3, (24, 40)), (5, (24, 40)), (17, (16, 24))],
}
DESC = {"r2d2": (128, 1), "sfd2": (128, 4), "d2net": (512, 8)}          # channels, H / div x W / div
UNSURE_CAP = 0.01               # SFD2: at most this share of a shape's pixels may have a float64 stability margin below sfd2_fixtures.MARGIN
# D2-Net in these two files: d2net_fixtures' M_H16 = 8 was measured on five single images; the batch of 17 at 16 x 24 reaches 9.49 (split-f16) and 11.18 (strict
# fp32) without a defect (tests/test_gpu_layer_net_shapes.py explains it).  The fixtures' rule -- the smallest power of two that is at least twice the largest
# measured ratio, never above 16 -- stops at its cap, for both arithmetics; the fixtures' constants and the per-net tests keep theirs.
M_D2NET = 16
F64_FACTOR = 4                # tests/test_gpu_net_shapes.py: max |gpu - chain64| <= 4 max |chain32 - chain64| where the usual bound is missed by magnitude


def sid(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def image(seed, H, W, view=0):
    return synthetic.image_pair(seed, max(H, 64), max(W, 64))[view][:, :H, :W].copy()


def sweep_image(H, W):
    return image(40 + H + W, H, W)[None]


def batch_images(B, H, W):
    """B different images: different seeds, alternating views."""
    return np.stack([image(300 + 10 * B + i, H, W, view=i & 1) for i in range(B)])


@functools.lru_cache(maxsize=None)
def tensors(name, double=False):
    """The folded tensors the net object of the GPU test is made from, as numpy arrays in fp32 or cast to float64."""
    if name == "r2d2":
        from r2d2_fixtures import checkpoint
        t = weights.fold_r2d2(checkpoint()["state_dict"])
    elif name == "sfd2":
        from sfd2_fixtures import state_dict
        t = weights.fold_sfd2(state_dict())
    else:
        from d2net_fixtures import state_dict
        t = weights.fold_d2net(state_dict())
    return {k: np.ascontiguousarray(v, np.float64 if double else np.float32) for k, v in t.items()}


@contextlib.contextmanager
def wrong(kind):
    """torch.nn.functional with one primitive wrong while the block runs (module docstring); kind None changes nothing."""
    conv2d, interpolate, pad = F.conv2d, F.interpolate, F.pad

    def conv_tap(x, w, b=None, **kw):
        if w.shape[-1] == 2:
            x = x.clone()
            x[..., -1, :] = 0
            x[..., :, -1] = 0
        return conv2d(x, w, b, **kw)

    def conv_replicate(x, w, b=None, **kw):
        if w.shape[-1] == 3 and kw.get("dilation", 1) > 1:
            x, kw = pad(x, [kw["padding"]] * 4, mode="replicate"), dict(kw, padding=0)
        return conv2d(x, w, b, **kw)

    patch = {None: {}, "tap": {"conv2d": conv_tap}, "replicate": {"conv2d": conv_replicate},
             "align": {"interpolate": lambda x, **kw: interpolate(x, **dict(kw, align_corners=not kw["align_corners"]))},
             "zeros": {"pad": lambda x, p, **kw: pad(x, p, **dict(kw, value=0.0))}}[kind]
    for k, f in patch.items():
        setattr(F, k, f)
    try:
        yield
    finally:
        F.conv2d, F.interpolate, F.pad = conv2d, interpolate, pad


def oracle(name, imgs, double=False, kind=None):
    """(score [B,H,W], desc [B,C,H/div,W/div], margin [B,H,W] or None) of imgs [B,3,H,W] (numpy) from the net's chain, in fp32 or with the folded tensors and the
    image cast to float64; `kind` names a deliberately wrong variant."""
    from d2net_fixtures import chain as d2net_chain
    from r2d2_fixtures import chain as r2d2_chain
    from sfd2_fixtures import chain as sfd2_chain
    x = torch.from_numpy(np.ascontiguousarray(imgs, np.float64 if double else np.float32))
    t = tensors(name, double)
    with torch.no_grad(), wrong(kind):
        if name == "sfd2":
            s, d, m = sfd2_chain(t, x, margin=True)
            return s[:, 0].numpy(), d.numpy(), m.numpy()
        s, d = (r2d2_chain if name == "r2d2" else d2net_chain)(t, x)
    return s[:, 0].numpy(), d.numpy(), None


def sfd2_classes(imgs):
    """[B,H,W]: the stability class of every pixel in the float64 chain -- the argmax of the upsampled logits, seen as F.interpolate hands them back."""
    from sfd2_fixtures import chain
    interpolate, seen = F.interpolate, []

    def spy(x, **kw):
        seen.append(interpolate(x, **kw))
        return seen[-1]
    F.interpolate = spy
    try:
        with torch.no_grad():
            chain(tensors("sfd2", True), torch.from_numpy(np.ascontiguousarray(imgs, np.float64)))
    finally:
        F.interpolate = interpolate
    assert len(seen) == 1 and seen[0].shape[1] == 3
    return seen[0].argmax(1).numpy()


def constant_per_channel(m):
    """Whether every channel of m [C, ...] holds one value at all its pixels."""
    m = m.reshape(m.shape[0], -1)
    return bool((m == m[:, :1]).all())


def ulp32(a):
    """One fp32 unit in the last place of the largest magnitude of `a`."""
    return float(np.spacing(np.float32(np.abs(a).max())))


def ref_err(r32, r64, keep=None):
    """max |chain32 - chain64| over the pixels of `keep`, floored at one fp32 unit in the last place of the float64 map's largest magnitude: a smaller difference is
    an accident of rounding in the reference, not accuracy that a correct fp32 result can reach."""
    d = np.abs(r32.astype(np.float64) - r64)
    r = r64 if keep is None else r64[keep]
    return max(float((d if keep is None else d[keep]).max()), ulp32(r))


def ratio_rule(got, r32, r64, keep=None):
    """SFD2 and D2-Net, the per-net files' rule: (max |got - chain64|, ref_err) over the pixels of `keep`; the GPU test asserts error <= M x ref_err."""
    d = np.abs(got.astype(np.float64) - r64)
    return float((d if keep is None else d[keep]).max()), ref_err(r32, r64, keep)


def r2d2_rule(got, r32, r64, atol):
    """R2D2: (max |got - chain32|, max |got - chain64|, e_ref, holds): within atol of the fp32 chain, or -- missed by magnitude -- within F64_FACTOR x the fp32
    chain's own distance from the float64 one."""
    e32 = float(np.abs(got - r32).max())
    e64, e_ref = float(np.abs(got.astype(np.float64) - r64).max()), float(np.abs(r32.astype(np.float64) - r64).max())
    return e32, e64, e_ref, e32 <= atol or e64 <= F64_FACTOR * e_ref


def r2d2_atols():
    from test_gpu_r2d2 import ATOL_DESC, ATOL_SCORE
    return ATOL_SCORE, ATOL_DESC


def multiplier(name):
    """(split-f16, strict fp32) multipliers of these two files: SFD2's are M_H16 / M_FP32 of its fixtures, D2-Net's M_D2NET (above) for both."""
    if name == "sfd2":
        from sfd2_fixtures import M_FP32, M_H16
        return M_H16, M_FP32
    from d2net_fixtures import M_FP32, M_H16
    assert M_H16 <= M_D2NET and M_FP32 <= M_D2NET
    return M_D2NET, M_D2NET


def is_constant(a):
    return float(a.max()) == float(a.min())
