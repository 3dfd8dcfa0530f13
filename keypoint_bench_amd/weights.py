"""Weight container (.kpbw) shared by the HIP path and the parity oracle.

Layout (little endian): 16-byte header {magic "KPBWGT1\\0", u32 arch, u32 n}, n records of
{char name[40]; u32 ndim; u32 dims[4]; u32 offset_in_floats}, then the fp32 payload.
Tensors keep the reference's OIHW order; kernels repack at kpb_net_create time.

``fold_alike`` turns a state_dict of models/ALike.py (ALNet) into the folded tensor set:
eval-mode BatchNorm (model_interface.py:86) is folded into the preceding conv.
"""
import struct

import numpy as np

MAGIC = b"KPBWGT1\0"
ARCH_ALIKE = 1
ARCH_SUPERPOINT = 2
ARCH_XFEAT = 3
ARCH_DISK = 4
ARCH_LIGHTGLUE = 5
ARCH_R2D2 = 6
ARCH_EDGEPOINT = 7
ARCH_GOODPOINT = 8
ARCH_LETNET = 9
ARCH_KEYNET = 10
ARCH_SFD2 = 11
ARCH_D2NET = 12
ARCH_HARRIS = 13
_REC = struct.Struct("<40sI4II")


def pack(tensors: dict, arch: int) -> bytes:
    names = list(tensors)
    recs, payload, off = [], [], 0
    for n in names:
        a = np.ascontiguousarray(np.asarray(tensors[n], dtype=np.float32))
        dims = list(a.shape) + [1] * (4 - a.ndim)
        assert len(n.encode()) <= 40, "tensor name longer than the 40-byte field: " + n
        recs.append(_REC.pack(n.encode(), a.ndim, *dims, off))
        payload.append(a.tobytes())
        off += a.size
    return MAGIC + struct.pack("<II", arch, len(names)) + b"".join(recs) + b"".join(payload)


def unpack(blob: bytes):
    assert blob[:8] == MAGIC, "not a .kpbw blob"
    arch, n = struct.unpack_from("<II", blob, 8)
    base = 16 + n * _REC.size
    out = {}
    for i in range(n):
        name, ndim, d0, d1, d2, d3, off = _REC.unpack_from(blob, 16 + i * _REC.size)
        shape = (d0, d1, d2, d3)[:ndim]
        cnt = int(np.prod(shape)) if ndim else 1
        out[name.rstrip(b"\0").decode()] = np.frombuffer(blob, np.float32, cnt, base + 4 * off).reshape(shape).copy()
    return arch, out


def _np(v):
    return v.detach().cpu().numpy().astype(np.float64) if hasattr(v, "detach") else np.asarray(v, np.float64)


def _check(sd, need, net, plan):
    """Every key of `need` is in the state_dict with the shape `need` gives it, or ValueError names the net, the key and what `plan` needs."""
    for key, shape in need.items():
        if key not in sd:
            raise ValueError("%s state_dict: %s is missing" % (net, key))
        if tuple(sd[key].shape) != shape:
            raise ValueError("%s state_dict: %s has shape %s, %s needs %s" % (net, key, tuple(sd[key].shape), plan, shape))


def _fold(sd, conv, bn, eps=1e-5):
    w = _np(sd[conv + ".weight"])
    g, b = _np(sd[bn + ".weight"]), _np(sd[bn + ".bias"])
    mu, var = _np(sd[bn + ".running_mean"]), _np(sd[bn + ".running_var"])
    s = g / np.sqrt(var + eps)
    return (w * s[:, None, None, None]).astype(np.float32), (b - mu * s).astype(np.float32)


def fold_alike(sd) -> dict:
    """state_dict of ALNet (models/ALike.py:84-134) -> folded tensors named as csrc/alike.hip expects."""
    t = {}
    t["b1c1.w"], t["b1c1.b"] = _fold(sd, "block1.conv1", "block1.bn1")
    t["b1c2.w"], t["b1c2.b"] = _fold(sd, "block1.conv2", "block1.bn2")
    for i in (2, 3, 4):
        p, q = "block%d" % i, "b%d" % i
        t[q + "c1.w"], t[q + "c1.b"] = _fold(sd, p + ".conv1", p + ".bn1")
        t[q + "c2.w"], t[q + "c2.b"] = _fold(sd, p + ".conv2", p + ".bn2")
        w = _np(sd[p + ".downsample.weight"]).astype(np.float32)
        t[q + "ds.w"] = w.reshape(w.shape[0], w.shape[1])
        t[q + "ds.b"] = _np(sd[p + ".downsample.bias"]).astype(np.float32)
    for i in (1, 2, 3, 4):
        w = _np(sd["conv%d.weight" % i]).astype(np.float32)
        t["agg%d.w" % i] = w.reshape(w.shape[0], w.shape[1])
    w = _np(sd["convhead2.weight"]).astype(np.float32)
    t["head.w"] = w.reshape(w.shape[0], w.shape[1])
    return t


EDGEPOINT_PLAN = dict(c1=8, c2=16, c3=32, c4=64, dim=64)


def fold_edgepoint(sd) -> dict:
    """state_dict of EdgePoint (models/EdgePoint.py:84-141) -> the folded ALIKE-t trunk of fold_alike (head.w is convhead2, 64 x 64) plus the head's
    own layers as csrc/alike.hip expects them: score (conv_score, 16 -> 1), d8 / d4 (conv_8 / conv_4, 1 x 1 with stride 8 / 4) and ct4
    (conv_transpose_4, kept [in][out][ky][kx] as the state_dict has it).  Refused: a missing or mis-shaped tensor, any plan but 8,16,32,64 / 64."""
    c1, c2, c3, c4, dim = (EDGEPOINT_PLAN[k] for k in ("c1", "c2", "c3", "c4", "dim"))
    q = dim // 4
    need = {"block1.conv1.weight": (c1, 3, 3, 3), "block1.conv2.weight": (c1, c1, 3, 3)}
    for i, (ci, co) in ((2, (c1, c2)), (3, (c2, c3)), (4, (c3, c4))):
        p = "block%d" % i
        need.update({p + ".conv1.weight": (co, ci, 3, 3), p + ".conv2.weight": (co, co, 3, 3),
                     p + ".downsample.weight": (co, ci, 1, 1), p + ".downsample.bias": (co,)})
    for i, c in ((1, c1), (2, c2), (3, c3), (4, c4)):
        need["conv%d.weight" % i] = (q, c, 1, 1)
    for blk, co in (("block1", c1), ("block2", c2), ("block3", c3), ("block4", c4)):
        for bn in ("bn1", "bn2"):
            for leaf in ("weight", "bias", "running_mean", "running_var"):
                need["%s.%s.%s" % (blk, bn, leaf)] = (co,)
    need.update({"convhead2.weight": (dim, dim, 1, 1), "conv_score.weight": (1, q, 1, 1), "conv_score.bias": (1,),
                 "conv_8.weight": (q, q, 1, 1), "conv_8.bias": (q,), "conv_4.weight": (q, q, 1, 1), "conv_4.bias": (q,),
                 "conv_transpose_4.weight": (q, q, 4, 4), "conv_transpose_4.bias": (q,)})
    _check(sd, need, "EdgePoint", "the supported plan (c1..c4 = 8,16,32,64, dim = 64)")
    t = fold_alike(sd)
    f32 = lambda k: _np(sd[k]).astype(np.float32)
    t["score.w"], t["score.b"] = f32("conv_score.weight").reshape(q), f32("conv_score.bias")
    t["d8.w"], t["d8.b"] = f32("conv_8.weight").reshape(q, q), f32("conv_8.bias")
    t["d4.w"], t["d4.b"] = f32("conv_4.weight").reshape(q, q), f32("conv_4.bias")
    t["ct4.w"], t["ct4.b"] = f32("conv_transpose_4.weight"), f32("conv_transpose_4.bias")
    return t


GOODPOINT_PLAN = dict(c0=3, c1=8)


def fold_goodpoint(sd) -> dict:
    """state_dict of GoodPoint (models/GoodPoint.py:84-93) -> block 1 folded under the names fold_alike gives it (b1c1.w/.b, b1c2.w/.b: the reference's
    ConvBlock(3, 8) is ALIKE-t's block 1, and csrc/alike.hip binds it the same way), plus the two heads: gp.desc.w [3][8] (conv_head1, 1 x 1, no bias)
    and gp.score.w [8][3][3] (conv_head2, 3 x 3, one output channel, no bias).  Refused: a missing or mis-shaped tensor, any plan but c0 = 3, c1 = 8."""
    c0, c1 = GOODPOINT_PLAN["c0"], GOODPOINT_PLAN["c1"]
    need = {"block.conv1.weight": (c1, c0, 3, 3), "block.conv2.weight": (c1, c1, 3, 3), "conv_head1.weight": (3, c1, 1, 1), "conv_head2.weight": (1, c1, 3, 3)}
    for bn in ("bn1", "bn2"):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            need["block.%s.%s" % (bn, leaf)] = (c1,)
    _check(sd, need, "GoodPoint", "the supported plan (c0 = 3, c1 = 8)")
    t = {}
    t["b1c1.w"], t["b1c1.b"] = _fold(sd, "block.conv1", "block.bn1")
    t["b1c2.w"], t["b1c2.b"] = _fold(sd, "block.conv2", "block.bn2")
    t["gp.desc.w"] = _np(sd["conv_head1.weight"]).astype(np.float32).reshape(3, c1)
    t["gp.score.w"] = _np(sd["conv_head2.weight"]).astype(np.float32).reshape(c1, 3, 3)
    return t


LETNET_PLAN = dict(c1=8, c2=16, grayscale=False)


def fold_letnet(sd) -> dict:
    """state_dict of LETNet (models/LETNet.py:31-42) -> block 1 folded under the names fold_alike gives it (b1c1.w/.b, b1c2.w/.b: the reference's ConvBlock(3, 8)
    is ALIKE-t's block 1 once more), plus the two 1 x 1 convolutions as they are: let.conv1.w [16][8] (conv1, no bias) and let.head.w [4][16] (conv_head, no bias;
    rows 0..2 the map, row 3 the score).  Refused: a missing or mis-shaped tensor, any plan but c1 = 8, c2 = 16 on colour input."""
    c1, c2 = LETNET_PLAN["c1"], LETNET_PLAN["c2"]
    need = {"block1.conv1.weight": (c1, 3, 3, 3), "block1.conv2.weight": (c1, c1, 3, 3), "conv1.weight": (c2, c1, 1, 1), "conv_head.weight": (4, c2, 1, 1)}
    for bn in ("bn1", "bn2"):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            need["block1.%s.%s" % (bn, leaf)] = (c1,)
    _check(sd, need, "LETNet", "the supported plan (c1 = 8, c2 = 16, grayscale = False)")
    t = {}
    t["b1c1.w"], t["b1c1.b"] = _fold(sd, "block1.conv1", "block1.bn1")
    t["b1c2.w"], t["b1c2.b"] = _fold(sd, "block1.conv2", "block1.bn2")
    t["let.conv1.w"] = _np(sd["conv1.weight"]).astype(np.float32).reshape(c2, c1)
    t["let.head.w"] = _np(sd["conv_head.weight"]).astype(np.float32).reshape(4, c2)
    return t


KEYNET_PLAN = dict(num_filters=8, num_levels=3, kernel_size=5)


def fold_keynet(sd, eps=1e-5) -> dict:
    """state_dict of KeyNet (models/KeyNet.py:99-114; the checkpoint keeps it under 'state_dict') -> the folded tensors csrc/keynet.hip expects: l0 / l1 / l2
    (.w [8][10 or 8][5][5], .b [8]) are the learnable block's Conv2d(bias) + eval-mode BatchNorm2d, w' = w g / sqrt(var + eps) and
    b' = (b - mean) g / sqrt(var + eps) + beta per output channel, and last.w [1][24][5][5] / last.b [1] the fusion layer as it is (input channels
    [level 0 | level 1 | level 2]).  num_batches_tracked is dropped.  Refused: a missing or mis-shaped tensor, any plan but 8 filters, 3 levels, 5 x 5."""
    nf, nl, ks = (KEYNET_PLAN[k] for k in ("num_filters", "num_levels", "kernel_size"))
    need = {"last_conv.0.weight": (1, nf * nl, ks, ks), "last_conv.0.bias": (1,)}
    for i, cin in enumerate((10, nf, nf)):
        p = "feature_extractor.lb_block.conv%d." % i
        need.update({p + "0.weight": (nf, cin, ks, ks), p + "0.bias": (nf,)})
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            need[p + "1." + leaf] = (nf,)
    _check(sd, need, "KeyNet", "the supported plan (num_filters = 8, num_levels = 3, kernel_size = 5)")
    t = {}
    for i in range(3):
        p = "feature_extractor.lb_block.conv%d." % i
        s = _np(sd[p + "1.weight"]) / np.sqrt(_np(sd[p + "1.running_var"]) + eps)
        t["l%d.w" % i] = (_np(sd[p + "0.weight"]) * s[:, None, None, None]).astype(np.float32)
        t["l%d.b" % i] = ((_np(sd[p + "0.bias"]) - _np(sd[p + "1.running_mean"])) * s + _np(sd[p + "1.bias"])).astype(np.float32)
    t["last.w"] = _np(sd["last_conv.0.weight"]).astype(np.float32)
    t["last.b"] = _np(sd["last_conv.0.bias"]).astype(np.float32)
    return t


def keynet_level_sizes(H, W, levels=3):
    """[(h, w)] of the pyramid of models/KeyNet.py:85-96, 122-126: level l + 1 is (int(h // 1.2), int(w // 1.2)) of level l -- Python's float floor division,
    which csrc/keynet.hip restates as floor(h / 1.2) in double (equal for every size from 8 to 8192: tests/test_keynet_cpu.py)."""
    out = [(int(H), int(W))]
    for _ in range(levels - 1):
        h, w = out[-1]
        out.append((int(h // 1.2), int(w // 1.2)))
    return out


HARRIS_BLOCK_SIZES = (2, 3, 4, 5, 6)      # from 7 on (A + C)^2 can pass 2^53: the float64 response of csrc/harris.hip would no longer be exact up to its last line


def harris_plan(params) -> dict:
    """The reference's Harris constructor argument (models/Harris.py:16-18: block_size, ksize, k, each read with []) -> the one tensor csrc/harris.hip
    expects: harris.plan = [block_size, ksize, float32(k)], all three exact in fp32.  Refused (NotImplementedError, what kpb_net_create answers with
    KPB_E_UNSUPPORTED): any ksize but 3, a block_size outside 2 .. 6 or not an integer, a k that is not finite in fp32."""
    bs, ks, k = params["block_size"], params["ksize"], params["k"]
    if ks != 3:
        raise NotImplementedError("this build carries the Harris response with the 3 x 3 Sobel (ksize = 3) only; got ksize = %r" % (ks,))
    if bs not in HARRIS_BLOCK_SIZES:
        raise NotImplementedError("this build carries the Harris response for block_size 2 .. 6 only (from 7 on its integer terms pass 2^53); got %r" % (bs,))
    with np.errstate(over="ignore"):
        k32 = np.float32(k)
    if not np.isfinite(k32):
        raise NotImplementedError("Harris: k = %r is not finite in float32" % (k,))
    return {"harris.plan": np.array([bs, ks, k32], np.float32)}


SFD2_PLAN = dict(outdim=128, require_feature=False, require_stability=True, ms_detector=True)
# ResSegNetV2 (models/sfd2.py:90-134) as (folded name, convolution key, BatchNorm key or None, affine, (cout, cin per group, k), conv bias).  The folded names
# are those csrc/sfd2.hip reads; `res<i>.c2` is the grouped 3 x 3 (32 groups of 8): its weight is [256][8][3][3].
_SFD2_LAYERS = (("conv1a", "conv1a.0", "conv1a.1", False, (64, 3, 3), True), ("conv1b", "conv1b.0", "bn1b.0", False, (64, 64, 3), True),
                ("conv2a", "conv2a.0", "conv2a.1", False, (128, 64, 3), True), ("conv2b", "conv2b.0", "bn2b.0", False, (128, 128, 3), True),
                ("conv3a", "conv3a.0", "conv3a.1", False, (256, 128, 3), True), ("conv3b", "conv3b.0", "bn3b.0", False, (256, 256, 3), True)) + tuple(
    ("res%d.c%d" % (i, j), "conv4.%d.conv%d" % (i, j), "conv4.%d.bn%d" % (i, j), True, (256, 8 if j == 2 else 256, 3 if j == 2 else 1), False)
    for i in range(3) for j in (1, 2, 3)) + (
    ("convPa0", "convPa.0", "convPa.1", True, (256, 256, 3), True), ("convPa3", "convPa.3", None, False, (256, 256, 3), True),
    ("convPb", "convPb", None, False, (65, 256, 1), True),
    ("convDa0", "convDa.0", "convDa.1", True, (256, 256, 3), True), ("convDa3", "convDa.3", None, False, (256, 256, 3), True),
    ("convDb", "convDb", None, False, (128, 256, 1), True), ("sta", "ConvSta", None, False, (3, 256, 1), True))


def _sfd2_need():
    need = {}
    for name, conv, bn, affine, (co, ci, k), bias in _SFD2_LAYERS:
        need[conv + ".weight"] = (co, ci, k, k)
        if bias:
            need[conv + ".bias"] = (co,)
        if bn:
            for leaf in ("running_mean", "running_var") + (("weight", "bias") if affine else ()):
                need[bn + "." + leaf] = (co,)
    return need


def fold_sfd2(sd, eps=1e-5) -> dict:
    """state_dict of ResSegNetV2(outdim = 128, require_stability = True) (models/sfd2.py:90-134; the checkpoint keeps it under 'model', which the caller
    strips) -> the folded tensors csrc/sfd2.hip expects, `<name>.w` [cout][cin per group][k][k] and `<name>.b` [cout] per layer of _SFD2_LAYERS: every eval-mode
    BatchNorm (eps 1e-5; weight and bias only where it is affine) goes into the convolution in front of it, w' = w g / sqrt(var + eps) and
    b' = (b - mean) g / sqrt(var + eps) + beta per output channel (b = 0 for the ResBlocks' bias-free convolutions).  Keys the forward does not use
    (num_batches_tracked, heads of other variants) are ignored, as the reference's load_state_dict(strict=False) ignores them.  Refused: a missing or
    mis-shaped tensor."""
    _check(sd, _sfd2_need(), "SFD2", "ResSegNetV2(outdim = 128, require_stability = True)")
    t = {}
    for name, conv, bn, affine, (co, ci, k), bias in _SFD2_LAYERS:
        w = _np(sd[conv + ".weight"])
        b = _np(sd[conv + ".bias"]) if bias else np.zeros(co)
        if bn:
            s = 1.0 / np.sqrt(_np(sd[bn + ".running_var"]) + eps)
            if affine:
                s = s * _np(sd[bn + ".weight"])
            w, b = w * s[:, None, None, None], (b - _np(sd[bn + ".running_mean"])) * s
            if affine:
                b = b + _np(sd[bn + ".bias"])
        t[name + ".w"], t[name + ".b"] = w.astype(np.float32), b.astype(np.float32)
    return t


def random_sfd2_state_dict(seed: int) -> dict:
    """Seeded stand-in for the absent weights/sfd2.pth (.MISSING_LARGE_BLOBS), drawn from numpy so the same seed gives the same tensors on every machine:
    conv weights N(0, 2 / fan_in) with fan_in = shape[1] k^2, conv biases and BatchNorm biases / running means N(0, 0.1^2), BatchNorm weights and running
    variances U(0.75, 1.25); num_batches_tracked as the reference's BatchNorms keep it."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, conv, bn, affine, (co, ci, k), bias in _SFD2_LAYERS:
        sd[conv + ".weight"] = rng.normal(0.0, np.sqrt(2.0 / (ci * k * k)), size=(co, ci, k, k)).astype(np.float32)
        if bias:
            sd[conv + ".bias"] = rng.normal(0.0, 0.1, size=(co,)).astype(np.float32)
        if bn:
            if affine:
                sd[bn + ".weight"] = rng.uniform(0.75, 1.25, size=(co,)).astype(np.float32)
                sd[bn + ".bias"] = rng.normal(0.0, 0.1, size=(co,)).astype(np.float32)
            sd[bn + ".running_mean"] = rng.normal(0.0, 0.1, size=(co,)).astype(np.float32)
            sd[bn + ".running_var"] = rng.uniform(0.75, 1.25, size=(co,)).astype(np.float32)
            sd[bn + ".num_batches_tracked"] = np.array(0, np.int64)
    return sd


# D2-Net's trunk (models/D2_Net.py:10-46) = torchvision's vgg16().features[:22] as (folded name, index in that Sequential, (cout, cin)): ten 3 x 3 layers with
# bias and no BatchNorm; a 2 x 2 max-pool follows conv1_2, conv2_2 and conv3_3, a ReLU every layer but conv4_3.  The folded names are those csrc/d2net.hip reads.
_D2NET_LAYERS = (("conv1_1", 0, (64, 3)), ("conv1_2", 2, (64, 64)), ("conv2_1", 5, (128, 64)), ("conv2_2", 7, (128, 128)),
                 ("conv3_1", 10, (256, 128)), ("conv3_2", 12, (256, 256)), ("conv3_3", 14, (256, 256)),
                 ("conv4_1", 17, (512, 256)), ("conv4_2", 19, (512, 512)), ("conv4_3", 21, (512, 512)))
_D2NET_KEY = "dense_feature_extraction.model.%d."


def fold_d2net(sd) -> dict:
    """state_dict of D2Net (models/D2_Net.py:84-96; the checkpoint keeps it under 'model', which the caller strips) -> the tensors csrc/d2net.hip expects,
    `<name>.w` [cout][cin][3][3] and `<name>.b` [cout] per layer of _D2NET_LAYERS.  There is nothing to fold (no BatchNorm): the ten pairs are renamed.  Keys the
    forward does not read are ignored.  Refused: a missing or mis-shaped tensor (ValueError names the key and the shape it needs)."""
    t = {}
    for name, idx, (co, ci) in _D2NET_LAYERS:
        for leaf, out, shape in (("weight", ".w", (co, ci, 3, 3)), ("bias", ".b", (co,))):
            key = _D2NET_KEY % idx + leaf
            if key not in sd:
                raise ValueError("D2Net state_dict: %s is missing (needs shape %s)" % (key, shape))
            if tuple(sd[key].shape) != shape:
                raise ValueError("D2Net state_dict: %s has shape %s, D2Net needs %s" % (key, tuple(sd[key].shape), shape))
            t[name + out] = _np(sd[key]).astype(np.float32)
    return t


def random_d2net_state_dict(seed: int) -> dict:
    """Seeded stand-in for the absent weights/d2_tf.pth (.MISSING_LARGE_BLOBS), drawn from numpy so the same seed gives the same tensors on every machine:
    He-scaled weights N(0, 2 / (9 cin)), biases N(0, 0.05^2)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, idx, (co, ci) in _D2NET_LAYERS:
        sd[_D2NET_KEY % idx + "weight"] = rng.normal(0.0, np.sqrt(2.0 / (9 * ci)), size=(co, ci, 3, 3)).astype(np.float32)
        sd[_D2NET_KEY % idx + "bias"] = rng.normal(0.0, 0.05, size=(co,)).astype(np.float32)
    return sd


def load_alike_t():
    """The ALIKE-t tensors shipped with the package (folded from the reference's weights/alike-t.pth)."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "weights", "alike-t.kpbw")
    with open(path, "rb") as f:
        return unpack(f.read())[1]


SUPERPOINT_LAYERS = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b",
                     "convPa", "convPb", "convDa", "convDb")


def tensors_superpoint(sd) -> dict:
    """state_dict of SuperPointNet (models/SuperPoint.py:9-28) -> fp32 tensors under the same names."""
    t = {}
    for n in SUPERPOINT_LAYERS:
        t[n + ".weight"] = _np(sd[n + ".weight"]).astype(np.float32)
        t[n + ".bias"] = _np(sd[n + ".bias"]).astype(np.float32)
    return t


def random_superpoint(seed: int) -> dict:
    """Seeded stand-in for the absent superpoint_v1.pth (.MISSING_LARGE_BLOBS): He-uniform conv weights, small
    biases, drawn from numpy so the same seed gives the same tensors on every machine."""
    rng = np.random.default_rng(seed)
    shapes = dict(conv1a=(64, 1, 3), conv1b=(64, 64, 3), conv2a=(64, 64, 3), conv2b=(64, 64, 3), conv3a=(128, 64, 3),
                  conv3b=(128, 128, 3), conv4a=(128, 128, 3), conv4b=(128, 128, 3), convPa=(256, 128, 3),
                  convPb=(65, 256, 1), convDa=(256, 128, 3), convDb=(256, 256, 1))
    t = {}
    for n in SUPERPOINT_LAYERS:
        co, ci, k = shapes[n]
        bound = np.sqrt(6.0 / (ci * k * k))
        t[n + ".weight"] = rng.uniform(-bound, bound, size=(co, ci, k, k)).astype(np.float32)
        t[n + ".bias"] = rng.uniform(-0.05, 0.05, size=(co,)).astype(np.float32)
    return t


XFEAT_BASIC = ("block1.0", "block1.1", "block1.2", "block1.3", "block2.0", "block2.1", "block3.0", "block3.1", "block3.2",
               "block4.0", "block4.1", "block4.2", "block5.0", "block5.1", "block5.2", "block5.3",
               "block_fusion.0", "block_fusion.1", "keypoint_head.0", "keypoint_head.1", "keypoint_head.2")
XFEAT_SHAPES = {"block1.0": (4, 1, 3), "block1.1": (8, 4, 3), "block1.2": (8, 8, 3), "block1.3": (24, 8, 3),
                "block2.0": (24, 24, 3), "block2.1": (24, 24, 3), "block3.0": (64, 24, 3), "block3.1": (64, 64, 3),
                "block3.2": (64, 64, 1), "block4.0": (64, 64, 3), "block4.1": (64, 64, 3), "block4.2": (64, 64, 3),
                "block5.0": (128, 64, 3), "block5.1": (128, 128, 3), "block5.2": (128, 128, 3), "block5.3": (64, 128, 1),
                "block_fusion.0": (64, 64, 3), "block_fusion.1": (64, 64, 3), "keypoint_head.0": (64, 64, 1),
                "keypoint_head.1": (64, 64, 1), "keypoint_head.2": (64, 64, 1)}


def fold_xfeat(sd, eps=1e-5) -> dict:
    """state_dict of XFeatModel (models/XFeat.py:22-94) -> folded tensors.  BasicLayer (XFeat.py:7-19) is
    conv(bias=False) + BatchNorm2d(affine=False) + ReLU: w' = w / sqrt(var + eps), b' = -mean / sqrt(var + eps).
    heatmap_head and fine_matcher are constructed by the reference but never used by forward (XFeat.py:112-140)."""
    t = {}
    for n in XFEAT_BASIC:
        w = _np(sd[n + ".layer.0.weight"])
        mu, var = _np(sd[n + ".layer.1.running_mean"]), _np(sd[n + ".layer.1.running_var"])
        s = 1.0 / np.sqrt(var + eps)
        t[n + ".w"] = (w * s[:, None, None, None]).astype(np.float32)
        t[n + ".b"] = (-mu * s).astype(np.float32)
    t["block_fusion.2.w"] = _np(sd["block_fusion.2.weight"]).astype(np.float32)
    t["block_fusion.2.b"] = _np(sd["block_fusion.2.bias"]).astype(np.float32)
    t["keypoint_head.3.w"] = _np(sd["keypoint_head.3.weight"]).astype(np.float32)
    t["keypoint_head.3.b"] = _np(sd["keypoint_head.3.bias"]).astype(np.float32)
    t["skip1.w"] = _np(sd["skip1.1.weight"]).astype(np.float32).reshape(24)
    t["skip1.b"] = _np(sd["skip1.1.bias"]).astype(np.float32)
    return t


def random_xfeat_state_dict(seed: int) -> dict:
    """Seeded stand-in for the absent xfeat.pt: the state_dict entries XFeatModel.forward reads."""
    rng = np.random.default_rng(seed)
    sd = {}
    for n in XFEAT_BASIC:
        co, ci, k = XFEAT_SHAPES[n]
        bound = np.sqrt(6.0 / (ci * k * k))
        sd[n + ".layer.0.weight"] = rng.uniform(-bound, bound, size=(co, ci, k, k)).astype(np.float32)
        sd[n + ".layer.1.running_mean"] = rng.normal(0.0, 0.1, size=(co,)).astype(np.float32)
        sd[n + ".layer.1.running_var"] = rng.uniform(0.5, 1.5, size=(co,)).astype(np.float32)
    for n, (co, ci) in (("block_fusion.2", (64, 64)), ("keypoint_head.3", (65, 64))):
        bound = np.sqrt(6.0 / ci)
        sd[n + ".weight"] = rng.uniform(-bound, bound, size=(co, ci, 1, 1)).astype(np.float32)
        sd[n + ".bias"] = rng.uniform(-0.05, 0.05, size=(co,)).astype(np.float32)
    sd["skip1.1.weight"] = rng.uniform(-1, 1, size=(24, 1, 1, 1)).astype(np.float32)
    sd["skip1.1.bias"] = rng.uniform(-0.05, 0.05, size=(24,)).astype(np.float32)
    return sd

DISK_BLOCKS = (("down1", "unet.path_down.1.1", 16, 32), ("down2", "unet.path_down.2.1", 32, 64),
               ("down3", "unet.path_down.3.1", 64, 64), ("down4", "unet.path_down.4.1", 64, 64),
               ("up0", "unet.path_up.0.conv", 128, 64), ("up1", "unet.path_up.1.conv", 128, 64),
               ("up2", "unet.path_up.2.conv", 96, 64), ("up3", "unet.path_up.3.conv", 80, 129))


def tensors_disk(sd) -> dict:
    """state_dict of DISK (models/disk.py:293-307; the reference loads checkpoint['extractor'],
    model_interface.py:76-78) -> tensors named as csrc/convnet.hip expects.  Conv = Sequential(norm, PReLU,
    dropout, conv) (disk.py:76-97): index 1 is the PReLU slope, index 3 the convolution."""
    t = {"down0.w": _np(sd["unet.path_down.0.1.3.weight"]).astype(np.float32),
         "down0.b": _np(sd["unet.path_down.0.1.3.bias"]).astype(np.float32)}
    for name, key, cin, cout in DISK_BLOCKS:
        t[name + ".w"] = _np(sd[key + ".3.weight"]).astype(np.float32)
        t[name + ".b"] = _np(sd[key + ".3.bias"]).astype(np.float32)
        slope = _np(sd[key + ".1.weight"]).astype(np.float32).reshape(-1)
        t[name + ".slope"] = np.broadcast_to(slope, (cin,)).copy() if slope.size == 1 else slope
    return t


def random_disk_state_dict(seed: int) -> dict:
    """Seeded stand-in for the absent disk.pth."""
    rng = np.random.default_rng(seed)
    sd = {}

    def conv(key, co, ci):
        bound = np.sqrt(6.0 / (ci * 25))
        sd[key + ".3.weight"] = rng.uniform(-bound, bound, size=(co, ci, 5, 5)).astype(np.float32)
        sd[key + ".3.bias"] = rng.uniform(-0.05, 0.05, size=(co,)).astype(np.float32)

    conv("unet.path_down.0.1", 16, 3)
    for name, key, cin, cout in DISK_BLOCKS:
        conv(key, cout, cin)
        sd[key + ".1.weight"] = rng.uniform(0.1, 0.4, size=(cin,)).astype(np.float32)
    return sd


# Quad_L2Net_ConfCFS (models/r2d2.py:101-131, dilated = True): every layer at full resolution, the strides of L2-Net turned into the dilation of
# the layers behind them.  (name, cin, cout, k, dilation, bn, relu); padding = (k - 1) dilation / 2, BatchNorm2d(affine=False, eps 1e-5); a 2 x 2
# kernel's taps sit at -dilation / 2 and +dilation / 2.  `name` is the folded tensor's prefix, ops.N the state_dict's (conv N, then its BN).
R2D2_PLAN = (("conv0", 3, 32, 3, 1, True, True), ("conv1", 32, 32, 3, 1, True, True), ("conv2", 32, 64, 3, 1, True, True),
             ("conv3", 64, 64, 3, 2, True, True), ("conv4", 64, 128, 3, 2, True, True), ("conv5", 128, 128, 3, 4, True, True),
             ("conv6", 128, 128, 2, 4, True, False), ("conv7", 128, 128, 2, 8, True, False), ("conv8", 128, 128, 2, 16, False, False))
R2D2_NET = "Quad_L2Net_ConfCFS()"


def fold_r2d2(sd, eps=1e-5) -> dict:
    """state_dict of Quad_L2Net_ConfCFS (the checkpoint's keys carry a `module.` prefix, model_interface.py:71) -> folded tensors named as
    csrc/r2d2.hip expects: w' = w / sqrt(var + eps), b' = (b - mean) / sqrt(var + eps) per output channel.  A state_dict whose tensors do not
    have the shapes of R2D2_PLAN (another variant of r2d2.py, another `dim` or `mchan`) is refused."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}

    def take(key, shape):
        if key not in sd:
            raise ValueError("R2D2 state_dict: %s is missing" % key)
        a = _np(sd[key])
        if tuple(a.shape) != tuple(shape):
            raise ValueError("R2D2 state_dict: %s has shape %s, the Quad_L2Net_ConfCFS plan needs %s" % (key, tuple(a.shape), tuple(shape)))
        return a

    t, op = {}, 0
    for name, cin, cout, k, dil, bn, relu in R2D2_PLAN:
        w, b = take("ops.%d.weight" % op, (cout, cin, k, k)), take("ops.%d.bias" % op, (cout,))
        op += 1
        if bn:
            mu, var = take("ops.%d.running_mean" % op, (cout,)), take("ops.%d.running_var" % op, (cout,))
            op += 1
            s = 1.0 / np.sqrt(var + eps)
            w, b = w * s[:, None, None, None], (b - mu) * s
        op += 1 if relu else 0
        t[name + ".w"], t[name + ".b"] = w.astype(np.float32), b.astype(np.float32)
    t["clf.w"], t["clf.b"] = take("clf.weight", (2, 128, 1, 1)).reshape(2, 128).astype(np.float32), take("clf.bias", (2,)).astype(np.float32)
    t["sal.w"], t["sal.b"] = take("sal.weight", (1, 128, 1, 1)).reshape(1, 128).astype(np.float32), take("sal.bias", (1,)).astype(np.float32)
    return t


MATRIX_MODES = {"split": 0, "f16": 1}       # the values of the optional tensor matrix.mode (include/kpb.h, KPB_ARCH_R2D2)


def matrix_mode(matrix) -> int:
    """The matrix.mode value of a net's `matrix` keyword: "split" (three split-f16 MFMAs per product, fp32-class results) or "f16" (one MFMA on the
    f16-rounded operands, fp32 accumulation: TF32-class).  Anything else is a ValueError."""
    if not isinstance(matrix, str) or matrix not in MATRIX_MODES:
        raise ValueError("matrix must be 'split' or 'f16', not %r" % (matrix,))
    return MATRIX_MODES[matrix]


def with_matrix_mode(tensors: dict, matrix) -> dict:
    """`tensors` for pack(), with the tensor matrix.mode = [1.0] added for matrix = "f16".  "split" adds nothing: its blob is the blob of a build without the
    mode, byte for byte.  The tensors themselves must not carry the name already."""
    mode = matrix_mode(matrix)
    if "matrix.mode" in tensors:
        raise ValueError("the tensor set already carries matrix.mode")
    return dict(tensors, **{"matrix.mode": np.array([mode], np.float32)}) if mode else dict(tensors)


LG_LAYERS = 9


def tensors_lightglue(sd) -> dict:
    """state_dict of LightGlue (models/lightglue.py:392-409) -> fp32 tensors under the reference's own names; old
    checkpoints' self_attn.{i} / cross_attn.{i} keys are renamed as the reference does at load time (427-433)."""
    t = {}
    for k, v in sd.items():
        for i in range(LG_LAYERS):
            if not k.startswith("transformers."):
                k = k.replace("self_attn.%d" % i, "transformers.%d.self_attn" % i)
                k = k.replace("cross_attn.%d" % i, "transformers.%d.cross_attn" % i)
        if k == "confidence_thresholds" or k.endswith("inner_attn") or not hasattr(v, "shape"):
            continue
        t[k] = _np(v).astype(np.float32)
    return t


def random_lightglue_state_dict(seed: int, input_dim: int = 256, variant: str = "plain") -> dict:
    """Seeded stand-in for the absent superpoint_lightglue / disk_lightglue checkpoints.  The transformer is a
    damped random network (its residual branches are scaled down so descriptors stay close to their input) and
    final_proj is near a scaled identity, so that corresponding keypoints of a synthetic pair really match.
      plain  : no layer is confident -> all nine layers run, nothing is pruned
      stop   : token confidence saturates from layer 2 on -> check_if_stop fires (lightglue.py:670-681)
      prune  : token confidence and matchability are bimodal at layers 0-3 -> get_pruning_mask drops points (659-668)"""
    rng = np.random.default_rng(seed)
    sd = {}

    def lin(name, co, ci, scale=1.0, bias=0.02):
        b = np.sqrt(3.0 / ci) * scale
        sd[name + ".weight"] = rng.uniform(-b, b, size=(co, ci)).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-bias, bias, size=(co,)).astype(np.float32)

    if input_dim != 256:
        lin("input_proj", 256, input_dim, 1.0)
    sd["posenc.Wr.weight"] = rng.normal(0, 1.0, size=(32, 2)).astype(np.float32)
    for i in range(LG_LAYERS):
        for blk, names in (("self_attn", (("Wqkv", 768, 256, 1.0), ("out_proj", 256, 256, 0.3))),
                           ("cross_attn", (("to_qk", 256, 256, 1.0), ("to_v", 256, 256, 1.0), ("to_out", 256, 256, 0.3)))):
            p = "transformers.%d.%s" % (i, blk)
            for n, co, ci, sc in names:
                lin(p + "." + n, co, ci, sc)
            lin(p + ".ffn.0", 512, 512, 1.0)
            sd[p + ".ffn.1.weight"] = rng.uniform(0.8, 1.2, size=(512,)).astype(np.float32)
            sd[p + ".ffn.1.bias"] = rng.uniform(-0.1, 0.1, size=(512,)).astype(np.float32)
            lin(p + ".ffn.3", 256, 512, 0.15)
        p = "log_assignment.%d" % i
        sd[p + ".final_proj.weight"] = (10.0 * np.eye(256) + rng.normal(0, 0.05, size=(256, 256))).astype(np.float32)
        sd[p + ".final_proj.bias"] = rng.uniform(-0.02, 0.02, size=(256,)).astype(np.float32)
        sd[p + ".matchability.weight"] = rng.normal(0, 0.05, size=(1, 256)).astype(np.float32)
        sd[p + ".matchability.bias"] = np.array([3.0], np.float32)
        if i < LG_LAYERS - 1:
            p = "token_confidence.%d.token.0" % i
            sd[p + ".weight"] = rng.normal(0, 0.05, size=(1, 256)).astype(np.float32)
            sd[p + ".bias"] = np.array([-1.0], np.float32)
    if variant == "stop":
        for i in range(2, LG_LAYERS - 1):
            sd["token_confidence.%d.token.0.bias" % i] = np.array([6.0], np.float32)
    elif variant == "prune":
        for i in range(0, 4):
            sd["token_confidence.%d.token.0.weight" % i] = rng.normal(0, 4.0, size=(1, 256)).astype(np.float32)
            sd["token_confidence.%d.token.0.bias" % i] = np.array([0.0], np.float32)
            sd["log_assignment.%d.matchability.weight" % i] = rng.normal(0, 4.0, size=(1, 256)).astype(np.float32)
            sd["log_assignment.%d.matchability.bias" % i] = np.array([0.0], np.float32)
    elif variant != "plain":
        raise ValueError(variant)
    return sd
