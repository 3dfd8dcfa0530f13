#!/usr/bin/env python3
"""Golden fixtures for Key.Net from the REFERENCE class (models/KeyNet.py as model_interface.py constructs it from KeyNet_params, utils/extracter.py detection)
and the checkpoint its tree ships (weights/keynet_pytorch.pth, {'state_dict', 'optimizer'}):
  keynet_state_dict.npz   the checkpoint's state_dict tensors (without num_batches_tracked);
  keynet*.npz             the reference's fp32 CPU score [H, W] on synthetic.image_pair(0, H, W)[0] at five shapes, with the image checksum, the map's
                          maximum `amax`, the three level sizes and `ref_err` = max |fp32 run - the same model in .double()|;
  keynet_detect.npz       the reference's detection on its own map at 96 x 160 and 37 x 61 for (nms_dist, top_k) = (2, 5000), (4, 5000), (2, 100), border_dist 8,
                          threshold 0, min_score 0.  STABILITY: the keypoints of the fp32 map and of the fp64 map rounded to fp32 must be the same set of
                          pixels (difference 0) on every case, or the generator fails -- the condition is never relaxed.
kornia is not installed where this runs: exactly two of its functions are stood in, kornia.filters.spatial_gradient (3 x 3 Sobel pair / 8, correlation,
replicate padding, output [B,C,2,H,W]) and kornia.filters.filter2d (correlation with the given kernel over the `border_type`-padded map), both dtype-generic.
The stand-ins are NOT pinned against kornia itself.  Build container only; a no-op without the reference checkout.  Files stay under 1 MiB each.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SHAPES = ((16, 16), (30, 50), (37, 61), (96, 160), (480, 640))
DETECT_SHAPES = ((96, 160), (37, 61))
DETECT_CASES = ((2, 5000), (4, 5000), (2, 100))
STABILITY_EXTRA = ((64, 96), (96, 128), (30, 50))          # shapes checked for stability beyond the stored ones, seeds 0 and 1


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if not os.path.isdir(REF):
        print("reference checkout not present; nothing to do")
        return 0
    sys.dont_write_bytecode = True
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from keypoint_bench_amd import synthetic
    from make_golden_r2d2 import save_parts

    def spatial_gradient(x, mode="sobel", order=1, normalized=True):
        b, c, h, w = x.shape
        kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=x.dtype) / 8
        g = F.conv2d(F.pad(x.reshape(b * c, 1, h, w), (1, 1, 1, 1), mode="replicate"), torch.stack([kx, kx.t()])[:, None])
        return g.reshape(b, c, 2, h, w)

    def filter2d(x, kernel, border_type="reflect"):
        b, c, h, w = x.shape
        k = kernel.to(x.dtype)
        ph, pw = k.shape[-2] // 2, k.shape[-1] // 2
        return F.conv2d(F.pad(x.reshape(b * c, 1, h, w), (pw, pw, ph, ph), mode=border_type), k.reshape(1, 1, *k.shape[-2:])).reshape(b, c, h, w)

    kornia, kf = types.ModuleType("kornia"), types.ModuleType("kornia.filters")
    kf.spatial_gradient, kf.filter2d = spatial_gradient, filter2d
    kornia.filters = kf
    sys.modules.update({"kornia": kornia, "kornia.filters": kf})
    ref = _load("ref_keynet", "models", "KeyNet.py")
    E = _load("ref_extracter", "utils", "extracter.py")

    sd = torch.load(os.path.join(REF, "weights", "keynet_pytorch.pth"), map_location="cpu")["state_dict"]
    conf = dict(num_filters=8, num_levels=3, kernel_size=5)
    net, net64 = ref.KeyNet(conf), ref.KeyNet(conf)
    print("  keynet", net.load_state_dict(sd), net64.load_state_dict(sd))
    net.eval()
    net64.double().eval()
    save_parts("keynet_state_dict", {k: v.numpy() for k, v in sd.items() if not k.endswith("num_batches_tracked")})
    torch.set_num_threads(8)

    def run(v0):
        with torch.no_grad():
            s32, none = net(torch.from_numpy(v0)[None])
            s64, _ = net64(torch.from_numpy(v0)[None].double())
        assert none is None
        return s32, s64

    def detect(score, nd, top_k):
        return E.detection(score, dict(nms_dist=nd, threshold=0.0, border_dist=8, top_k=top_k, min_score=0.0))

    def pixels(k, H, W):       # detection gives ((column + 0.5) / W, (row + 0.5) / H, score) rows
        return set(map(tuple, np.rint(k[:, :2].numpy().astype(np.float64) * np.array([W, H]) - 0.5).astype(np.int64).tolist()))

    out = {}
    for H, W in SHAPES:
        v0, _ = synthetic.image_pair(0, H, W)
        s32, s64 = run(v0)
        tag = "%dx%d" % (H, W)
        err = float((s32.double() - s64).abs().max())
        h1, w1 = int(H // 1.2), int(W // 1.2)
        out[tag + ".img.sum"] = np.array(synthetic.checksum(v0))
        out[tag + ".score"] = s32[0, 0].numpy()
        out[tag + ".amax"] = np.array(float(s32.max()), np.float64)
        out[tag + ".levels"] = np.array([[H, W], [h1, w1], [int(h1 // 1.2), int(w1 // 1.2)]], np.int64)
        out[tag + ".ref_err"] = np.array(err, np.float64)
        print("  keynet", tag, "levels", out[tag + ".levels"].tolist(), "min %.4g max %.6g zeros %d ref_err %.3g (%.3g of amax)"
              % (float(s32.min()), float(s32.max()), int((s32 == 0).sum()), err, err / float(s32.max())))
    save_parts("keynet", out)

    det = {}
    for H, W in DETECT_SHAPES + STABILITY_EXTRA:
        for seed in (0, 1):
            v0, _ = synthetic.image_pair(seed, H, W)
            s32, s64 = run(v0)
            for nd, top_k in DETECT_CASES:
                k32, k64 = detect(s32, nd, top_k), detect(s64.float(), nd, top_k)
                diff = len(pixels(k32, H, W) ^ pixels(k64, H, W))
                assert len(pixels(k32, H, W)) == k32.shape[0]
                print("  keynet detect %dx%d seed %d nms_dist %d top_k %d: %d keypoints, fp32 / fp64 maps differ in %d" % (H, W, seed, nd, top_k, k32.shape[0], diff))
                assert diff == 0, "the reference's own keypoints are not stable on %dx%d seed %d nms_dist %d" % (H, W, seed, nd)
                if seed == 0 and (H, W) in DETECT_SHAPES:
                    det["%dx%d.nd%d.k%d" % (H, W, nd, top_k)] = k32.numpy()
    save_parts("keynet_detect", det)
    return 0


if __name__ == "__main__":
    sys.exit(main())
