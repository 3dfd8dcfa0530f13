#!/usr/bin/env python3
"""Golden fixtures for ALIKE-l from the REFERENCE class (models/ALike.py, ALNet(param=None): c1..c4 = 32, 64, 128, 128, dim = 128).  The reference ships no
checkpoint for this plan, so the weights are SEEDED STAND-INS: torch's default initialisation under a fixed seed, and every BatchNorm given non-trivial
weight / bias / running_mean / running_var from the same generator so that folding is exercised.  Saved: the state dict (alike_l_state_dict*.npz) and the
reference's fp32 CPU outputs on synthetic.image_pair(0, H, W)[0] at five shapes (alike_l*.npz) -- the image checksum, the full score map, and the descriptor
map in full for the first two shapes, desc[::8, ::8] for the other three.  Build container only; a no-op without the reference checkout.  Files stay under
1 MiB each: make_golden_r2d2.save_parts cuts the arrays into pieces (tests/alike_l_fixtures.py joins them again).
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SHAPES = ((32, 32), (32, 64), (64, 96), (96, 160), (160, 224))
FULL_DESC = 2           # the first FULL_DESC shapes keep the whole descriptor map
SEED = 2024
# BatchNorm ranges.  torch's default convolution initialisation shrinks a map by about 1 / sqrt(3) per layer, and the two layers behind the last BatchNorm
# (aggregation and head) have nothing to undo it: with weights around 1 the descriptors end at 0.1 and the score within 0.005 of 0.49 everywhere.  Weights of
# 2.5 .. 4 make up for it -- printed below: score 0.10 .. 0.48 (nowhere saturated), max |desc| 2.5 .. 4.5 -- and with the other three ranges a wrong fold
# misses every bar.
BN_WEIGHT, BN_BIAS, BN_MEAN, BN_VAR = (2.5, 4.0), (-0.5, 1.0), (-0.2, 0.2), (0.6, 1.5)


def main():
    if not os.path.isdir(REF):
        print("reference checkout not present; nothing to do")
        return 0
    import torch
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from keypoint_bench_amd import synthetic
    from make_golden_r2d2 import save_parts
    # the two torchvision conv factories the reference model uses, as tests/golden/make_golden.py stands them in
    tv, tvm, tvr = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.models.resnet")
    tvr.conv3x3 = lambda i, o, stride=1, groups=1, dilation=1: nn.Conv2d(i, o, 3, stride, dilation, dilation, groups, False)
    tvr.conv1x1 = lambda i, o, stride=1: nn.Conv2d(i, o, 1, stride, bias=False)
    tv.models, tvm.resnet = tvm, tvr
    ue, ux = types.ModuleType("utils"), types.ModuleType("utils.export")        # ALike.py imports utils.export.export_model and never calls it
    ux.export_model = lambda *a, **k: None
    ue.export = ux
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.models.resnet": tvr, "utils": ue, "utils.export": ux})
    spec = importlib.util.spec_from_file_location("ref_alike", os.path.join(REF, "models", "ALike.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(SEED)
    net = ref.ALNet()
    g = torch.Generator().manual_seed(SEED + 1)
    uni = lambda n, lo_hi: torch.rand(n, generator=g) * (lo_hi[1] - lo_hi[0]) + lo_hi[0]
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            with torch.no_grad():
                m.weight.copy_(uni(n, BN_WEIGHT)); m.bias.copy_(uni(n, BN_BIAS))
                m.running_mean.copy_(uni(n, BN_MEAN)); m.running_var.copy_(uni(n, BN_VAR))
    net.eval()
    sd = {k: v.detach().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    print("  alike_l state dict: %d tensors, %d floats" % (len(sd), sum(v.size for v in sd.values())))
    save_parts("alike_l_state_dict", sd)
    torch.set_num_threads(8)
    out = {}
    with torch.no_grad():
        for i, (H, W) in enumerate(SHAPES):
            v0, _ = synthetic.image_pair(0, H, W)
            score, desc = net(torch.from_numpy(v0)[None])
            tag = "%dx%d" % (H, W)
            d = desc[0].permute(1, 2, 0).contiguous().numpy()
            out[tag + ".img.sum"] = np.array(synthetic.checksum(v0))
            out[tag + ".score"] = score[0, 0].numpy()
            out[tag + ".desc"] = d if i < FULL_DESC else np.ascontiguousarray(d[::8, ::8])
            s = score[0, 0]
            print("  alike_l", tag, "score [%.4f, %.4f] mean %.4f, within 1e-3 of 0 or 1: %.3f; max |desc| %.3f, mean |desc| %.3f"
                  % (float(s.min()), float(s.max()), float(s.mean()), float(((s < 1e-3) | (s > 1 - 1e-3)).float().mean()), float(np.abs(d).max()), float(np.abs(d).mean())))
    save_parts("alike_l", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
