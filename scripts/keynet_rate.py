#!/usr/bin/env python3
"""Key.Net's forward against ALIKE-t's: both nets (Key.Net with the reference checkpoint of the fixtures, ALIKE-t with the packaged weights, no dense descriptor
map) forward the SAME 512 images of 480 x 640 in one process.  Two passes, nothing outside the repository:
  1. whole forwards between two events on the launch stream, profiling off, the nets in alternation over two rounds (the better round counts);
  2. a kernel trace of its own -- the library's per-kernel profile (kpb_prof_enable / kpb_prof_report) around every launch.
The summary has the two forward times, their ratio, Key.Net's kernels, and the share of the split-f16 MFMA layers (keynet_level_hc + keynet_conv5) in it.

    python scripts/keynet_rate.py [--images 512] [--steps 5] [--warmup 2] [--out profiles/keynet_rate.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
H, W = 480, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from keypoint_bench_amd import synthetic
    from keypoint_bench_amd._lib import Context, ptr
    from keypoint_bench_amd.models.ALike import alike_t
    from keypoint_bench_amd.models.KeyNet import KeyNet
    import keynet_fixtures
    dev, B = "cuda:0", args.images
    key = KeyNet(keynet_fixtures.PLAN)
    key.load_state_dict(keynet_fixtures.checkpoint())
    alike = alike_t(dense_descriptors=False)
    ctx = Context.get(torch.device(dev))
    v = [synthetic.image_pair(5000 + i, H, W)[i & 1] for i in range(16)]
    images = torch.from_numpy(np.stack([v[i % 16] for i in range(B)])).to(dev)
    score = torch.empty((B, 1, H, W), device=dev)
    nets = (("alike_t", alike), ("keynet", key))
    for _, net in nets:
        net._ensure(images.device)
    fwd = lambda net: ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(images), B, H, W, ptr(score), ptr(None)))
    out = {"images": B, "shape": [H, W], "arithmetic": "fp32" if os.environ.get("KPB_FP32_MATRIX") == "1" else "split-f16"}
    stream = torch.cuda.current_stream(images.device)
    for rnd in range(2):
        for name, net in nets:
            for _ in range(args.warmup):
                fwd(net)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                fwd(net)
            e1.record(stream)
            e1.synchronize()
            out["%s.forward_ms.%d" % (name, rnd)] = round(e0.elapsed_time(e1) / args.steps, 4)
    for name, net in nets:          # the kernel trace, a run of its own
        ctx.sync()
        ctx.prof_enable(True)
        try:
            ctx.prof_report()
            for _ in range(args.steps):
                fwd(net)
            ctx.sync()
            rep = ctx.prof_report()
        finally:
            ctx.prof_enable(False)
        out["%s.kernels_ms" % name] = {k: round(ms / args.steps, 4) for k, (_, ms) in rep.items()}
    a = min(out["alike_t.forward_ms.%d" % r] for r in range(2))
    k = min(out["keynet.forward_ms.%d" % r] for r in range(2))
    kk = out["keynet.kernels_ms"]
    mfma = kk.get("keynet_level_hc", 0.0) + kk.get("keynet_conv5", 0.0)
    out["summary"] = {"alike_t_forward_ms": a, "keynet_forward_ms": k, "ratio": round(k / a, 3), "keynet_kernels_ms_sum": round(sum(kk.values()), 4),
                      "keynet_layers_share": round(mfma / max(sum(kk.values()), 1e-9), 3),
                      "keynet_layers_TFLOPs": round(2 * (2000 + 1600 + 1600) * (1 + 400 * 533 / (H * W) + 333 * 444 / (H * W)) * H * W * B / max(mfma, 1e-9) / 1e9, 2)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
