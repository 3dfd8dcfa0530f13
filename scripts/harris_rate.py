#!/usr/bin/env python3
"""Harris's forward (csrc/harris.hip: one kernel, harris_response) on 512 images of 480 x 640 resident in HBM, against its byte floor: 12 B read and 4 B
written per pixel.  Prints the forward time between two events on the launch stream (profiling off) and what 16 B / pixel over that time comes to; the
kernel's own time is taken by running this script under a kernel trace, a run of its own:

    python scripts/harris_rate.py [--images 512] [--steps 20] [--warmup 3] [--block-size 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/harris_rate.py --steps 10

The floor's rate is what scripts/hbm_mix_rate.hip reports on the same box for its mixed load / store kernel."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 480, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-size", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from keypoint_bench_amd import synthetic
    from keypoint_bench_amd._lib import Context, ptr
    from keypoint_bench_amd.models.Harris import Harris
    dev, B = "cuda:0", args.images
    net = Harris(dict(block_size=args.block_size, ksize=3, k=0.04))
    ctx = Context.get(torch.device(dev))
    v = [synthetic.image_pair(5000 + i, H, W)[i & 1] for i in range(16)]
    images = torch.from_numpy(np.stack([v[i % 16] for i in range(B)])).to(dev)
    score = torch.empty((B, 1, H, W), device=dev)
    net._ensure(images.device)
    fwd = lambda: ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(images), B, H, W, ptr(score), ptr(None)))
    stream = torch.cuda.current_stream(images.device)
    best = None
    for _ in range(2):
        for _ in range(args.warmup):
            fwd()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            fwd()
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        best = ms if best is None else min(best, ms)
    nbytes = 16 * B * H * W
    print(json.dumps({"images": B, "shape": [H, W], "block_size": args.block_size, "steps": args.steps, "forward_ms": round(best, 4),
                      "bytes_16_per_pixel": nbytes, "TB_per_s_at_16B_per_pixel": round(nbytes / (best * 1e-3) / 1e12, 3)}))


if __name__ == "__main__":
    main()
