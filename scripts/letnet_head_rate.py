#!/usr/bin/env python3
"""letnet_head against goodpoint_head: both nets with their real checkpoints (the fixtures) forward the SAME 512 images of 480 x 640 in one process, the
library's own per-kernel profile (kpb_prof_enable / kpb_prof_report) around every launch -- no outside tool, nothing outside the repository.  Two rounds,
the nets in alternation; the summary takes each head's better round, their ratio, and both heads' TB/s on their 48 bytes per pixel.

    python scripts/letnet_head_rate.py [--images 512] [--steps 5] [--warmup 2] [--out profiles/letnet_head_rate.json]"""
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
    from keypoint_bench_amd.models.GoodPoint import GoodPoint
    from keypoint_bench_amd.models.LETNet import LETNet
    import goodpoint_fixtures
    import letnet_fixtures
    dev, B = "cuda:0", args.images
    gp = GoodPoint(goodpoint_fixtures.PARAM)
    gp.load_state_dict(goodpoint_fixtures.checkpoint())
    let = LETNet()
    let.load_state_dict(letnet_fixtures.checkpoint())
    ctx = Context.get(torch.device(dev))
    v = [synthetic.image_pair(5000 + i, H, W)[i & 1] for i in range(16)]
    images = torch.from_numpy(np.stack([v[i % 16] for i in range(B)])).to(dev)
    score = torch.empty((B, 1, H, W), device=dev)
    desc = torch.empty((B, H, W, 3), device=dev)
    out = {}
    for rnd in range(2):
        for name, net in (("goodpoint", gp), ("letnet", let)):
            net._ensure(images.device)
            fwd = lambda: ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(images), B, H, W, ptr(score), ptr(desc)))
            for _ in range(args.warmup):
                fwd()
            ctx.sync()
            ctx.prof_enable(True)
            try:
                ctx.prof_report()
                for _ in range(args.steps):
                    fwd()
                ctx.sync()
                rep = ctx.prof_report()
            finally:
                ctx.prof_enable(False)
            out["%s.%d" % (name, rnd)] = {k: round(ms / args.steps, 4) for k, (_, ms) in rep.items()}
    g = min(out["goodpoint.%d" % r]["goodpoint_head"] for r in range(2))
    l = min(out["letnet.%d" % r]["letnet_head"] for r in range(2))
    tbps = lambda ms: round(48.0 * H * W * B / (ms * 1e-3) / 1e12, 3)
    out["summary"] = {"goodpoint_head_ms": g, "letnet_head_ms": l, "ratio": round(l / g, 3), "letnet_head_TBps": tbps(l), "goodpoint_head_TBps": tbps(g)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
