#!/usr/bin/env python3
"""D2-Net (seeded stand-in weights, weights.random_d2net_state_dict(0): the reference's d2_tf.pth is not in its tree) under the batched PairPipeline: 640 x 480
pairs, nms_dist 6, top_k 1000, 16 pairs per step.

    python scripts/d2net_rate.py [--pairs 16] [--steps 30] [--warmup 3] [--repeats 3] [--out profiles/d2net_rate.json]

One JSON record: pairs/s from HIP events around the timed steps (the median of --repeats runs of --steps steps, after --warmup steps; the spread is recorded);
per-layer ms of one forward of 2 x pairs images from the context's own profile (HIP events around every launch, names d2_*) against each layer's split-f16 roof;
and the four head kernels' ms."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROOF = 838.9e12         # split-f16 FLOP/s roof of DESIGN section 5
H, W = 480, 640
SEED = 0
# output resolution divisor of every layer of weights._D2NET_LAYERS (the pooled layers are computed at their input's resolution)
DIV = {"conv1_1": 1, "conv1_2": 1, "conv2_1": 2, "conv2_2": 2, "conv3_1": 4, "conv3_2": 4, "conv3_3": 4, "conv4_1": 8, "conv4_2": 8, "conv4_3": 8}
HEAD = ("max", "softdetect", "sum", "upsample")


def layer_macs():
    from keypoint_bench_amd import weights
    return {name: co * ci * 9 * (H // DIV[name]) * (W // DIV[name]) for name, idx, (co, ci) in weights._D2NET_LAYERS}


def profile_forward(net, x, ctx, reps):
    import torch
    net(x)
    torch.cuda.synchronize()
    ctx.prof_enable(True)
    try:
        ctx.prof_report()
        for _ in range(reps):
            net(x)
        torch.cuda.synchronize()
        rep = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
    return {k[len("d2_"):]: v[1] / reps for k, v in rep.items() if k.startswith("d2_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    from keypoint_bench_amd.models.D2_Net import d2net_random
    from keypoint_bench_amd.pipeline import PairPipeline
    dev = "cuda:0"
    ep = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
    bf = dict(metric="euclidean", max_distance=5, cross_check=True)
    v = [synthetic.image_pair(5000 + i, H, W) for i in range(args.pairs)]
    images = torch.from_numpy(np.concatenate([np.stack([a for a, _ in v]), np.stack([b for _, b in v])])).to(dev)
    net = d2net_random(SEED)
    pipe = PairPipeline(net, ep, bf, args.pairs, H, W, device=dev)
    for _ in range(args.warmup):
        pipe.run(images)
    torch.cuda.synchronize()
    runs = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            pipe.run(images)
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / args.steps)
    ms = sorted(runs)[len(runs) // 2]
    ctx = _lib.Context.get(torch.device(dev))
    n_img = 2 * args.pairs
    kern = profile_forward(net, images, ctx, 3)
    macs = layer_macs()
    roof = {n: round(2.0 * macs[n] * n_img / (kern[n] * 1e-3) / ROOF, 4) for n in macs if n != "conv1_1"}       # conv1_1 runs on the vector ALU
    rec = {"workload": "D2-Net seeded stand-in, %d pairs of %dx%d per step, nms_dist 6, top_k 1000, brute-force matcher (exact path: 512 channels)" % (args.pairs, W, H),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "ms_per_step": round(ms, 3), "ms_per_step_runs": [round(r, 3) for r in runs],
           "pairs_per_s": round(args.pairs / ms * 1e3, 2), "mean_matches": float(pipe.k.float().mean()), "images_per_forward": n_img,
           "forward_ms": round(sum(kern.values()), 3), "kernels_ms": {n: round(t, 4) for n, t in kern.items()}, "roof_fraction": roof,
           "head_ms": {n: round(kern[n], 4) for n in HEAD},
           "furthest_from_roof": min(roof, key=lambda n: roof[n]), "gmac_per_image": round(sum(macs.values()) / 1e9, 2),
           "lib_sha256": hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:12], "lib_path_override": os.environ.get("KPB_LIB_PATH")}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
