#!/usr/bin/env python3
"""ALIKE-l (the reference's default ALNet(): c1..c4 = 32, 64, 128, 128, dim 128; SEEDED STAND-IN weights, tests/golden/alike_l_state_dict*.npz -- the reference
ships no checkpoint for this plan) forward rates at 640 x 480, 2 x 16 images per step as the other rate scripts batch them.

    python scripts/alike_l_rate.py [--pairs 16] [--steps 10] [--warmup 3] [--out profiles/alike_l_rate.json]

One JSON record: images/s and ms per step of the dense forward (score + the [B, 480, 640, 128] descriptor map) and of the keypoint-only forward (score only),
from HIP events around the timed steps; the per-kernel ms of one forward of each kind from the context's own profile (HIP events around every launch, names
alikel_*); and for the dense head the achieved bytes/s of its ALGORITHMIC traffic -- 128 B read (x1) + 516 B written per pixel = 644 B/px, the small coarse maps
left out -- as a fraction of 8 TB/s, beside the ALIKE-t head's committed 0.66."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
H, W = 480, 640
HEAD_BYTES_PER_PIXEL = 128 + 516
HBM = 8.0e12
ALIKE_T_HEAD = 0.66


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def profile(fn, ctx, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ctx.prof_enable(True)
    try:
        ctx.prof_report()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        rep = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
    return {k: round(v[1] / reps, 4) for k, v in rep.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    from keypoint_bench_amd.models.ALike import ALNet
    from alike_l_fixtures import state_dict
    dev = "cuda:0"
    n_img = 2 * args.pairs
    v = [synthetic.image_pair(5000 + i, H, W) for i in range(args.pairs)]
    images = torch.from_numpy(np.concatenate([np.stack([a for a, _ in v]), np.stack([b for _, b in v])])).to(dev)
    net = ALNet().eval()
    net.load_state_dict(state_dict())
    dense = lambda: net._run(images, True)
    sparse = lambda: net._run(images, False)
    ms_dense, ms_sparse = timed(dense, args.steps, args.warmup), timed(sparse, args.steps, args.warmup)
    ctx = _lib.Context.get(torch.device(dev))
    k_dense, k_sparse = profile(dense, ctx, 3), profile(sparse, ctx, 3)
    head_ms = k_dense["alikel_head_dense"]
    head_bytes = HEAD_BYTES_PER_PIXEL * H * W * n_img
    rec = {"workload": "ALIKE-l seeded stand-in, %d images of %dx%d per step" % (n_img, W, H), "steps": args.steps, "warmup": args.warmup,
           "dense": {"ms_per_step": round(ms_dense, 3), "images_per_s": round(n_img / ms_dense * 1e3, 1), "kernels_ms": k_dense, "kernels_ms_sum": round(sum(k_dense.values()), 3)},
           "keypoint_only": {"ms_per_step": round(ms_sparse, 3), "images_per_s": round(n_img / ms_sparse * 1e3, 1), "kernels_ms": k_sparse,
                             "kernels_ms_sum": round(sum(k_sparse.values()), 3)},
           "dense_head": {"ms": head_ms, "algorithmic_bytes": head_bytes, "bytes_per_pixel": HEAD_BYTES_PER_PIXEL, "bytes_per_s": round(head_bytes / (head_ms * 1e-3), 0),
                          "fraction_of_8TBps": round(head_bytes / (head_ms * 1e-3) / HBM, 4), "alike_t_head_fraction": ALIKE_T_HEAD},
           "lib_sha256": hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:12], "lib_path_override": os.environ.get("KPB_LIB_PATH")}
    text = json.dumps(rec)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
