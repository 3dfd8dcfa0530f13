#!/usr/bin/env python3
"""DISK (seeded weights, disk_random(5)) dense against keypoint-only at 640 x 480, in ONE process on one box, the two modes alternated.

    python scripts/disk_keypoint_only_rate.py [--pairs 16] [--rounds 5] [--steps 5] [--warmup 2] [--top-k 1000] [--out profiles/disk_keypoint_only.txt]

Measured with device events around synchronised work, each figure the median over --rounds rounds of --steps steps, a round of one mode followed by a round of the other:
  kpb_net_forward on 2 x pairs images, dense (score + the [B, 480, 640, 128] map) and keypoint-only (score only);
  kpb_net_desc_at at top-k points per image on that batch;
  PairPipeline (DISK + brute force, top_k = top-k, place_map off for both) in pairs/s, both modes;
  the per-kernel ms of one forward of each kind and of desc_at from the context's own profile (events around every launch).
Beside them the work each new kernel has from the shapes and what share of the matrix peak / HBM rate that is."""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 480, 640
F16_DENSE_PEAK = 2.5e15         # v_mfma_f32_32x32x16_f16, dense, whole chip (MI355X data sheet)
HBM = 8.0e12


def timed(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def alternated(fns, rounds, steps, warmup):
    """{name: (median ms, [ms per round])}: every round runs each fn in turn."""
    for f in fns.values():
        for _ in range(warmup):
            f()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            ms[k].append(timed(f, steps))
    return {k: (statistics.median(v), [round(x, 3) for x in v]) for k, v in ms.items()}


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--top-k", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    from keypoint_bench_amd._lib import ptr
    from keypoint_bench_amd.models.disk import disk_random
    from keypoint_bench_amd.pipeline import PairPipeline
    dev = torch.device("cuda:0")
    B, K = 2 * args.pairs, args.top_k
    v = [synthetic.image_pair(5000 + i, H, W) for i in range(args.pairs)]
    images = torch.from_numpy(np.concatenate([np.stack([a for a, _ in v]), np.stack([b for _, b in v])])).to(dev)
    net = disk_random(5).eval()
    net._ensure(dev)
    ctx = _lib.Context.get(dev)
    score = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    desc = torch.empty((B, H, W, 128), dtype=torch.float32, device=dev)
    pts = torch.rand((B, K, 2), device=dev)
    n = torch.full((B,), K, dtype=torch.int32, device=dev)
    out = torch.empty((B, K, 128), dtype=torch.float32, device=dev)
    fwd = lambda d: ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(images), B, H, W, ptr(score), ptr(d)))
    dense, sparse = (lambda: fwd(desc)), (lambda: fwd(None))
    desc_at = lambda: ctx.check(ctx.lib.kpb_net_desc_at(net._handle, ptr(pts), 2, K, ptr(n), ptr(out)))
    f = alternated({"dense": dense, "keypoint_only": sparse}, args.rounds, args.steps, args.warmup)
    sparse()
    a = alternated({"desc_at": desc_at}, args.rounds, args.steps, args.warmup)
    k_dense, k_sparse, k_at = profile(dense, ctx, 3), profile(sparse, ctx, 3), profile(desc_at, ctx, 3)
    del desc
    torch.cuda.empty_cache()
    ep = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=K, min_score=0.0)
    bf = {"metric": "euclidean", "max_distance": float("inf"), "cross_check": True}
    pipes = {m: PairPipeline(disk_random(5, dense_descriptors=(m == "dense")).eval(), ep, bf, args.pairs, H, W, device=dev, place_map=False) for m in ("dense", "keypoint_only")}
    p = alternated({m: (lambda q=q: q.run(images)) for m, q in pipes.items()}, args.rounds, args.steps, args.warmup)
    matches = {m: int(q.k.sum().item()) for m, q in pipes.items()}
    P = H * W
    up3_ms, score_ms, at_ms = k_dense["disk_up3"], k_sparse["disk_up3_score"], k_at["disk_desc_at"]
    dense_flop, tap_flop, score_flop = 2.0 * 25 * 80 * 129 * P * B, 8.0 * K * 2000 * 128 * B, 2.0 * 2000 * P * B
    score_bytes = B * P * (16 * 4 + 16 * 4 + 4.0)       # f1 read once, u2 a quarter-resolution 64 channels = 16 floats per pixel, the logit written
    lines = ["DISK dense against keypoint-only, %d images of %dx%d per step, top_k %d; median of %d rounds x %d steps, modes alternated; lib %s"
             % (B, W, H, K, args.rounds, args.steps, hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:12]),
             "kpb_net_forward   dense %.3f ms   keypoint-only %.3f ms   (rounds: %s / %s)" % (f["dense"][0], f["keypoint_only"][0], f["dense"][1], f["keypoint_only"][1]),
             "kpb_net_desc_at   %.3f ms for %d x %d points   (rounds: %s)" % (a["desc_at"][0], B, K, a["desc_at"][1]),
             "keypoint-only forward + desc_at %.3f ms against dense forward %.3f ms" % (f["keypoint_only"][0] + a["desc_at"][0], f["dense"][0]),
             "PairPipeline      dense %.1f pairs/s (%.3f ms/step)   keypoint-only %.1f pairs/s (%.3f ms/step)   matches per step %d / %d   (rounds: %s / %s)"
             % (args.pairs / p["dense"][0] * 1e3, p["dense"][0], args.pairs / p["keypoint_only"][0] * 1e3, p["keypoint_only"][0], matches["dense"], matches["keypoint_only"],
                p["dense"][1], p["keypoint_only"][1]),
             "kernels, dense forward (ms): %s" % json.dumps(k_dense),
             "kernels, keypoint-only forward (ms): %s" % json.dumps(k_sparse),
             "kernels, desc_at (ms): %s" % json.dumps(k_at),
             "disk_up3 (dense)   %.3f ms   %.1f GFLOP = %.3f of the f16 matrix peak at three MFMAs per product" % (up3_ms, dense_flop / 1e9, 3 * dense_flop / (up3_ms * 1e-3) / F16_DENSE_PEAK),
             "disk_up3_score     %.3f ms   %.2f GFLOP on the VALU (2 x 2 000 per pixel) and %.2f GB of input read once: %.3f of 8 TB/s"
             % (score_ms, score_flop / 1e9, score_bytes / 1e9, score_bytes / (score_ms * 1e-3) / HBM),
             "disk_desc_at       %.3f ms   <= %.2f GFLOP (8 K 2 000 128 per image) = %.4f of the f16 matrix peak at three MFMAs per product"
             % (at_ms, tap_flop / 1e9, 3 * tap_flop / (at_ms * 1e-3) / F16_DENSE_PEAK),
             "not carved / not allocated in keypoint-only mode: %.1f MB per image (feature map 129 floats + descriptor map 128 floats per pixel)" % (P * 257 * 4 / 1e6)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(text + "\n")


if __name__ == "__main__":
    main()
