#!/usr/bin/env python3
"""SFD2 (seeded stand-in weights, weights.random_sfd2_state_dict(17): the reference's sfd2.pth is not in its tree) under the batched PairPipeline: 640 x 480
pairs, nms_dist 6, top_k 1000, 16 pairs per step.

    python scripts/sfd2_rate.py [--pairs 16] [--steps 10] [--warmup 3] [--out profiles/sfd2_rate.json]

One JSON record: pairs/s from HIP events around the timed steps; per-layer ms of one forward of 2 x pairs images from the context's own profile (HIP events around
every launch, names sfd2_*) against each layer's split-f16 roof; and the grouped 3 x 3 layer (120 x 160 x 256 per image) in its two forms -- the split-f16 MFMA
kernel the library runs and the fp32 vector kernel of the strict path, timed the same way on the same images by a child process started with KPB_FP32_MATRIX=1
(the knob is read once per process; `--grouped-only` is that child's mode)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ROOF = 838.9e12         # split-f16 FLOP/s roof of DESIGN section 5
H, W = 480, 640
SEED = 17
# output resolution divisor of every layer of weights._SFD2_LAYERS
DIV = {"conv1a": 1, "conv1b": 2, "conv2a": 2, "conv2b": 4, "convPa0": 8, "convPa3": 8, "convPb": 8}


def layer_macs():
    from keypoint_bench_amd import weights
    out = {}
    for name, conv, bn, affine, (co, ci, k), bias in weights._SFD2_LAYERS:
        d = DIV.get(name, 4)
        out[name] = co * ci * k * k * (H // d) * (W // d)
    return out


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
    return {k[len("sfd2_"):]: v[1] / reps for k, v in rep.items() if k.startswith("sfd2_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--grouped-only", action="store_true", help="print the mean ms of the three grouped layers for 2 x pairs images and stop")
    args = ap.parse_args()
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    from keypoint_bench_amd.models.sfd2 import sfd2_random
    from keypoint_bench_amd.pipeline import PairPipeline
    dev = "cuda:0"
    ep = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
    bf = dict(metric="euclidean", max_distance=5, cross_check=True)
    v = [synthetic.image_pair(5000 + i, H, W) for i in range(args.pairs)]
    images = torch.from_numpy(np.concatenate([np.stack([a for a, _ in v]), np.stack([b for _, b in v])])).to(dev)
    net = sfd2_random(SEED)
    g = ("res0.c2", "res1.c2", "res2.c2")
    if args.grouped_only:
        t = profile_forward(net, images, _lib.Context.get(torch.device(dev)), 3)
        print("GROUPED_MS %.6f" % (sum(t[n] for n in g) / 3))
        return
    pipe = PairPipeline(net, ep, bf, args.pairs, H, W, device=dev)
    for _ in range(args.warmup):
        pipe.run(images)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        pipe.run(images)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    ctx = _lib.Context.get(torch.device(dev))
    n_img = 2 * args.pairs
    layers = profile_forward(net, images, ctx, 3)
    macs = layer_macs()
    roof = {n: round(2.0 * macs[n] * n_img / (layers[n] * 1e-3) / ROOF, 4) for n in macs if n in layers}
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--grouped-only", "--pairs", str(args.pairs)], env=dict(os.environ, KPB_FP32_MATRIX="1"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert child.returncode == 0 and "GROUPED_MS" in child.stdout, child.stdout
    valu_ms = float(child.stdout.split("GROUPED_MS")[-1].split()[0])
    rec = {"workload": "SFD2 seeded stand-in, %d pairs of %dx%d per step, nms_dist 6, top_k 1000, brute-force matcher" % (args.pairs, W, H),
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "pairs_per_s": round(args.pairs / ms * 1e3, 2),
           "mean_matches": float(pipe.k.float().mean()), "images_per_forward": n_img,
           "forward_ms": round(sum(layers.values()), 3), "kernels_ms": {n: round(t, 4) for n, t in layers.items()}, "roof_fraction": roof,
           "furthest_from_roof": min((n for n in roof if macs[n] * 100 > sum(macs.values())), key=lambda n: roof[n]),       # among layers with over 1 % of the work
           "gmac_per_image": round(sum(macs.values()) / 1e9, 2),
           "grouped_3x3_120x160x256": {"images": n_img, "mfma_split_f16_ms": round(sum(layers[n] for n in g) / 3, 4),
                                       "valu_fp32_ms": round(valu_ms, 4)},
           "lib_sha256": hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:12], "lib_path_override": os.environ.get("KPB_LIB_PATH")}
    text = json.dumps(rec)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
