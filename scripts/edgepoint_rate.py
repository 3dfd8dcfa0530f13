#!/usr/bin/env python3
"""EdgePoint (real checkpoint, tests/golden/edgepoint_state_dict.npz) under the batched PairPipeline: 640 x 480 pairs, nms_dist 6, top_k 1000, 256 pairs per
step (--pairs 16: R2D2's figure).  The score is a raw logit, so the pipeline detects with KPB_OPT_DETECT_SIGNED.

    python scripts/edgepoint_rate.py [--pairs 256] [--steps 10] [--warmup 3]            one JSON line: pairs/s from HIP events around the timed steps
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/edgepoint_rate.py --steps 3
    python scripts/edgepoint_rate.py --trace DIR [--pairs 256]                          per-kernel ms per step from that trace (a run of its own)

--distinct N synthetic pairs are generated and cycled to fill the batch (default 16: the host generates them one by one)."""
import argparse
import collections
import csv
import glob
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 8.0e12            # bytes/s, the chip's peak
H, W = 480, 640


def short(name):
    m = re.search(r"(\w+?)(<|\(|$)", name.replace("(anonymous namespace)::", "").replace("void ", ""))
    return m.group(1) if m else name[:40]


def from_trace(d, pairs, steps):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    last = [i for i, r in enumerate(rows) if "alike_block1" in r["Kernel_Name"]]
    last = last[-steps:]                # the forwards of the last `steps` steps: past allocation and warm-up
    ms, calls = collections.Counter(), collections.Counter()
    for r in rows[last[0]:]:
        n = short(r["Kernel_Name"])
        ms[n] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 / len(last)
        calls[n] += 1
    out = {"steps_read": len(last), "images_per_forward": 2 * pairs,
           "kernels_ms_per_step": {n: round(v, 4) for n, v in sorted(ms.items(), key=lambda kv: -kv[1])},
           "launches_per_step": {n: round(calls[n] / len(last), 2) for n in ms}, "total_ms_per_step": round(sum(ms.values()), 3)}
    if ms.get("edgepoint_score"):
        out["edgepoint_score_hbm_fraction"] = round(36.0 * H * W * 2 * pairs / (ms["edgepoint_score"] * 1e-3) / HBM, 4)      # 32 bytes read, 4 written per pixel
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(from_trace(args.trace, args.pairs, args.steps)))
        return
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    from keypoint_bench_amd.models.EdgePoint import EdgePoint
    from keypoint_bench_amd.pipeline import PairPipeline
    from edgepoint_fixtures import PARAM, checkpoint
    dev = "cuda:0"
    ep = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
    bf = dict(metric="euclidean", max_distance=5, cross_check=True)
    n = min(args.distinct, args.pairs)
    v = [synthetic.image_pair(5000 + i, H, W) for i in range(n)]
    pick = [i % n for i in range(args.pairs)]
    images = torch.from_numpy(np.concatenate([np.stack([v[i][0] for i in pick]), np.stack([v[i][1] for i in pick])])).to(dev)
    net = EdgePoint(PARAM)
    net.load_state_dict(checkpoint())
    pipe = PairPipeline(net.eval(), ep, bf, args.pairs, H, W, device=dev)
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
    print(json.dumps({"workload": "EdgePoint real checkpoint, %d pairs of %dx%d per step (%d distinct), nms_dist 6, top_k 1000, signed detection, brute-force matcher"
                                  % (args.pairs, W, H, n),
                      "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "pairs_per_s": round(args.pairs / ms * 1e3, 2),
                      "mean_keypoints": float(pipe.n.float().mean()), "mean_matches": float(pipe.k.float().mean()), "nms_reruns": pipe.reruns,
                      "lib_sha256": hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:12], "lib_path_override": os.environ.get("KPB_LIB_PATH")}))


if __name__ == "__main__":
    main()
