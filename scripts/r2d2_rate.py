#!/usr/bin/env python3
"""R2D2 (real checkpoint, tests/golden/r2d2_state_dict*.npz) under the batched PairPipeline: 640 x 480 pairs, nms_dist 6, top_k 1000, 16 pairs per step.

    python scripts/r2d2_rate.py [--pairs 16] [--steps 10] [--warmup 3] [--matrix split|f16]     one JSON line: pairs/s from HIP events around the timed steps,
                                                                                        the net's forward alone (ms per 2 x pairs images) and, with --prof, the
                                                                                        per-kernel ms of one forward under kpb_prof_enable
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/r2d2_rate.py --steps 3
    python scripts/r2d2_rate.py --trace DIR [--pairs 16]                                per-layer ms and fraction of the split-f16 roof from that trace

The layers share kernels (conv6 .. 8 are one gemm_h instance), so the trace is read by launch order: the ten launches behind every conv_rgb32 (conv0; ALIKE-l's
first layer is the same kernel, so a run also has to end in r2d2_head)."""
import argparse
import csv
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ROOF = 838.9e12         # split-f16 FLOP/s roof of DESIGN section 5
H, W = 480, 640


def from_trace(d, pairs):
    from keypoint_bench_amd import weights
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    names = ["conv0"] + [p[0] for p in weights.R2D2_PLAN[1:]] + ["head"]
    runs = [i for i, r in enumerate(rows) if "conv_rgb32" in r["Kernel_Name"] and i + 10 < len(rows) and "r2d2_head" in rows[i + 10]["Kernel_Name"]]
    runs = runs[len(runs) // 2:]       # the later half: past allocation and the pipeline's placement probes
    ms = {n: sum((int(rows[i + k]["End_Timestamp"]) - int(rows[i + k]["Start_Timestamp"])) for i in runs) / len(runs) / 1e6 for k, n in enumerate(names)}
    out = {"forwards_read": len(runs), "images_per_forward": 2 * pairs, "kernels_ms": {n: round(v, 4) for n, v in ms.items()},
           "kernel_of": {n: rows[runs[0] + k]["Kernel_Name"][:60] for k, n in enumerate(names)}, "roof_fraction": {}}
    for name, cin, cout, k, dil, bn, relu in weights.R2D2_PLAN:
        flop = 2.0 * cin * cout * k * k * H * W * 2 * pairs
        out["roof_fraction"][name] = round(flop / (ms[name] * 1e-3) / ROOF, 4)
    convs = sum(ms[p[0]] for p in weights.R2D2_PLAN)
    out["convs_ms"] = round(convs, 4)
    out["convs_roof_fraction"] = round(2.0 * 483168 * H * W * 2 * pairs / (convs * 1e-3) / ROOF, 4)
    out["furthest_from_roof"] = min((p[0] for p in weights.R2D2_PLAN[1:]), key=lambda n: out["roof_fraction"][n])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--matrix", choices=("split", "f16"), default="split", help="the net's matrix mode (Quad_L2Net_ConfCFS(matrix=...))")
    ap.add_argument("--prof", action="store_true", help="per-kernel ms of one forward (kpb_prof_enable) after the timed steps")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(from_trace(args.trace, args.pairs)))
        return
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    from keypoint_bench_amd.models.r2d2 import from_checkpoint
    from keypoint_bench_amd.pipeline import PairPipeline
    from r2d2_fixtures import checkpoint
    dev = "cuda:0"
    ep = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
    bf = dict(metric="euclidean", max_distance=5, cross_check=True)
    v = [synthetic.image_pair(5000 + i, H, W) for i in range(args.pairs)]
    images = torch.from_numpy(np.concatenate([np.stack([a for a, _ in v]), np.stack([b for _, b in v])])).to(dev)
    net = from_checkpoint(checkpoint(), matrix=args.matrix) if args.matrix != "split" else from_checkpoint(checkpoint())
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
    fwd = []        # the forward alone, on a net of its own (the pipeline keeps its net's outputs)
    solo = from_checkpoint(checkpoint(), matrix=args.matrix) if args.matrix != "split" else from_checkpoint(checkpoint())
    for i in range(args.warmup + args.steps):
        e0.record()
        solo(images)
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            fwd.append(e0.elapsed_time(e1))
    kernels = None
    if args.prof:
        ctx = _lib.Context.get(torch.device(dev))
        ctx.prof_enable(True)
        ctx.prof_report()
        solo(images)
        torch.cuda.synchronize()
        kernels = {k: round(v[1], 4) for k, v in sorted(ctx.prof_report().items()) if k.startswith(("r2d2_", "conv"))}
        ctx.prof_enable(False)
    print(json.dumps({"matrix": args.matrix, "forward_ms": round(sum(fwd) / len(fwd), 3), "forward_ms_min_max": [round(min(fwd), 3), round(max(fwd), 3)],
                      "kernels_ms": kernels, "workload": "R2D2 real checkpoint, %d pairs of %dx%d per step, nms_dist 6, top_k 1000, brute-force matcher" % (args.pairs, W, H),
                      "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "pairs_per_s": round(args.pairs / ms * 1e3, 2),
                      "mean_matches": float(pipe.k.float().mean()), "lib_sha256": hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:12],
                      "lib_path_override": os.environ.get("KPB_LIB_PATH")}))


if __name__ == "__main__":
    main()
