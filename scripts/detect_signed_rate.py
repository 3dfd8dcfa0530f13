#!/usr/bin/env python3
"""The signed round path (KPB_OPT_DETECT_SIGNED, csrc/detect.hip nms_round) against the default path on the same maps clamped at zero: 32 maps of
640 x 480 per call (the images of 16 pairs), nms_dist 6, border 8, top_k 1000, HIP events around the timed calls.

    python scripts/detect_signed_rate.py [--maps 32] [--steps 10] [--warmup 3] [--out profiles/detect_signed_rate.json]

The maps are smooth responses shifted below zero (sigmoid(36 z) - 0.5 of synthetic.score_smooth: about half of the pixels negative).  The two paths are two
functions -- the rounds stop by the reference's count rule, the default path takes the fixed point of the clamped map -- so their keypoint counts are
reported side by side, not compared."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 480, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    from keypoint_bench_amd.utils.extracter import detection_batch
    dev = "cuda:0"
    ep = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
    s = np.stack([synthetic.score_smooth(7000 + i, H, W) - np.float32(0.5) for i in range(args.maps)])[:, None]
    signed = torch.from_numpy(s).to(dev)
    clamped = signed.clamp(min=0.0).contiguous()

    def timed(x, flag):
        for _ in range(args.warmup):
            _, _, n = detection_batch(x, ep, signed=flag)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            _, _, n = detection_batch(x, ep, signed=flag)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps, float(n.float().mean())

    ms_r, n_r = timed(signed, True)
    ms_d, n_d = timed(clamped, False)
    out = {"workload": "%d maps of %dx%d per call, nms_dist 6, border 8, top_k 1000; synchronous kpb_detect" % (args.maps, W, H),
           "negative_fraction": round(float((s < 0).mean()), 4), "steps": args.steps, "warmup": args.warmup,
           "signed_rounds_ms_per_call": round(ms_r, 3), "default_on_clamped_ms_per_call": round(ms_d, 3),
           "mean_kps_signed_rounds": n_r, "mean_kps_default_on_clamped": n_d,
           "lib_sha256": hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:12]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
