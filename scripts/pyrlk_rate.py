#!/usr/bin/env python
"""Times kpb_lk_track_batch under KPB_OPT_LK_PYRLK (csrc/pyrlk.hip, the tracker behind optical_flow_cv: restated, cv2 parity unpinned) at the visual_odometer task's shape:
2000 points, 480 x 640, win 21, levels 3, C 3 -- one pair, and a chunk of 16 pairs in one call -- and, as a YARDSTICK ONLY (a different algorithm: fp32
windows, 40 fixed iterations a level, no status), the same shapes through the same entry without the option, with config_fund.yaml's parameters.

    python scripts/pyrlk_rate.py [--reps 200] [--warmup 10] [--out profiles/pyrlk_rate.json]

Every figure is device time between two events on the launch stream around `reps` back-to-back calls, after `warmup` calls of the same shape; the points are
seeded, spread over the image, and start 0 .. 3 px off; the frames are a synthetic pair.  One JSON line: ms per call and points per second, per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keypoint_bench_amd import synthetic                                        # noqa: E402
from keypoint_bench_amd.utils import matcher                                    # noqa: E402

H, W, K, WIN, LEVELS = 480, 640, 2000, 21, 3
LK = dict(distance=10, win_size=WIN, levels=LEVELS, interation=40, gray=False)  # config_fund.yaml's optical_flow_params


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pyrlk_rate.py measures on an MI355X; no device is visible")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    res = {"shape": [H, W], "points": K, "win_size": WIN, "levels": LEVELS, "C": 3, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for B in (1, 16):
        frames = np.stack([np.stack(synthetic.image_pair(50 + j, H, W)) for j in range(B)])        # [B, 2, 3, H, W]
        m1 = torch.from_numpy(np.ascontiguousarray(frames[:, 0])).to(dev)
        m2 = torch.from_numpy(np.ascontiguousarray(frames[:, 1])).to(dev)
        p1 = rng.uniform(0.05, 0.95, (B, K, 2)).astype(np.float32)
        p2 = (p1 + rng.uniform(-3, 3, (B, K, 2)) / np.array([W - 1, H - 1])).astype(np.float32)
        p1, p2 = torch.from_numpy(p1).to(dev), torch.from_numpy(p2).to(dev)
        ang = torch.from_numpy(rng.normal(size=(B, K)).astype(np.float32) * 6.28).to(dev)
        prm = {"win_size": WIN, "levels": LEVELS}
        _, status = matcher.optical_flow_cv_batch(m1, m2, p1, p2, None, prm)
        tracked = float((status == 1).float().mean())
        reps = a.reps if B == 1 else max(a.reps // 4, 1)
        ms = timed(lambda: matcher.optical_flow_cv_batch(m1, m2, p1, p2, None, prm), reps, a.warmup)
        ms_lk = timed(lambda: matcher.optical_flow_batch(m1, m2, p1, p2, None, LK, random_angle=ang), reps, a.warmup)
        res["cases"]["pairs_%d" % B] = {"pyrlk_ms": round(ms, 4), "pyrlk_points_per_s": round(B * K / ms * 1e3), "status_1_share": round(tracked, 4),
                                        "lk_track_batch_ms": round(ms_lk, 4), "lk_points_per_s": round(B * K / ms_lk * 1e3), "reps": reps}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
