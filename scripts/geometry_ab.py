#!/usr/bin/env python3
"""A/B partner for csrc/geometry.hip's three RANSAC kernels and recover_pose: runs whichever library KPB_LIB_PATH names (default: the tree's own)
through utils/mvg.py, so that two builds can be compared output bit for output bit and timing for timing, each in a fresh process:

    KPB_LIB_PATH=old/libkpb.so python scripts/geometry_ab.py dump old.npz        every output of every input below, as arrays
    KPB_LIB_PATH=old/libkpb.so python scripts/geometry_ab.py time old.json       device times of the seven workloads and their medians, one JSON line
    python scripts/geometry_ab.py compare old.npz new.npz old_1.json new_1.json old_2.json new_2.json      the verdict (no GPU), as profiles/geometry_ransac_ab.txt has it

Inputs.  (1) Every case of tests/geometry_cases.py, solo, through tests/test_gpu_geometry_edges.device -- the calls the edge tests make; an
essential-matrix case runs twice, through estimate_pose (R, t, recoverPose's mask and count) and through the two ABI calls that also hand out E
and the RANSAC mask.  (2) The timing workloads: 256 pairs x 1000 matches (the benchmark's pairs per step and top_k) of seeded synth / fscene /
scene scenes (tests/test_oracle_geometry.py) with inlier share 0.3 (long searches) and 0.7 (searches that stop early), for find_homography,
find_fundamental and estimate_pose, and 256 pairs x 14 matches for find_fundamental's least-median branch: seven in all.

time: per workload 3 warm-up calls, then 20 calls each between two events on the launch stream, one synchronise at the end, the median of the 20.
The mean hypothesis count info[2] of each workload is printed beside its time: it says how long the searches really ran.

compare: every array of the two dumps must be numpy.array_equal (NaNs in the same places count as equal; none occurs); per workload the two old runs'
40 calls and the two new runs' 40 calls are pooled and their medians compared: the new one is "no worse" when new - old <= |median(old_1) -
median(old_2)|, the old library's own spread between its two alternated runs.  Exit status 1 if an array differs or a workload is slower than that."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PAIRS, MATCHES, LMEDS_MATCHES = 256, 1000, 14


def workloads():
    """name -> (function of no arguments that runs the workload on the device and returns its outputs as a dict of tensors)"""
    import numpy as np
    import torch
    import geometry_cases as gc
    from keypoint_bench_amd.utils.mvg import estimate_pose, find_fundamental, find_homography
    from test_oracle_geometry import fscene, scene, synth
    dev = "cuda:0"

    def batch(cases):
        m0 = torch.from_numpy(np.stack([c["m0"] for c in cases])).to(dev)
        m1 = torch.from_numpy(np.stack([c["m1"] for c in cases])).to(dev)
        return m0, m1, np.arange(len(cases)) + 1

    def hf(fn, cases):
        m0, m1, seeds = batch(cases)
        return lambda: dict(zip(("model", "mask", "info"), fn(m0, m1, gc.SC, seeds=seeds)))

    def pose(cases):
        m0, m1, seeds = batch(cases)
        return lambda: dict(zip(("Rt", "mask_pose", "good", "info"), estimate_pose(m0, m1, gc.SC, gc.KC, gc.KC, seeds=seeds)))

    out = {}
    for share in (0.3, 0.7):
        tag = "%02d" % round(share * 10)
        out["h_" + tag] = hf(find_homography, [gc._case("H", *synth(MATCHES, share, 0.5, 100 + s)[:2], gc.SC, s) for s in range(PAIRS)])
        out["f_" + tag] = hf(find_fundamental, [gc._case("F", *fscene(MATCHES, share, 0.4, 200 + s)[:2], gc.SC, s) for s in range(PAIRS)])
        out["e_" + tag] = pose([gc._ecase(*scene(MATCHES, share, 0.3, 300 + s)[:2], gc.KC, gc.KC, gc.SC, s) for s in range(PAIRS)])
    out["f_lmeds"] = hf(find_fundamental, [gc._case("F", *fscene(LMEDS_MATCHES, 0.8, 0.4, 400 + s)[:2], gc.SC, s) for s in range(PAIRS)])
    return out


def dump(path):
    import numpy as np
    import torch
    import geometry_cases as gc
    import test_gpu_geometry_edges as edges
    arrays = {}
    for name in sorted(gc.BUILDERS):
        runs = [("", False)] + ([("raw.", True)] if gc.case(name)["kind"] == "E" else [])
        for tag, raw in runs:
            got = edges.device([name], raw=raw)[0]
            for k, v in got.items():
                arrays["case.%s.%s%s" % (name, tag, k)] = np.asarray(v)
    for name, run in workloads().items():
        for k, v in run().items():
            arrays["load.%s.%s" % (name, k)] = v.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(path, **arrays)
    print(json.dumps({"lib": os.environ.get("KPB_LIB_PATH") or "tree", "arrays": len(arrays), "cases": len(gc.BUILDERS), "file": path}))


def time_(path, warmup=3, steps=20):
    import numpy as np
    import torch
    stream = torch.cuda.current_stream(torch.device("cuda:0"))
    res = {"lib": os.environ.get("KPB_LIB_PATH") or "tree", "warmup": warmup, "steps": steps, "median_ms": {}, "mean_hypotheses": {}, "times_ms": {}}
    for name, run in workloads().items():
        for _ in range(warmup):
            got = run()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for e0, e1 in ev:
            e0.record(stream)
            run()
            e1.record(stream)
        torch.cuda.synchronize()
        res["times_ms"][name] = [round(e0.elapsed_time(e1), 4) for e0, e1 in ev]
        res["median_ms"][name] = round(float(np.median(res["times_ms"][name])), 4)
        res["mean_hypotheses"][name] = round(float(got["info"][:, 2].float().mean()), 1)
    line = json.dumps(res)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


def compare(old_npz, new_npz, old_1, new_1, old_2, new_2):
    import numpy as np
    a, b = np.load(old_npz), np.load(new_npz)
    keys = sorted(set(a.files) | set(b.files))
    differ = [k for k in keys if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k], equal_nan=True)]
    print("dumps: %d arrays in old, %d in new; arrays that differ: %d %s" % (len(a.files), len(b.files), len(differ), ", ".join(differ[:40])))
    print("verdict: %s" % ("DIFFER" if differ else "BIT-EQUAL"))
    t = {}
    for k, path in (("old_1", old_1), ("new_1", new_1), ("old_2", old_2), ("new_2", new_2)):
        with open(path) as f:
            t[k] = json.load(f)
    print("\nmedian ms of 20 timed calls (3 warm-up), run order old_1, new_1, old_2, new_2; old / new: median of a library's 40 pooled calls")
    print("%-8s %9s %9s %9s %9s | %9s %9s | %8s %8s  %-9s hypotheses" % ("workload", "old_1", "new_1", "old_2", "new_2", "old", "new", "new-old", "spread", "verdict"))
    slower = []
    for w in t["old_1"]["median_ms"]:
        m = {k: t[k]["median_ms"][w] for k in t}
        old = float(np.median(t["old_1"]["times_ms"][w] + t["old_2"]["times_ms"][w]))
        new = float(np.median(t["new_1"]["times_ms"][w] + t["new_2"]["times_ms"][w]))
        spread = abs(m["old_1"] - m["old_2"])
        ok = new - old <= spread
        slower += [] if ok else [w]
        print("%-8s %9.4f %9.4f %9.4f %9.4f | %9.4f %9.4f | %+8.4f %8.4f  %-9s %s / %s" % (w, m["old_1"], m["new_1"], m["old_2"], m["new_2"], old, new, new - old, spread,
              "no worse" if ok else "SLOWER", t["old_1"]["mean_hypotheses"][w], t["new_1"]["mean_hypotheses"][w]))
    sys.exit(1 if differ or slower else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["dump", "time", "compare"])
    ap.add_argument("out", nargs="+")
    args = ap.parse_args()
    {"dump": dump, "time": time_, "compare": compare}[args.mode](*args.out)


if __name__ == "__main__":
    main()
