#!/usr/bin/env python3
"""R2D2's two matrix modes (Quad_L2Net_ConfCFS(matrix="split" | "f16")) side by side, in ONE process on one MI355X, real checkpoint (tests/golden/r2d2_state_dict*.npz).

    python scripts/r2d2_matrix_modes.py [--pairs 16] [--rounds 7] [--steps 3] [--effect-pairs 32] [--out profiles/r2d2_matrix_modes.txt]

1. Forward: 2 x --pairs images of 640 x 480 through each net, between device events; every shape warmed up first, then --rounds rounds of --steps forwards per mode,
   the modes ALTERNATED round by round.  Reported per mode: the median round, every round, and the spread (max - min of its rounds) a difference has to exceed.
2. Per-kernel ms of one forward of each mode from the context's own profile (kpb_prof_enable: events around every launch; the f16 net's kernels carry the
   suffix _h1), with the ratio split / f16 per layer.
3. Effect, reported and not gated: both nets on --effect-pairs pairs of the graded viewpoint family (synthetic.warped_pair x viewpoint_case, ground-truth homography
   known), nms_dist 6, top_k 1000: the repeatability task's repeatability / mean_error (th 3), MHA's hits at 3 / 5 / 7 px, matches per pair.
(The pipeline's pairs/s, and the split mode on another build of the library, come from scripts/r2d2_rate.py --matrix ..., one process per figure.)"""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
H, W = 480, 640
EP = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
BF = dict(metric="euclidean", max_distance=5, cross_check=True)
TH = [3, 5, 7]
MODES = ("split", "f16")


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


def forward(args, nets, lines):
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    dev = "cuda:0"
    v = [synthetic.image_pair(5000 + i, H, W) for i in range(args.pairs)]
    images = torch.from_numpy(np.concatenate([np.stack([a for a, _ in v]), np.stack([b for _, b in v])])).to(dev)
    for m in MODES:
        for _ in range(3):
            nets[m](images)
    rounds = {m: [] for m in MODES}
    for _ in range(args.rounds):
        for m in MODES:
            rounds[m].append(timed(lambda: nets[m](images), args.steps))
    lines.append("forward of %d images of %dx%d, ms; median of %d rounds x %d forwards, modes alternated" % (2 * args.pairs, W, H, args.rounds, args.steps))
    med = {m: statistics.median(rounds[m]) for m in MODES}
    for m in MODES:
        lines.append("  matrix %-5s %.3f ms   spread %.3f   (rounds: %s)" % (m, med[m], max(rounds[m]) - min(rounds[m]), [round(r, 3) for r in rounds[m]]))
    lines.append("  split / f16 = %.3f; GFLOP per image 296.9: split %.1f TFLOP/s, f16 %.1f TFLOP/s" % (med["split"] / med["f16"], 296.9 * 2 * args.pairs / med["split"], 296.9 * 2 * args.pairs / med["f16"]))
    ctx = _lib.Context.get(torch.device(dev))
    ctx.prof_enable(True)
    per = {}
    for m in MODES:
        ctx.prof_report()
        for _ in range(args.steps):
            nets[m](images)
        torch.cuda.synchronize()
        per[m] = {k[5:] if k.startswith("r2d2_") else k: ms / args.steps for k, (n, ms) in ctx.prof_report().items() if k.startswith(("r2d2_", "conv"))}
    ctx.prof_enable(False)
    lines.append("per-kernel ms per forward under kpb_prof_enable (%d images):" % (2 * args.pairs))
    for name in ["conv%d" % i for i in range(9)] + ["head"]:
        a, b = per["split"].get(name), per["f16"].get(name + "_h1", per["f16"].get(name))
        lines.append("  %-6s split %8.3f   f16 %8.3f   split / f16 %.2f" % (name, a, b, a / b))
    lines.append("  sum    split %8.3f   f16 %8.3f" % (sum(per["split"].values()), sum(per["f16"].values())))
    return med, per


def effect(args, nets, lines):
    import numpy as np
    import torch
    from keypoint_bench_amd import synthetic
    from keypoint_bench_amd.tasks.MHA import corner_hits
    from keypoint_bench_amd.tasks.repeatability import val_key_points
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import brute_force_matcher
    from keypoint_bench_amd.utils.mvg import find_homography
    from keypoint_bench_amd.utils.projection import warp
    dev = "cuda:0"
    t = lambda a: torch.from_numpy(a).to(dev)
    rows = {m: [] for m in MODES}
    for i in range(args.effect_pairs):
        v0, v1, h01 = synthetic.warped_pair(i, H, W, *synthetic.viewpoint_case(i))
        h10 = np.linalg.inv(h01.astype(np.float64)).astype(np.float32)
        w01 = dict(mode="homo", homography_matrix=t(h01), width=torch.tensor(W), height=torch.tensor(H))
        w10 = dict(mode="homo", homography_matrix=t(h10), width=torch.tensor(W), height=torch.tensor(H))
        for m in MODES:
            s0, d0 = nets[m](t(v0)[None])
            s0, d0 = s0.clone(), d0.clone()
            s1, d1 = nets[m](t(v1)[None])
            k0, k1 = detection(s0, EP), detection(s1, EP)
            rep = val_key_points(k0, k1, w01, w10, th=3)
            c0, c1 = warp(k0, w01)[0], warp(k1, w10)[0]
            flags, nm = [0.0] * len(TH), 0
            if c0.shape[0] and c1.shape[0]:
                m0, m1 = brute_force_matcher(c0, c1, d0, d1, BF)
                nm = int(m0.shape[0])
                if nm >= 4:
                    Hm, _, info = find_homography(m0[:, 0:2], m1[:, 0:2], [W - 1, H - 1, W - 1, H - 1], seed=0)
                    if int(info[0, 0]):
                        flags, _ = corner_hits(Hm[0].cpu().numpy(), h01, np.asarray(H), np.asarray(W), H, W, TH)
            rows[m].append(dict(rep=float(rep["repeatability"]), err=float(rep["mean_error"]), flags=[float(f) for f in flags], matches=nm))
    lines.append("R2D2 (reference checkpoint) on %d pairs of synthetic.warped_pair x viewpoint_case at %dx%d, nms_dist 6, top_k 1000, th 3 / MHA th %s (reported, not gated):"
                 % (args.effect_pairs, W, H, TH))
    for m in MODES:
        r = rows[m]
        lines.append("  matrix %-5s repeatability %.4f   mean_error %.4f px   MHA@3/5/7 %s   matches/pair %.1f"
                     % (m, np.mean([q["rep"] for q in r]), np.nanmean([q["err"] for q in r]), ["%.4f" % np.mean([q["flags"][j] for q in r]) for j in range(len(TH))],
                        np.mean([q["matches"] for q in r])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--effect-pairs", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from keypoint_bench_amd import _lib
    from keypoint_bench_amd.models.r2d2 import from_checkpoint
    from r2d2_fixtures import checkpoint
    nets = {m: from_checkpoint(checkpoint(), matrix=m) for m in MODES}
    lines = ["R2D2 matrix modes: split (three f16 MFMAs per product) and f16 (one); lib %s" % hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:12]]
    forward(args, nets, lines)
    if args.effect_pairs:
        effect(args, nets, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
