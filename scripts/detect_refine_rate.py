#!/usr/bin/env python3
"""Sub-pixel refinement (KPB_OPT_DETECT_REFINE): what refine_kps costs and what it does to the localisation metrics, in ONE process on one MI355X.

    python scripts/detect_refine_rate.py [--maps 512] [--rounds 5] [--steps 3] [--pairs 32] [--out profiles/detect_refine.txt]

1. Cost, at the BASELINE detection workload: --maps score maps of 640 x 480 (ALIKE-t on 16 synthetic pairs, the 32 maps repeated), nms_dist 6, border 8, top_k 1 000, one
   kpb_detect call per step.  Per mode (off, quadratic, softargmax): the whole call between device events (median over --rounds rounds of --steps steps, the modes
   alternated), and the per-call time of every kernel of the call from the context's own profile (kpb_prof_enable: events around every launch) -- refine_kps beside
   nms_sweep and select_topk from the same run.
2. Effect, reported and not gated: ALIKE-t (packaged weights) on --pairs pairs of the graded viewpoint family (synthetic.warped_pair x viewpoint_case, ground-truth
   homography known), the repeatability task's repeatability / mean_error (th 3) and MHA's hits at 3 / 5 / 7 px with the mean corner error of the pairs that found a
   homography, through the drop-in task functions, per mode."""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 480, 640
EP = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
BF = dict(metric="euclidean", max_distance=5, cross_check=True)
TH = [3, 5, 7]
MODES = (None, "quadratic", "softargmax")


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


def cost(args, lines):
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    from keypoint_bench_amd.models.ALike import alike_t
    from keypoint_bench_amd.utils.extracter import detection_batch
    dev = torch.device("cuda:0")
    net = alike_t().eval()
    maps = []
    for i in range(16):
        for v in synthetic.image_pair(5000 + i, H, W):
            maps.append(net(torch.from_numpy(v)[None].to(dev))[0])
    x = torch.cat(maps).repeat((args.maps + 31) // 32, 1, 1, 1)[: args.maps].contiguous()
    ctx = _lib.Context.get(dev)
    calls = {m: (lambda m=m: detection_batch(x, dict(EP, refine=m))) for m in MODES}
    for f in calls.values():
        for _ in range(2):
            f()
    ms = {m: [] for m in MODES}
    for _ in range(args.rounds):
        for m, f in calls.items():
            ms[m].append(timed(f, args.steps))
    kernels = {}
    for m, f in calls.items():
        torch.cuda.synchronize()
        ctx.prof_enable(True)
        try:
            ctx.prof_report()
            for _ in range(args.steps):
                f()
            torch.cuda.synchronize()
            kernels[m] = {k: (v[0] / args.steps, round(v[1] / args.steps, 4)) for k, v in ctx.prof_report().items()}
        finally:
            ctx.prof_enable(False)
    n = detection_batch(x, EP)[2]
    lines.append("kpb_detect on %d maps of %dx%d (ALIKE-t scores), nms_dist 6, border 8, top_k 1000: %.0f rows per map; median of %d rounds x %d steps, modes alternated"
                 % (args.maps, W, H, float(n.float().mean()), args.rounds, args.steps))
    for m in MODES:
        lines.append("  refine %-10s whole call %.3f ms   (rounds: %s)" % (m or "off", statistics.median(ms[m]), [round(v, 3) for v in ms[m]]))
    lines.append("per-kernel time per call under kpb_prof_enable, ms (launches per call):")
    for m in MODES:
        lines.append("  refine %-10s %s" % (m or "off", "   ".join("%s %.4f (%g)" % (k, v[1], v[0]) for k, v in sorted(kernels[m].items()))))
    sel = kernels[None]["select_topk"][1]
    for m in MODES[1:]:
        r = kernels[m]["refine_kps"][1]
        lines.append("  refine_kps (%s) %.4f ms = %.2f x select_topk (%.4f ms), %.3f x nms_sweep (%.4f ms)"
                     % (m, r, r / kernels[m]["select_topk"][1], sel, r / kernels[m]["nms_sweep"][1], kernels[m]["nms_sweep"][1]))
    del x
    torch.cuda.empty_cache()


def effect(args, lines):
    import numpy as np
    import torch
    from keypoint_bench_amd import synthetic
    from keypoint_bench_amd.models.ALike import alike_t
    from keypoint_bench_amd.tasks.MHA import corner_hits
    from keypoint_bench_amd.tasks.repeatability import val_key_points
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import brute_force_matcher
    from keypoint_bench_amd.utils.mvg import find_homography
    from keypoint_bench_amd.utils.projection import warp
    dev = "cuda:0"
    net = alike_t().eval()
    t = lambda a: torch.from_numpy(a).to(dev)
    rows = {m: [] for m in MODES}
    for i in range(args.pairs):
        v0, v1, h01 = synthetic.warped_pair(i, H, W, *synthetic.viewpoint_case(i))
        h10 = np.linalg.inv(h01.astype(np.float64)).astype(np.float32)
        s0, d0 = net(t(v0)[None])
        s1, d1 = net(t(v1)[None])
        s0, d0, s1, d1 = s0.clone(), d0.clone(), s1.clone(), d1.clone()
        w01 = dict(mode="homo", homography_matrix=t(h01), width=torch.tensor(W), height=torch.tensor(H))
        w10 = dict(mode="homo", homography_matrix=t(h10), width=torch.tensor(W), height=torch.tensor(H))
        for m in MODES:
            ep = dict(EP, refine=m)
            k0, k1 = detection(s0, ep), detection(s1, ep)
            rep = val_key_points(k0, k1, w01, w10, th=3)
            c0, c1 = warp(k0, w01)[0], warp(k1, w10)[0]
            flags, dist, nm = [0.0] * len(TH), float("nan"), 0
            if c0.shape[0] and c1.shape[0]:
                m0, m1 = brute_force_matcher(c0, c1, d0, d1, BF)
                nm = int(m0.shape[0])
                if nm >= 4:
                    Hm, _, info = find_homography(m0[:, 0:2], m1[:, 0:2], [W - 1, H - 1, W - 1, H - 1], seed=0)
                    if int(info[0, 0]):
                        flags, dist = corner_hits(Hm[0].cpu().numpy(), h01, np.asarray(H), np.asarray(W), H, W, TH)
            rows[m].append(dict(rep=float(rep["repeatability"]), err=float(rep["mean_error"]), flags=[float(f) for f in flags], dist=float(dist), matches=nm))
    lines.append("ALIKE-t (packaged weights) on %d pairs of synthetic.warped_pair x viewpoint_case at %dx%d, nms_dist 6, top_k 1000, th 3 / MHA th %s (reported, not gated):" % (args.pairs, W, H, TH))
    good = [i for i in range(args.pairs) if all(np.isfinite(rows[m][i]["dist"]) and rows[m][i]["dist"] < 50 for m in MODES)]
    for m in MODES:
        r = rows[m]
        lines.append("  refine %-10s repeatability %.4f   mean_error %.4f px   MHA@3/5/7 %s   matches/pair %.1f   mean corner error %.4f px, median %.4f px (the %d pairs every mode solved)"
                     % (m or "off", np.mean([q["rep"] for q in r]), np.nanmean([q["err"] for q in r]), ["%.4f" % np.mean([q["flags"][j] for q in r]) for j in range(len(TH))],
                        np.mean([q["matches"] for q in r]), np.mean([r[i]["dist"] for i in good]), np.median([r[i]["dist"] for i in good]), len(good)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None, help="the per-pair rows of part 2")
    args = ap.parse_args()
    from keypoint_bench_amd import _lib
    lines = ["sub-pixel refinement of kpb_detect's rows (KPB_OPT_DETECT_REFINE); lib %s" % hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:12]]
    cost(args, lines)
    rows = effect(args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(text + "\n")
    if args.json:
        with open(args.json, "w") as fo:
            json.dump({str(k): v for k, v in rows.items()}, fo)


if __name__ == "__main__":
    main()
