#!/usr/bin/env python3
"""GoodPoint (real checkpoint, tests/golden/goodpoint_state_dict.npz) and the batched Lucas-Kanade tracker, measured with HIP events and the library's
own per-kernel profile (kpb_prof_report) -- no outside tool, nothing outside the repository.

  forward   512 images of 480 x 640 per call: ms per call; alike_block1 (+ amax_reduce) and goodpoint_head apart; the head's fraction of 8 TB/s on its
            48 bytes per pixel (32 read, 4 + 12 written).
  sequence  F = 64 frames of 480 x 640 through SequencePipeline(track=...) with config_fund.yaml's parameters (nms_dist 6, top_k 1000, tracker
            distance 10, window 21, 3 levels, 40 iterations): frames/s; kpb_lk_track_batch's share of a chunk (its kernels' profile); and F single
            kpb_lk_track calls on the same maps made planar with the same keypoints -- the way the frames were tracked before the batch entry, and the
            figure it is measured against.

    python scripts/goodpoint_rate.py [--images 512] [--frames 64] [--steps 5] [--warmup 2] [--out profiles/goodpoint_rate.json]"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 8.0e12            # bytes/s, the chip's peak
H, W = 480, 640
LK_KERNELS = ("lk_init", "lk_avgpool", "lk_sobel", "lk_level", "lk_finish")


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


def profiled(ctx, fn, steps):
    """{kernel: ms per call of fn} from the library's event pairs around every launch (a pass of its own: the events cost time between kernels)."""
    ctx.sync()
    ctx.prof_enable(True)
    try:
        ctx.prof_report()
        for _ in range(steps):
            fn()
        ctx.sync()
        rep = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
    return {k: round(ms / steps, 4) for k, (_, ms) in sorted(rep.items(), key=lambda kv: -kv[1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    from keypoint_bench_amd._lib import Context, LkParams, ptr
    from keypoint_bench_amd.models.GoodPoint import GoodPoint
    from keypoint_bench_amd.pipeline import SequencePipeline
    from goodpoint_fixtures import PARAM, checkpoint
    dev = "cuda:0"
    net = GoodPoint(PARAM)
    net.load_state_dict(checkpoint())
    net.eval()
    ctx = Context.get(torch.device(dev))
    out = {"lib_sha256": hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:12], "steps": args.steps, "warmup": args.warmup,
           "fp32_matrix": os.environ.get("KPB_FP32_MATRIX") == "1"}

    # ---- forward
    B = args.images
    n = min(args.distinct, B)
    v = [synthetic.image_pair(5000 + i, H, W)[i & 1] for i in range(n)]
    images = torch.from_numpy(np.stack([v[i % n] for i in range(B)])).to(dev)
    net._ensure(images.device)
    score = torch.empty((B, 1, H, W), device=dev)
    desc = torch.empty((B, H, W, 3), device=dev)
    fwd = lambda: ctx.check(ctx.lib.kpb_net_forward(net._handle, ptr(images), B, H, W, ptr(score), ptr(desc)))
    ms = timed(fwd, args.steps, args.warmup)
    k = profiled(ctx, fwd, args.steps)
    out["forward"] = {"workload": "GoodPoint real checkpoint, %d images of %dx%d per call (%d distinct)" % (B, W, H, n), "ms_per_call": round(ms, 3),
                      "images_per_s": round(B / ms * 1e3, 1), "kernels_ms_per_call": k,
                      "goodpoint_head_hbm_fraction": round(48.0 * H * W * B / (k["goodpoint_head"] * 1e-3) / HBM, 4)}
    del images, score, desc
    torch.cuda.empty_cache()

    # ---- sequence
    F = args.frames
    canvas, _ = synthetic.image_pair(300, H + 2 * F + 8, W + 2 * F + 8)
    frames = torch.from_numpy(np.stack([canvas[:, i:i + H, 2 * i:2 * i + W] for i in range(F)]).astype(np.float32)).to(dev)
    ep = dict(nms_dist=6, threshold=0.0, border_dist=8, top_k=1000, min_score=0.0)
    track = dict(distance=10, win_size=21, levels=3, interation=40, gray=False)
    pipe = SequencePipeline(net, ep, None, F, H, W, device=dev, track=track)
    K = pipe.top_k
    angles = torch.from_numpy((np.random.default_rng(7).normal(size=(F, K)) * 6.28).astype(np.float32)).to(dev)
    pipe.run(frames, first=True, angles=angles)
    chunk = lambda: pipe.run(frames, first=False, angles=angles)        # steady state: slot 0 carries the chunk before
    ms = timed(chunk, args.steps, args.warmup)
    k = profiled(ctx, chunk, args.steps)
    lk_ms = sum(k.get(name, 0.0) for name in LK_KERNELS)
    # the same maps, keypoints and angles through F single calls (planar copies made beforehand, counts read back beforehand)
    maps = pipe.maps.contiguous()                                       # [F + 1, 3, H, W] planar
    counts = pipe.n[:F].tolist()
    pts = pipe.kps[:F].clone()
    unit = torch.stack([torch.cos(angles), torch.sin(angles)], dim=2).contiguous()
    o1, e1 = torch.empty((F, K, 2), device=dev), torch.empty((F, K), device=dev)
    prm = LkParams(float(track["distance"]), track["win_size"], track["levels"], track["interation"])

    def singles():
        for j in range(F):
            ctx.check(ctx.lib.kpb_lk_track(ctx.handle, ptr(maps[j]), ptr(maps[j + 1]), 3, H, W, ptr(pts[j]), ptr(pts[j]), 3, ptr(unit[j]), counts[j],
                                           ctypes.byref(prm), ptr(o1[j]), ptr(e1[j])))

    def batch():
        ctx.check(ctx.lib.kpb_lk_track_batch(ctx.handle, ptr(pipe.maps), ptr(pipe.maps[1:]), F, 3, H, W, *pipe.maps.stride(), ptr(pts), ptr(pts), 3,
                                             ptr(unit), K, ptr(pipe.n), ctypes.byref(prm), ptr(pipe.tracked), ptr(pipe.track_err)))

    ms_single = timed(singles, args.steps, args.warmup)
    ms_batch = timed(batch, args.steps, args.warmup)
    same = all(torch.equal(o1[j, :counts[j]], pipe.tracked[j, :counts[j]]) for j in range(F))
    out["sequence"] = {"workload": "GoodPoint, %d frames of %dx%d per chunk, nms_dist 6, top_k 1000, tracker 10/21/3/40 on the net's maps" % (F, W, H),
                       "ms_per_chunk": round(ms, 3), "frames_per_s": round(F / ms * 1e3, 1), "mean_keypoints": float(pipe.n[:F].float().mean()),
                       "kernels_ms_per_chunk": k, "lk_kernels_ms_per_chunk": round(lk_ms, 3), "lk_share_of_kernel_time": round(lk_ms / sum(k.values()), 4),
                       "lk_track_batch_ms": round(ms_batch, 3), "lk_track_single_calls_ms": round(ms_single, 3),
                       "batch_speedup_over_single_calls": round(ms_single / ms_batch, 3), "batch_rows_equal_single_rows": bool(same)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
