#!/usr/bin/env python3
"""The brute-force matcher (csrc/match.hip: kpb_match_ratio under every KPB_OPT_MATCH_METRIC) at the benchmark's match shape -- 256 pairs of 1000 x 1000 descriptors of
64 channels, resident in HBM -- for every metric, with the prefilter on (the default from 8 pairs up) and off (KPB_MATCH_PREFILTER=0: match_tile alone).
Prints ms per 256 pairs: the call time between two events on the launch stream (profiling off), the best of the timed windows of a process, for
each round.

The library reads KPB_MATCH_PREFILTER once per process, so every setting runs in a fresh child python, one at a time, and the two settings
ALTERNATE over --rounds rounds: the spread between the rounds of one setting is the noise a difference between settings has to exceed.  A child
also prints the match count and a checksum of its index pairs and distance bits per metric; the parent refuses to report two settings whose
results differ.  Euclidean is the context as it comes -- the code path of every release before the metrics -- and is the yardstick.

    python scripts/match_metric_rate.py [--pairs 256] [--n 1000] [--channels 64] [--steps 20] [--warmup 3] [--rounds 2] [--max-ratio 1.0]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/match_metric_rate.py --child --steps 5      (kernel times: a run of its own)

The descriptors are seeded: a normal, half of b's rows noisy copies (sigma 0.05) of distinct rows of a, the rest normal -- the layout of
tests/match_cases.noisy_pair at the benchmark's size."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import torch
    from keypoint_bench_amd._lib import METRICS, Context, MatchParams, ptr
    dev = torch.device("cuda:0")
    B, N, C = args.pairs, args.n, args.channels
    g = torch.Generator(device=dev).manual_seed(1234)
    a = torch.randn((B, N, C), device=dev, generator=g)
    b = torch.randn((B, N, C), device=dev, generator=g)
    perm = torch.stack([torch.randperm(N, device=dev, generator=g)[: N // 2] for _ in range(B)])
    b[:, : N // 2] = torch.gather(a, 1, perm[:, :, None].expand(-1, -1, C)) + 0.05 * torch.randn((B, N // 2, C), device=dev, generator=g)
    ctx = Context.get(dev)
    pairs = torch.empty((B, N, 2), dtype=torch.int32, device=dev)
    dist = torch.empty((B, N), dtype=torch.float64, device=dev)
    k = torch.empty((B,), dtype=torch.int32, device=dev)
    prm = MatchParams(float("inf"), 1)
    head = (ctx.handle, ptr(a), ptr(b), B, C, N, N, ptr(None), ptr(None), ctypes.byref(prm))
    tail = (ptr(pairs), ptr(dist), ptr(k))
    stream = torch.cuda.current_stream(dev)
    out = {}
    for name, mid in METRICS.items():
        ctx.set_option(Context.OPT_MATCH_METRIC, mid)
        call = lambda: ctx.check(ctx.lib.kpb_match_ratio(*head, args.max_ratio, *tail))
        best = None
        for _ in range(2):
            for _ in range(args.warmup):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                call()
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1) / args.steps
            best = ms if best is None else min(best, ms)
        kk = k.cpu().long()
        mask = torch.arange(N)[None, :] < kk[:, None]
        p = pairs.cpu().long()
        bits = dist.cpu().view(torch.int64)
        check = int(((p[:, :, 0] * 1000003 + p[:, :, 1] * 7919 + (bits & 0xFFFFFFFF) + (bits >> 32)) * mask).sum().item())
        out[name] = {"ms": round(best, 4), "matches": int(kk.sum()), "checksum": check}
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-ratio", type=float, default=1.0)
    ap.add_argument("--child", action="store_true", help="measure in this process under the environment as it is")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    runs = {"on": [], "off": []}
    for _ in range(args.rounds):
        for setting, value in (("on", "1"), ("off", "0")):          # alternate: a fresh child (never an exec of a GPU process) per setting and round
            p = subprocess.run(cmd, env=dict(os.environ, KPB_MATCH_PREFILTER=value), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            lines = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                sys.exit("child with KPB_MATCH_PREFILTER=%s failed (exit %d):\n%s" % (value, p.returncode, "\n".join(p.stdout.splitlines()[-20:])))
            runs[setting].append(json.loads(lines[-1][7:]))
    table = {}
    for name in runs["on"][0]:
        seen = {(r[name]["matches"], r[name]["checksum"]) for s in runs.values() for r in s}
        if len(seen) != 1:
            sys.exit("%s: the settings or rounds disagree on the result: %r" % (name, sorted(seen)))
        on, off = [r[name]["ms"] for r in runs["on"]], [r[name]["ms"] for r in runs["off"]]
        table[name] = {"prefilter_on_ms": min(on), "prefilter_off_ms": min(off), "on_rounds": on, "off_rounds": off, "matches": runs["on"][0][name]["matches"]}
    print(json.dumps({"pairs": args.pairs, "shape": [args.n, args.n, args.channels], "steps": args.steps, "max_ratio": args.max_ratio,
                      "ms_per_%d_pairs" % args.pairs: table}))


if __name__ == "__main__":
    main()
