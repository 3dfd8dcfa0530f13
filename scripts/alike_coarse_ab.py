#!/usr/bin/env python3
"""Interleaved A/B of KPB_OPT_ALIKE_COARSE_FUSED inside ONE process and ONE library (include/kpb.h): arm A = 0, conv2 of ALIKE's blocks 3 / 4 followed by
maxpool4_x3, conv1x1_agg3 and conv1x1_agg4 (seven launches); arm B = 1, the blocks finished in conv2's epilogue (four launches).
    python scripts/alike_coarse_ab.py [--sparse] [--rounds 4] [--steps 40]          (GPU box; prints the record, profiles/alike_coarse_tail_ab.txt keeps it)
One PairPipeline at bench.py's batch (256 pairs) on bench.py's seeded images; the arms alternate A, B, A, B ... after a warm-up of both; a round is `steps` whole
pipeline steps between two events on the launch stream.  The per-kernel figures come from a SEPARATE pair of rounds under kpb_prof_enable (its events serialise
the launches: those rounds are not step times).  Decision rule of the record: an arm wins if it is faster in EVERY round and the mean difference is at least three
times the largest spread between rounds of the same arm."""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHAIN = ["conv3x3_b3c1", "conv3x3_b3c2", "maxpool4_x3", "conv1x1_agg3", "conv3x3_b4c1", "conv3x3_b4c2", "conv1x1_agg4"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sparse", action="store_true", help="keypoint-only descriptors (the step every task runs)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=256)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from keypoint_bench_amd import synthetic
    from keypoint_bench_amd._lib import Context
    from keypoint_bench_amd.models.ALike import alike_t
    from keypoint_bench_amd.pipeline import PairPipeline
    dev = torch.device("cuda:0")
    B, H, W = args.pairs, bench.H, bench.W
    with ThreadPoolExecutor(bench.generator_threads(1)) as ex:
        v0s, v1s = zip(*ex.map(lambda i: synthetic.image_pair(i, H, W), range(B)))
    images = torch.from_numpy(np.stack(list(v0s) + list(v1s))).to(dev).contiguous()
    pipe = PairPipeline(alike_t(dense_descriptors=not args.sparse).eval(), bench.EXTRACTOR, bench.BRUTE_FORCE, B, H, W, device=dev)
    ctx = Context.get(dev)
    stream = torch.cuda.current_stream(dev)

    def round_ms(option, steps):
        ctx.set_option(Context.OPT_ALIKE_COARSE_FUSED, option)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            pipe.run(images)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    for option in (0, 1, 0, 1):         # warm-up of both arms (the first run also places the descriptor map: PairPipeline._place_map)
        round_ms(option, 5)
    outs = {}
    for option in (0, 1):               # same results, once, at workload size (the 40 GB descriptor map by the wrapping sum of its bit patterns and a strided sample)
        round_ms(option, 1)
        outs[option] = [t.clone() for t in (pipe.score, pipe.n, pipe.kps, pipe.k, pipe.pairs, pipe.sdesc)]
        if pipe.desc is not None:
            outs[option] += [pipe.desc.view(torch.int32).sum(dtype=torch.int64), pipe.desc.view(-1)[::997].clone()]
    same = all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    del outs
    print("# KPB_OPT_ALIKE_COARSE_FUSED A/B: %s, %d pairs per step, %d rounds of %d steps per arm, interleaved; ms per step" %
          ("keypoint-only" if args.sparse else "dense", B, args.rounds, args.steps))
    print("outputs of arm A and arm B identical (score map, keypoints, descriptors at keypoints, matches%s): %s" % ("" if args.sparse else ", descriptor map", same))
    t = {0: [], 1: []}
    for r in range(args.rounds):
        for option in (0, 1):
            t[option].append(round_ms(option, args.steps))
        print("round %d   A (0, seven launches) %.4f   B (1, four launches) %.4f   A - B %+.4f" % (r, t[0][-1], t[1][-1], t[0][-1] - t[1][-1]))
    mean = {o: sum(v) / len(v) for o, v in t.items()}
    spread = max(max(v) - min(v) for v in t.values())
    diff = mean[0] - mean[1]
    every = all(b < a for a, b in zip(t[0], t[1]))
    print("mean      A %.4f   B %.4f   A - B %+.4f (%.2f %%)   largest same-arm spread %.4f   B faster in every round: %s   |A - B| >= 3 x spread: %s" %
          (mean[0], mean[1], diff, 100.0 * diff / mean[0], spread, every, abs(diff) >= 3.0 * spread))
    print("decision: B (fused) %s" % ("kept" if every and diff >= 3.0 * spread else "NOT shown faster by the rule"))
    prof = {}
    for option in (0, 1):
        round_ms(option, 2)
        ctx.prof_enable(True)
        round_ms(option, 10)
        prof[option] = ctx.prof_report()
        ctx.prof_enable(False)
    print("# per-kernel ms per step (kpb_prof_enable, 10 steps per arm; launches serialised by their events)")
    print("%-20s %10s %10s" % ("kernel", "A", "B"))
    for k in CHAIN + sorted(k for k in set(prof[0]) | set(prof[1]) if k not in CHAIN):
        a, b = prof[0].get(k), prof[1].get(k)
        print("%-20s %10s %10s" % (k, "%.4f" % (a[1] / 10) if a else "-", "%.4f" % (b[1] / 10) if b else "-"))
    print("%-20s %10.4f %10.4f" % ("blocks 3/4 chain", sum(prof[0].get(k, (0, 0.0))[1] for k in CHAIN) / 10, sum(prof[1].get(k, (0, 0.0))[1] for k in CHAIN) / 10))
    ctx.set_option(Context.OPT_ALIKE_COARSE_FUSED, 1)


if __name__ == "__main__":
    main()
