#!/usr/bin/env python3
"""Are the kernels of two builds the same kernels?  Compares, per kernel symbol, the instruction text and the .amdhsa_ descriptor block (registers, LDS,
scratch) of the assembly build.py leaves in _obj/<unit>.fixed.s:
    python scripts/kernel_diff.py OLD/keypoint_bench_amd/_obj [NEW/keypoint_bench_amd/_obj]      (exit status 1 if a symbol is lost, new or differs)
A kernel that changed its name only: --renamed OLD=NEW (repeatable; a substring of each mangled name that fits one symbol).  The pair is compared with the symbol
name itself substituted out and, if equal, reported as `renamed`; several old kernels may map onto one new one."""
import argparse
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the template kernels of conv_mfma.h: their instantiations are the only symbols more than one translation unit may hold
SHARED_TEMPLATES = re.compile(r"N_1(11conv_mfma_h|9conv_mfma|6gemm_h)I")


def kernels(obj):
    """{symbol: (normalised body + descriptor, {units that hold it})} of every .amdhsa_kernel in obj/*.fixed.s"""
    out = {}
    for path in sorted(glob.glob(os.path.join(obj, "*.fixed.s"))):
        text = open(path).read()
        for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.S | re.M):
            sym = m.group(1)
            body = text[text.index("\n%s:" % sym):m.start()]
            norm = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+", r".\1", body + m.group(2))       # function-numbered local labels
            norm = "\n".join(l.split(";")[0].rstrip() for l in norm.splitlines())               # comments carry unit-local numbering too
            units = out.setdefault(sym, (norm, set()))[1]
            units.add(os.path.basename(path)[:-len(".fixed.s")])
            if out[sym][0] != norm:
                out[sym] = (None, units)        # two units of one build disagree: reported as different
    return out


def anonymous(sym, norm):
    """a kernel's normalised text with its own symbol name substituted out (None stays None: units that disagree)"""
    return None if norm is None else norm.replace(sym, "@")


def one(ks, part, which):
    hits = [s for s in ks if part in s]
    if len(hits) != 1:
        sys.exit("--renamed: %r fits %d symbols of the %s build" % (part, len(hits), which))
    return hits[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new", nargs="?", default=os.path.join(ROOT, "keypoint_bench_amd", "_obj"))
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    lost, added = set(old) - set(new), set(new) - set(old)
    differ = sorted(s for s in set(old) & set(new) if old[s][0] is None or old[s][0] != new[s][0])
    for pair in args.renamed:
        o, n = (one(ks, part, which) for ks, part, which in zip((old, new), pair.split("=", 1), ("old", "new")))
        if anonymous(o, old[o][0]) is not None and anonymous(o, old[o][0]) == anonymous(n, new[n][0]):
            print("%-8s %s -> %s" % ("renamed", o, n))
            lost.discard(o)
            added.discard(n)
    lost, added = sorted(lost), sorted(added)
    for tag, syms in (("lost", lost), ("new", added), ("differs", differ)):
        for s in syms:
            print("%-8s %s" % (tag, s))
    for name, ks in (("old", old), ("new", new)):
        per = {}
        for s, (_, units) in ks.items():
            for u in units:
                per[u] = per.get(u, 0) + 1
        print("%s: %d distinct kernel symbols; per unit: %s" % (name, len(ks), ", ".join("%s %d" % kv for kv in sorted(per.items()))))
    for s in sorted(new):
        if SHARED_TEMPLATES.search(s) and new[s][1] != old.get(s, (0, new[s][1]))[1]:
            print("moved    %s: %s -> %s" % (s[:110], ",".join(sorted(old[s][1])), ",".join(sorted(new[s][1]))))
    sys.exit(1 if lost or added or differ else 0)


if __name__ == "__main__":
    main()
