"""kpb_match_ratio (csrc/match.hip): skimage's max_ratio filter on the exact float64 second nearest, from both matcher paths -- match_tile<true>
handing over two entries per column tile, and the prefilter listing every row candidate within the margin of the row's SECOND smallest approximate
distance (match_approx<.., 0, true>), match_exact filing them in row slots row_depth = max(2 tiles_j, 8) deep -- and match_finalize<true> on top.

Every comparison is BIT FOR BIT with `expect` of tests/test_match_ratio_cpu.py (numpy over scipy's cdist; pinned there on oracle.match without
a GPU): index pairs, float64 distance bits, out_k_dev and the pinned host counts of kpb_match_counts; rows beyond a count keep their sentinel.
A call of 8 pairs or more takes the prefilter by default; test_the_other_two_paths_give_the_same_bits runs this file again in fresh child
processes under KPB_MATCH_PREFILTER=0 (match_tile on everything) and =2: all three are held to the same expectation, hence to the same bits."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_cases as mc
from test_match_ratio_cpu import expect

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFILTER = os.environ.get("KPB_MATCH_PREFILTER", "1").strip()
C0 = 64
BELOW_ONE = float(np.nextafter(1.0, 0.0))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ctx():
    from keypoint_bench_amd._lib import Context
    return Context.get(torch.device(DEV))


_CASES, _WANT = {}, {}


def _case(make, *args):
    """A case (match_cases' dict), built once, with its device copies."""
    key = (make.__name__,) + args
    if key not in _CASES:
        c = make(*args)
        c["key"], c["src"] = key, list(range(c["B"]))
        c["dev"] = [_t(c[v]) for v in ("a", "b", "n", "m")]
        _CASES[key] = c
    return _CASES[key]


def _reordered(case, order):
    c = mc.reorder(case, order)
    c["dev"] = [_t(c[v]) for v in ("a", "b", "n", "m")]
    c["src"] = [case["src"][i] for i in order]
    return c


def _want(case, p, maxd, cc, ratio):
    """The expectation of one pair, computed once per pair and parameter set."""
    key = (case["key"], case["src"][p], maxd, cc, ratio)
    if key not in _WANT:
        _WANT[key] = expect(*mc.pair_inputs(case, p), maxd, cc, ratio)
    return _WANT[key]


def _run(ctx, c, maxd, cc, ratio):
    """One call: kpb_match_ratio, or kpb_match itself for ratio = None.  Raw outputs over sentinels, device counts, host counts."""
    from keypoint_bench_amd._lib import MatchParams, ptr
    B, max_n = c["B"], c["max_n"]
    a, b, n, m = c["dev"]
    pairs = torch.full((B, max_n, 2), -1, dtype=torch.int32, device=DEV)
    dist = torch.full((B, max_n), -1.0, dtype=torch.float64, device=DEV)
    k = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    prm = MatchParams(float(maxd), 1 if cc else 0)
    head = (ctx.handle, ptr(a), ptr(b), B, c["C"], max_n, c["max_m"], ptr(n), ptr(m), ctypes.byref(prm))
    if ratio is None:
        ctx.check(ctx.lib.kpb_match(*head, ptr(pairs), ptr(dist), ptr(k)))
    else:
        ctx.check(ctx.lib.kpb_match_ratio(*head, float(ratio), ptr(pairs), ptr(dist), ptr(k)))
    host = (ctypes.c_int32 * B)()
    ctx.check(ctx.lib.kpb_match_counts(ctx.handle, host, B))
    return pairs.cpu().numpy(), dist.cpu().numpy(), k.cpu().tolist(), list(host)


def _check(ctx, c, maxd, cc, ratio, what):
    """One kpb_match_ratio call on the case, every pair against the expectation.  Returns (kept per pair, unfiltered per pair)."""
    pairs, dist, k, host = _run(ctx, c, maxd, cc, ratio)
    want = [_want(c, p, maxd, cc, ratio) for p in range(c["B"])]
    assert host == k == [len(w[0]) for w in want], (what, host, k, [len(w[0]) for w in want])
    for p, (wp, wd, _) in enumerate(want):
        tag = "%s: pair %d (%d of its case), n %d m %d, max_distance %g, cross_check %d, max_ratio %r" % (
            what, p, c["src"][p], c["n"][p], c["m"][p], maxd, cc, ratio)
        K = len(wp)
        np.testing.assert_array_equal(pairs[p, :K], wp, err_msg=tag)
        np.testing.assert_array_equal(dist[p, :K].view(np.uint64), wd.view(np.uint64), err_msg=tag)
        assert (pairs[p, K:] == -1).all() and (dist[p, K:] == -1.0).all(), tag + ": rows beyond the count were written"
    return k, [len(w[2]) for w in want]


# ------------------------------------------------------------------------------------------------ 1. tile edges
@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_tile_edges_with_the_ratio_on(C, cc):
    """match_cases.tile_edge_case(C): 8 pairs with counts at a wave's and a workgroup's rows, the slot tile (128) and the 16-column block (144),
    plus or minus one, at 0 and 1; noisy copies, one pair of integers, decoys beyond the counts.  max_ratio 0.8, max_distance inf and 0.5 sqrt(C)."""
    ctx, c = _ctx(), _case(mc.tile_edge_case, C)
    assert c["B"] == 8 and c["max_m"] == 145
    kept, unfiltered = _check(ctx, c, np.inf, cc, 0.8, "C = %d" % C)
    assert 0 < sum(kept) < sum(unfiltered), (kept, unfiltered)
    kept_d, unfiltered_d = _check(ctx, c, 0.5 * math.sqrt(C), cc, 0.8, "C = %d, finite" % C)
    assert 0 < sum(kept_d) <= sum(unfiltered_d) <= sum(unfiltered), (kept_d, unfiltered_d)
    assert kept[0] == 0 and kept[1] == 0        # n = 0, m = 0


# ------------------------------------------------------------------------------------------------ 2. where the second nearest lies
PLACED_ROWS = 8


def _placed(rng, n, m, C, place):
    """Normal descriptors; for the rows i that place(i) answers with (j1, j2): column j1 is a copy of a[i] at 0.05 sigma-noise, column j2 one
    at 0.05 .. 0.09 (graded by i), so best / second runs from ~1 down to ~0.55 across the rows: 0.8 keeps some and drops some."""
    a = rng.normal(size=(n, C)).astype(np.float32)
    b = rng.normal(size=(m, C)).astype(np.float32)
    for i in range(min(n, PLACED_ROWS)):
        jj = place(i)
        if jj is None:
            continue
        j1, j2 = jj
        assert 0 <= j1 < m and 0 <= j2 < m and j1 != j2
        b[j1] = a[i] + np.float32(0.05) * rng.normal(size=C).astype(np.float32)
        b[j2] = a[i] + np.float32(0.05 + 0.005 * i) * rng.normal(size=C).astype(np.float32)
    return a, b


def second_place_case(C=C0):
    """8 pairs, max_n = 80 (two 64-row tiles), max_m = 145 (two 128-column slot tiles, ten 16-column blocks):
      0  n 80 m 145  second in the nearest's own 16-column block            4  n 33 m 127  the same with m one short of the slot tile
      1  n 65 m 128  second in another block of the same slot tile          5  n 80 m 1    one column: second = inf, ratio 0, every row kept
      2  n 80 m 145  second in the other slot tile, either way round        6  n 17 m 2    two columns
      3  n 64 m 129  second is the LAST valid column (128), alone in its     7  n 1  m 145  one row
                     tile; columns 129.. are decoys: exact copies of a[0..]"""
    rng = np.random.default_rng(8100 + C)
    pairs = [
        _placed(rng, 80, 145, C, lambda i: (16 * i + 2, 16 * i + 9)),
        _placed(rng, 65, 128, C, lambda i: (16 * i + 2, 16 * ((i + 3) % 8) + 9)),
        _placed(rng, 80, 145, C, lambda i: (5 + 9 * i, 128 + 2 * i) if i % 2 == 0 else (128 + 2 * i, 5 + 9 * i)),
        _placed(rng, 64, 129, C, lambda i: (7 + 11 * i, 128) if i == 0 else (7 + 11 * i, 60 + i)),
        _placed(rng, 33, 127, C, lambda i: (7 + 11 * i, 126) if i == 0 else (7 + 11 * i, 60 + i)),
        _placed(rng, 80, 1, C, lambda i: None),
        _placed(rng, 17, 2, C, lambda i: (0, 1) if i == 0 else None),
        _placed(rng, 1, 145, C, lambda i: (140, 3)),
    ]
    return mc._pack(pairs, C, 80, 145)


@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
def test_the_second_nearest_wherever_it_lies(cc):
    ctx, c = _ctx(), _case(second_place_case)
    assert (c["B"], c["max_n"], c["max_m"]) == (8, 80, 145) and c["m"].tolist() == [145, 128, 145, 129, 127, 1, 2, 145]
    assert np.array_equal(c["b"][3, 129], c["a"][3, 0])                 # the decoy behind the last valid column is row 0 itself
    kept, unfiltered = _check(ctx, c, np.inf, cc, 0.8, "second place")
    assert 0 < sum(kept) < sum(unfiltered), (kept, unfiltered)
    assert kept[5] == unfiltered[5] == (1 if cc else 80)                # m = 1: ratio 0, kept
    # the placed rows straddle the threshold: some of them stay, some go (so a wrong second nearest changes the answer)
    for p in (0, 1, 2, 3, 4):
        r = _want(c, p, np.inf, False, 0.8)[2][:PLACED_ROWS]
        assert (r < 0.8).any() and (r >= 0.8).any() and (r < 1.0).all(), (p, r)
    _check(ctx, c, 0.5 * math.sqrt(C0), cc, 0.8, "second place, finite")


# ------------------------------------------------------------------------------------------------ 3. ties and zeros
TWIN_ROWS = 10


def _twins(rng, n, m, C, sigma):
    """Rows i < 10: columns 3 i + 1 and 140 - 5 i (another block, mostly the other side of column 128) are ONE vector, a[i] + sigma noise (sigma 0: a[i]
    itself, distance 0 twice -> 0 / eps = 0, kept; sigma > 0: ratio exactly 1, dropped)."""
    a = rng.normal(size=(n, C)).astype(np.float32)
    b = rng.normal(size=(m, C)).astype(np.float32)
    for i in range(TWIN_ROWS):
        v = a[i] + np.float32(sigma) * rng.normal(size=C).astype(np.float32)
        b[3 * i + 1] = v
        b[140 - 5 * i] = v
    return a, b


def _integers(rng, n, m, C):
    """Components in {-1, 0, 1}: squared distances are small integers, dozens of exact ties for every place."""
    return (np.round(0.7 * rng.normal(size=(n, C))).astype(np.float32), np.round(0.7 * rng.normal(size=(m, C))).astype(np.float32))


def ties_case(C=C0):
    rng = np.random.default_rng(8200 + C)
    pairs = [_twins(rng, 80, 145, C, 0.0), _twins(rng, 70, 145, C, 0.0), _twins(rng, 80, 145, C, 0.05), _twins(rng, 66, 144, C, 0.05),
             _integers(rng, 80, 145, C), _integers(rng, 65, 129, C), _integers(rng, 80, 128, C), _twins(rng, 80, 145, C, 0.05)]
    return mc._pack(pairs, C, 80, 145)


@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
def test_ties_and_zeros(cc):
    ctx, c = _ctx(), _case(ties_case)
    kept, unfiltered = _check(ctx, c, np.inf, cc, 0.8, "ties")
    assert 0 < sum(kept) < sum(unfiltered), (kept, unfiltered)
    rows = lambda p, ratio: set(_want(c, p, np.inf, cc, ratio)[0][:, 0].tolist())
    for p in (0, 1):            # identical columns at distance 0: kept through eps, for any positive max_ratio
        assert set(range(TWIN_ROWS)) <= rows(p, 0.8) and (_want(c, p, np.inf, cc, 0.8)[2][:TWIN_ROWS] == 0.0).all()
    for p in (2, 3, 7):         # identical columns at a positive distance: ratio exactly 1
        assert not set(range(TWIN_ROWS)) & rows(p, 0.8) and (_want(c, p, np.inf, cc, 0.8)[2][:TWIN_ROWS] == 1.0).all()
    for p in (4, 5, 6):         # integers: most rows tie for the second place (and many for the first: ratio exactly 1)
        r = _want(c, p, np.inf, False, 0.8)[2]
        assert (r == 1.0).sum() > 5 and ((r < 1.0) & (r > 0.8)).sum() > 5, r
    kept1, _ = _check(ctx, c, np.inf, cc, BELOW_ONE, "ties, max_ratio one ulp below 1")       # every ratio but exactly 1 passes
    assert sum(kept) < sum(kept1) < sum(unfiltered) and all(kept1[p] <= unfiltered[p] - (0 if cc else TWIN_ROWS) for p in (2, 3, 7))
    tiny, _ = _check(ctx, c, np.inf, cc, 1e-300, "ties, max_ratio 1e-300")                     # only 0 / eps passes
    assert tiny[0] >= TWIN_ROWS and tiny[1] >= TWIN_ROWS and sum(tiny[2:]) == 0, tiny


# ------------------------------------------------------------------------------------------------ 4. near-ties for the second place
NEAR2_ROWS = 30


def _near_second(rng, n, m, C):
    """Rows i < 30: column 4 i is a copy of a[i] at 0.03 noise (the nearest); columns 4 i + 1 .. 4 i + 3 are ONE copy at 0.05 noise and that copy
    with one component moved by one fp32 ulp, up in one and down in the other.  Their squared distances differ by ~1e-8 relative: the fp32
    approximate distances (and the 22-bit split operands) cannot order them, float64 can -- and which of the three is the second nearest
    decides the ratio's last bits."""
    a = rng.normal(size=(n, C)).astype(np.float32)
    b = rng.normal(size=(m, C)).astype(np.float32)
    for i in range(NEAR2_ROWS):
        b[4 * i] = a[i] + np.float32(0.03) * rng.normal(size=C).astype(np.float32)
        c = (a[i] + 0.05 * rng.normal(size=C)).astype(np.float32)
        up, down = c.copy(), c.copy()
        up[i % C] = np.nextafter(c[i % C], np.float32(np.inf))
        down[(i + 7) % C] = np.nextafter(c[(i + 7) % C], np.float32(-np.inf))
        b[4 * i + 1], b[4 * i + 2], b[4 * i + 3] = c, up, down
    return a, b


def near_second_case(C=C0):
    return mc._pack([_near_second(np.random.default_rng(8300 + C + p), 80, 145, C) for p in range(8)], C, 80, 145)


def test_near_ties_for_the_second_place_are_decided_in_float64():
    """For three rows of pair 0: with max_ratio = the row's own float64 ratio the row is dropped (strict), one ulp above it is kept -- a second
    nearest taken from the wrong one of the three columns (a larger second, a smaller ratio) keeps it both times."""
    from scipy.spatial.distance import cdist
    ctx, c = _ctx(), _case(near_second_case)
    a, b = mc.pair_inputs(c, 0)
    D = cdist(a.astype(np.float64), b.astype(np.float64))
    which = np.array([int(np.argmin(D[i, 4 * i + 1: 4 * i + 4])) for i in range(NEAR2_ROWS)])
    assert len(set(which.tolist())) == 3, which          # each of the three columns is the exact second nearest of some row
    ratios = _want(c, 0, np.inf, False, 0.8)[2]
    rows = [int(np.flatnonzero(which == w)[0]) for w in (0, 1, 2)]
    for i in rows:
        three = np.sort(D[i, 4 * i + 1: 4 * i + 4])
        assert three[0] < three[1] and D[i, 4 * i] / three[1] < ratios[i] == D[i, 4 * i] / three[0]
        for cc in (True, False):
            r = float(ratios[i])
            _check(ctx, c, np.inf, cc, r, "near second, row %d at its ratio" % i)
            _check(ctx, c, np.inf, cc, float(np.nextafter(r, 1.0)), "near second, row %d one ulp above" % i)
        assert i not in _want(c, 0, np.inf, False, r)[0][:, 0] and i in _want(c, 0, np.inf, False, float(np.nextafter(r, 1.0)))[0][:, 0]


@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
def test_near_ties_for_the_first_place_with_the_ratio_on(cc):
    """8 copies of match_cases' near-tie pair (two columns one fp32 ulp apart are a row's nearest and second nearest; in about half of the rows
    the float64 nearest is the HIGHER index, which an approximate arg-minimum gets wrong): with max_ratio one ulp below 1 the rows stay, with
    the exact nearest's distance bits; with 0.8 they go."""
    ctx, c = _ctx(), _case(mc.fallback_case, C0)
    c8 = _reordered(c, [mc.FB_NEAR] * 8)
    kept, unfiltered = _check(ctx, c8, np.inf, cc, BELOW_ONE, "8 x near ties, below one")
    wp = _want(c8, 0, np.inf, False, BELOW_ONE)[0]
    first = wp[np.isin(wp[:, 0], np.arange(mc.NEAR_ROWS))]
    odd = int((first[:, 1] % 2 == 1).sum())
    assert len(first) == mc.NEAR_ROWS and 0.3 * mc.NEAR_ROWS <= odd <= 0.7 * mc.NEAR_ROWS, (len(first), odd)
    kept8, _ = _check(ctx, c8, np.inf, cc, 0.8, "8 x near ties, 0.8")
    assert sum(kept8) < sum(kept) <= sum(unfiltered) and sum(kept) >= 8 * mc.NEAR_ROWS, (kept8, kept, unfiltered)
    assert not set(range(mc.NEAR_ROWS)) & set(_want(c8, 0, np.inf, cc, 0.8)[0][:, 0].tolist())


# ------------------------------------------------------------------------------------------------ 5. the threshold's edge, and the ratio off
def _launches(ctx, fn):
    ctx.prof_enable(True)
    try:
        ctx.prof_report()
        out = fn()
        ctx.sync()
        rep = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
    return out, {name: v[0] for name, v in rep.items()}


@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
def test_the_threshold_is_strict_and_the_ratio_off_is_kpb_match(cc):
    ctx, c = _ctx(), _case(mc.tile_edge_case, C0)
    p = 7
    wp, _, ratios = _want(c, p, np.inf, cc, 1.0)
    at = int(np.argmin(np.abs(ratios - 0.5)))                    # a match in the middle of the range
    r, row = float(ratios[at]), int(wp[at, 0])
    assert 0.0 < r < 1.0 and 0.0 < float(np.nextafter(r, 1.0)) < 1.0
    _check(ctx, c, np.inf, cc, r, "at the ratio")
    assert row not in _want(c, p, np.inf, cc, r)[0][:, 0]
    up = float(np.nextafter(r, 1.0))
    _check(ctx, c, np.inf, cc, up, "one ulp above the ratio")
    assert row in _want(c, p, np.inf, cc, up)[0][:, 0]
    plain, launched = _launches(ctx, lambda: _run(ctx, c, np.inf, cc, None))
    for off in (1.0, np.inf):
        got, same = _launches(ctx, lambda: _run(ctx, c, np.inf, cc, off))
        assert same == launched, (off, same, launched)
        assert all(np.array_equal(x, y) for x, y in zip(got[:2], plain[:2])) and got[2:] == plain[2:]
        _check(ctx, c, np.inf, cc, off, "ratio off (%r)" % off)
    assert launched["match_tile"] == 1 and launched["match_finalize"] == 1 and ("match_approx_min" in launched) == (PREFILTER != "0")
    _, on = _launches(ctx, lambda: _run(ctx, c, np.inf, cc, 0.8))
    assert on.get("match_finalize_ratio") == 1 and on.get("match_tile2") == 1 and "match_finalize" not in on and "match_tile" not in on, on
    assert ("match_approx_min2" in on) == (PREFILTER != "0") and "match_approx_min" not in on, on


def test_nan_is_refused_on_a_live_context_and_the_counts_go_with_it():
    from keypoint_bench_amd._lib import KpbError
    ctx, c = _ctx(), _case(mc.tile_edge_case, C0)
    _run(ctx, c, np.inf, True, 0.8)
    with pytest.raises(KpbError) as e:
        _run(ctx, c, np.inf, True, float("nan"))
    assert e.value.code == -1 and "max_ratio is NaN" in str(e.value)
    host = (ctypes.c_int32 * c["B"])()
    assert ctx.lib.kpb_match_counts(ctx.handle, host, c["B"]) == -1      # no completed match: the refused call's counts are nobody's
    _check(ctx, c, np.inf, True, 0.8, "after the refusal")


# ------------------------------------------------------------------------------------------------ 6. fallbacks
MANY = 20


def _many_seconds(rng, C):
    """150 x 300 noisy copies in which row 7 has its copy at column 3 and TWENTY identical columns at 0.08 noise behind it: 21 row candidates
    against row_depth = max(2 x 3, 8) = 8 slots -- the slot overflow flag sends the pair to match_tile<true>."""
    a, b = mc.noisy_pair(rng, mc.FB_N, mc.FB_M, C)
    near = np.flatnonzero(((b - a[7]) ** 2).sum(1) < 0.1 * C)
    b[near] = rng.normal(size=(len(near), C)).astype(np.float32)
    b[3] = a[7] + np.float32(0.05) * rng.normal(size=C).astype(np.float32)
    b[20: 20 + 14 * MANY: 14] = a[7] + np.float32(0.08) * rng.normal(size=C).astype(np.float32)
    return a, b


def many_seconds_case(C=C0):
    """Pair 0: the overflowing pair; pairs 1..7: the control pair of fallback_case(C) (seed 5000 + C)."""
    clean = mc.fb_control(np.random.default_rng(5000 + C), C)
    return mc._pack([_many_seconds(np.random.default_rng(8400 + C), C)] + [clean] * 7, C, mc.FB_N, mc.FB_M)


@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
@pytest.mark.parametrize("C", [64, 160])
def test_fallbacks_with_the_ratio_on_alone_and_mixed_then_a_clean_call(C, cc):
    """match_cases.fallback_case(C) -- list overflow, row / column slot overflow, NaN row, 2^15, empty, beside clean pairs -- in one call, in
    reverse order, the dirty pairs ALONE (8 copies each), then the pair with 20 identical second-best columns alone, first and last among clean
    pairs, then 8 clean pairs on the workspace all that left behind."""
    ctx, c = _ctx(), _case(mc.fallback_case, C)
    k, u = _check(ctx, c, np.inf, cc, 0.8, "C = %d, in order" % C)
    assert 0 < sum(k) < sum(u) and 0 < k[mc.FB_CONTROL] and k[11] == 0, (k, u)
    kr, _ = _check(ctx, _reordered(c, list(range(12, -1, -1))), np.inf, cc, 0.8, "C = %d, reversed" % C)
    assert kr == k[::-1]
    for p in (1, 4, 5, 7, 8, 9, 11):
        kp, _ = _check(ctx, _reordered(c, [p] * 8), 0.5 * math.sqrt(C), cc, 0.8, "C = %d, pair %d alone" % (C, p))
        assert len(set(kp)) == 1
    m = _case(many_seconds_case, C)
    r7 = _want(m, 0, np.inf, False, 0.8)[2][7]
    assert 0.4 < r7 < 0.8 and r7 == _want(m, 0, np.inf, False, 1.0)[2][7], r7
    for order, what in (([0] * 8, "alone"), (list(range(8)), "first"), (list(range(7, -1, -1)), "last")):
        km, um = _check(ctx, _reordered(m, order), np.inf, cc, 0.8, "C = %d, many seconds %s" % (C, what))
        assert 0 < sum(km) < sum(um)
        at = order.index(0)
        assert 7 in _want(m, 0, np.inf, cc, 0.8)[0][:, 0] and km[at] == len(_want(m, 0, np.inf, cc, 0.8)[0])
    kc, _ = _check(ctx, _case(mc.control_case, C), np.inf, cc, 0.8, "C = %d, 8 x control after the dirty calls" % C)
    assert kc == [k[mc.FB_CONTROL]] * 8
    kc0, _ = _check(ctx, _case(mc.control_case, C), np.inf, cc, 1.0, "C = %d, 8 x control, ratio off, after the ratio calls" % C)
    assert kc0[0] > kc[0]


# ------------------------------------------------------------------------------------------------ 7. paths
def test_calling_twice_gives_the_same_bits():
    ctx = _ctx()
    for c in (_case(mc.tile_edge_case, C0), _case(ties_case), _case(many_seconds_case, C0)):
        first = _run(ctx, c, np.inf, True, 0.8)
        again = _run(ctx, c, np.inf, True, 0.8)
        for p in range(c["B"]):
            K = first[2][p]
            assert np.array_equal(first[0][p, :K], again[0][p, :K]) and np.array_equal(first[1][p, :K].view(np.uint64), again[1][p, :K].view(np.uint64))
        assert first[2:] == again[2:]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode", ["0", "2"])
def test_the_other_two_paths_give_the_same_bits(mode):
    """This file again in a fresh child process (subprocess.run: a child, never an exec of this GPU-initialised process) under KPB_MATCH_PREFILTER=0
    -- match_tile<true> on every pair -- and =2: every mode is held to the same expectation bit for bit, so all three give identical bits."""
    env = dict(os.environ, KPB_MATCH_PREFILTER=mode)
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not other_two_paths and not python_layers",
           "tests/test_gpu_match_ratio.py"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=550)
    tail = "\n".join(p.stdout.splitlines()[-25:])
    assert p.returncode == 0, "child pytest with KPB_MATCH_PREFILTER=%s failed:\n%s" % (mode, tail)
    assert " passed" in tail and "skipped" not in tail.split("passed")[-1], tail


# ------------------------------------------------------------------------------------------------ 8. the Python layers
EP = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
BF = dict(metric="euclidean", max_distance=5, cross_check=True)


def test_python_layers_read_max_ratio():
    """ALIKE at 96 x 128: match_descriptors(max_ratio = 0.8) is the expectation; brute_force_matcher and PairPipeline with the key return those
    rows; the runner's match_stats rows are the same for batch 1 and batch 4, with counts strictly below those without the key."""
    from keypoint_bench_amd import runner, synthetic
    from keypoint_bench_amd.models.ALike import alike_t
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import brute_force_matcher, match_descriptors, sample_descriptors
    B, H, W = 2, 96, 128
    v = [synthetic.image_pair(100 + i, H, W) for i in range(B)]
    i0, i1 = np.stack([a for a, _ in v]), np.stack([b for _, b in v])
    on = dict(BF, max_ratio=0.8)
    net = alike_t(dense_descriptors=True).eval()
    pipe = PairPipeline(net, EP, on, B, H, W, device=DEV)
    pipe.run(torch.from_numpy(np.concatenate([i0, i1])).to(DEV))
    single = alike_t(dense_descriptors=True).eval()
    for b in range(B):
        s0, d0 = single(torch.from_numpy(i0[b])[None].to(DEV))
        k0 = detection(s0, EP)
        f0 = sample_descriptors(k0, d0)
        s1, d1 = single(torch.from_numpy(i1[b])[None].to(DEV))
        k1 = detection(s1, EP)
        f1 = sample_descriptors(k1, d1)
        wp, wd, _ = expect(f0.cpu().numpy(), f1.cpu().numpy(), 5, True, 0.8)
        wall = expect(f0.cpu().numpy(), f1.cpu().numpy(), 5, True, 1.0)[0]
        assert 0 < len(wp) < len(wall), (len(wp), len(wall))
        pairs, dist = match_descriptors(f0, f1, max_distance=5, cross_check=True, return_distance=True, max_ratio=0.8)
        np.testing.assert_array_equal(pairs.cpu().numpy(), wp)
        np.testing.assert_array_equal(dist.cpu().numpy().view(np.uint64), wd.view(np.uint64))
        np.testing.assert_array_equal(match_descriptors(f0, f1, max_distance=5, cross_check=True).cpu().numpy(), wall)      # the default is off
        m0, m1 = brute_force_matcher(k0, k1, d0, d1, on)
        np.testing.assert_array_equal(m0.cpu().numpy(), k0.cpu().numpy()[wp[:, 0]])
        np.testing.assert_array_equal(m1.cpu().numpy(), k1.cpu().numpy()[wp[:, 1]])
        got = pipe.pair(b)
        np.testing.assert_array_equal(got["pairs"], wp)
        np.testing.assert_array_equal(got["dist"].view(np.uint64), wd.view(np.uint64))
        np.testing.assert_array_equal(got["m0"], m0.cpu().numpy())
        np.testing.assert_array_equal(got["m1"], m1.cpu().numpy())

    def params(bf):
        return {"model_type": "Alike", "task_type": "match_stats", "Alike_params": dict(c1=8, c2=16, c3=32, c4=64, dim=64), "extractor_params": EP,
                "matcher_params": {"type": "brute_force", "brute_force_params": bf}}

    ds = [{"image0": synthetic.image_pair(100 + i, H, W)[0], "image1": synthetic.image_pair(100 + i, H, W)[1], "dataset": "HPatches"} for i in range(6)]
    rows = {}
    for name, bf, batch in (("on1", on, 1), ("on4", on, 4), ("off4", BF, 4)):
        r = runner.PairRunner(params(bf), device=DEV, batch=batch)
        rows[name] = r.run(ds)[1]
        assert r.batched_pairs == (0 if batch == 1 else 6)
    assert np.array_equal(rows["on1"].view(np.uint64), rows["on4"].view(np.uint64)), (rows["on1"], rows["on4"])
    assert (rows["on4"][:, :2] == rows["off4"][:, :2]).all() and (0 < rows["on4"][:, 2]).all() and (rows["on4"][:, 2] < rows["off4"][:, 2]).all(), rows
