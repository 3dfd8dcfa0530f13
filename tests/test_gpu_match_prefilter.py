"""The match prefilter of csrc/match.hip (match_prep, match_approx<KB, RT, 0 / 1>, match_exact) where the goldens and the fuzz do not reach:
all eight channel forms at the edges of their wave, workgroup and slot tiles; the three ways a pair falls back to match_tile (candidate
list overflow, slot overflow, non-finite / 2^15), alone and mixed with pairs that do not, in both orders and followed by a clean call on
the dirty workspace; near-ties below the filter's resolution; a wave buffer that flushes inside the column loop.  And kpb_sample
(sample_bilinear) on the border, outside the map, on one-row / one-column maps, in the tail of its four-keypoint group and with ragged counts.

Every comparison is BIT FOR BIT with the CPU oracle (oracle.match, oracle.sample, oracle.sample_hwc) on the inputs of tests/match_cases.py,
which tests/test_oracle_match_edge.py and tests/test_oracle_sample_edge.py pin on scipy / grid_sample without a GPU: index pairs, float64
distance bits, the counts of kpb_match_counts and out_k_dev.  Whether a pair raised the fallback flag is not observable (and no ABI is added
for it): match_cases states per pair, from the code, why it must or must not; both paths have to give the oracle's bits.

tests/test_gpu_variants.py runs this file again under KPB_MATCH_PREFILTER=0 (match_tile itself on every family and at C = 96 .. 224) and =2."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
import match_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PREFILTER_OFF = os.environ.get("KPB_MATCH_PREFILTER", "1").strip() == "0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ctx():
    from keypoint_bench_amd._lib import Context
    return Context.get(torch.device(DEV))


_CASES, _WANT = {}, {}


def _case(make, *args):
    """A case of match_cases, built once, with its device copies."""
    key = (make.__name__,) + args
    if key not in _CASES:
        c = make(*args)
        c["key"] = key
        c["dev"] = [_t(c[v]) for v in ("a", "b", "n", "m")]
        c["src"] = list(range(c["B"]))      # pair p of this case is pair src[p] of the case the oracle ran on
        _CASES[key] = c
    return _CASES[key]


def _reordered(case, order):
    c = mc.reorder(case, order)
    c["dev"] = [_t(c[v]) for v in ("a", "b", "n", "m")]
    c["src"] = [case["src"][i] for i in order]
    return c


def _want(case, p, maxd, cc):
    """The oracle's (pairs, distances) of one pair: computed once per pair and parameter set, shared by every call that holds the pair."""
    key = (case["key"], case["src"][p], maxd, cc)
    if key not in _WANT:
        _WANT[key] = oracle.match(*mc.pair_inputs(case, p), maxd, cc)
    return _WANT[key]


def _match(ctx, c, maxd, cc):
    from keypoint_bench_amd._lib import MatchParams, ptr
    B, max_n = c["B"], c["max_n"]
    a, b, n, m = c["dev"]
    pairs = torch.full((B, max_n, 2), -1, dtype=torch.int32, device=DEV)
    dist = torch.full((B, max_n), -1.0, dtype=torch.float64, device=DEV)
    k = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    prm = MatchParams(float(maxd), 1 if cc else 0)
    ctx.check(ctx.lib.kpb_match(ctx.handle, ptr(a), ptr(b), B, c["C"], max_n, c["max_m"], ptr(n), ptr(m), ctypes.byref(prm), ptr(pairs), ptr(dist), ptr(k)))
    host = (ctypes.c_int32 * B)()
    ctx.check(ctx.lib.kpb_match_counts(ctx.handle, host, B))
    return pairs.cpu().numpy(), dist.cpu().numpy(), k.cpu().tolist(), list(host)


def _check(ctx, c, maxd, cc, what):
    """One kpb_match call on the case; every pair against the oracle.  Returns the number of matches per pair."""
    pairs, dist, k, host = _match(ctx, c, maxd, cc)
    want = [_want(c, p, maxd, cc) for p in range(c["B"])]
    assert host == k == [len(w[0]) for w in want], (what, host, k, [len(w[0]) for w in want])
    for p, (wp, wd) in enumerate(want):
        tag = "%s: pair %d (%d of its case), n %d m %d, max_distance %g, cross_check %d" % (what, p, c["src"][p], c["n"][p], c["m"][p], maxd, cc)
        K = len(wp)
        np.testing.assert_array_equal(pairs[p, :K], wp, err_msg=tag)
        np.testing.assert_array_equal(dist[p, :K].view(np.uint64), wd.view(np.uint64), err_msg=tag)
        assert (pairs[p, K:] == -1).all() and (dist[p, K:] == -1.0).all(), tag + ": rows beyond the count were written"
    return k


# ------------------------------------------------------------------------------------------------ 2. every channel form at its tile edges
CHANNELS = (32, 64, 96, 128, 160, 192, 224, 256)


@pytest.mark.parametrize("finite", [False, True], ids=["inf", "finite"])
@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
@pytest.mark.parametrize("C", CHANNELS)
def test_every_channel_form_at_its_tile_edges(C, cc, finite):
    """match_approx<C / 32, RT>: 8 pairs of up to (64 RT + 17) x 145 with counts at a wave's rows (16 RT) and a workgroup's rows (64 RT)
    plus or minus one, at the slot tile (128) and the 16-column block (144) plus or minus one, and at 0 and 1; noisy copies, one pair of
    integers (exact ties), decoys beyond the counts (match_cases.tile_edge_case).  0.5 sqrt(C) lies between a copy's distance
    (0.05 sqrt(C)) and a chance neighbour's (~sqrt(C))."""
    c = _case(mc.tile_edge_case, C)
    assert c["max_n"] == 64 * mc.RT_OF[C] + 17 and c["max_m"] == 145 and c["B"] == 8
    maxd = 0.5 * float(np.sqrt(C)) if finite else np.inf
    k = _check(_ctx(), c, maxd, cc, "C = %d" % C)
    assert k[0] == 0 and k[1] == 0 and sum(k) > 60, k        # n = 0 and m = 0 give nothing; the others match (RT = 1: ~90 copies in all)


@pytest.mark.parametrize("C", CHANNELS)
def test_the_calls_above_stand_on_the_prefilter(C):
    """The library's own launch record of one such call names match_approx_cand (and its siblings) -- unless KPB_MATCH_PREFILTER=0 is
    set, as tests/test_gpu_variants.py sets it for its child run: then match_tile alone serves the call and no prefilter kernel runs."""
    ctx, c = _ctx(), _case(mc.tile_edge_case, C)
    ctx.prof_enable(True)
    try:
        ctx.prof_report()
        _check(ctx, c, np.inf, True, "C = %d, recorded" % C)
        ctx.sync()
        rep = ctx.prof_report()
    finally:
        ctx.prof_enable(False)
    print("C = %d (KPB_MATCH_PREFILTER %s): %s" % (C, os.environ.get("KPB_MATCH_PREFILTER", "unset"), {k: v[0] for k, v in sorted(rep.items())}))
    assert rep["match_tile"][0] == 1 and rep["match_finalize"][0] == 1, rep
    pre = ("match_prep", "match_approx_min", "match_approx_cand", "match_exact")
    if PREFILTER_OFF:
        assert not [name for name in pre if name in rep], rep
    else:
        assert [rep.get(name, (0, 0))[0] for name in pre] == [1, 1, 1, 1], rep


# ------------------------------------------------------------------------------------------------ 3. the fallbacks, alone and mixed
@pytest.mark.parametrize("finite", [False, True], ids=["inf", "finite"])
@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
@pytest.mark.parametrize("C", [64, 160])
def test_fallbacks_alone_and_mixed_in_both_orders_then_a_clean_call(C, cc, finite):
    """13 pairs of 150 x 300 (3 x 3 slot tiles, cap = 3600) in ONE call: pairs that overflow the candidate list (1, 2, 3, 10), a row's
    slots (4, 7), a column's slots (5), that are non-finite (8) or reach 2^15 (9), beside pairs the filter keeps (0, 6 at exactly 3 of 3
    slots, 12 with near-ties it cannot resolve) and an empty one (11) -- match_cases.FALLBACK_PAIRS says why, pair by pair.  Then the
    same pairs in reverse order: a flag, a candidate count or a slot counter indexed by the wrong pair gives another pair's result.  Then
    8 copies of the control pair on the same context: flags, counts and slot fills of the workspace the two calls left are reset.
    C = 64 is an RT = 4 form, C = 160 an RT = 1 form."""
    ctx, c = _ctx(), _case(mc.fallback_case, C)
    assert (c["B"], c["max_n"], c["max_m"]) == (13, 150, 300)
    maxd = 0.5 * float(np.sqrt(C)) if finite else np.inf
    k = _check(ctx, c, maxd, cc, "C = %d, in order" % C)
    kr = _check(ctx, _reordered(c, list(range(12, -1, -1))), maxd, cc, "C = %d, reversed" % C)
    assert kr == k[::-1] and k[11] == 0 and k[0] > 60
    kc = _check(ctx, _case(mc.control_case, C), maxd, cc, "C = %d, 8 x control after the mixed calls" % C)
    assert kc == [k[0]] * 8


@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
def test_near_ties_keep_the_float64_nearest_of_two_columns_the_filter_cannot_tell_apart(cc):
    """8 copies of the near-tie pair alone (nothing else in the call can trigger anything): in about half of the 60 rows the match is
    the odd column, which precedes only in float64."""
    ctx, c = _ctx(), _case(mc.fallback_case, 64)
    c8 = _reordered(c, [mc.FB_NEAR] * 8)
    _check(ctx, c8, np.inf, cc, "8 x near ties")
    odd = int((_want(c8, 0, np.inf, False)[0][: mc.NEAR_ROWS, 1] % 2 == 1).sum())
    assert 0.3 * mc.NEAR_ROWS <= odd <= 0.7 * mc.NEAR_ROWS, odd


@pytest.mark.parametrize("finite", [False, True], ids=["inf", "finite"])
@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
def test_the_filter_at_the_top_of_its_range(cc, finite):
    """Whole pairs scaled by 2^12 with components at nextafter(32768, 0): match_prep admits them and the margins stay small against the
    distances, so the filter itself decides, one ulp below where its half-precision hi pieces would saturate."""
    c = _case(mc.top_of_range_case, 64)
    k = _check(_ctx(), c, 0.5 * 8.0 * 4096.0 if finite else np.inf, cc, "top of range")
    assert min(k) > 20, k


# ------------------------------------------------------------------------------------------------ 4. the wave buffer flushes mid-loop
@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
def test_a_wave_that_collects_more_candidates_than_its_buffer_flushes(cc):
    """8 pairs of 130 x 520 x 64: rows 0..63, one wave of match_approx<2, 4>, list 4 identical nearest columns each -- 256 entries
    through a buffer of 192 that is flushed above 128 (match_cases.wave_flush_case).  An entry lost or doubled between two flushes
    changes a row's or a column's arg-minimum."""
    c = _case(mc.wave_flush_case, 64)
    assert (c["B"], c["max_n"], c["max_m"]) == (8, 130, 520)
    k = _check(_ctx(), c, np.inf, cc, "wave flush")
    assert min(k) >= (mc.WF_ROWS if cc else mc.WF_N), k


# ------------------------------------------------------------------------------------------------ 5. kpb_sample at its edges
SENTINEL = -7.0


def _sample(d_dev, layout, C, Hd, Wd, pts_dev, max_n, n_dev=None):
    """kpb_sample on d_dev: [B, C, Hd, Wd] ("chw") or [B, Hd, Wd, C] ("hwc"), through its element strides; pts_dev [B, max_n, cols]."""
    from keypoint_bench_amd._lib import ptr
    ctx = _ctx()
    B = d_dev.shape[0]
    sb, sc, sh, sw = (C * Hd * Wd, Hd * Wd, Wd, 1) if layout == "chw" else (C * Hd * Wd, 1, Wd * C, C)
    out = torch.full((B, max_n, C), SENTINEL, device=DEV)
    ctx.check(ctx.lib.kpb_sample(ctx.handle, ptr(d_dev), B, C, Hd, Wd, sb, sc, sh, sw, ptr(pts_dev), pts_dev.shape[-1], max_n, ptr(n_dev), ptr(out)))
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", mc.SAMPLE_MAPS, ids=lambda s: "x".join(map(str, s)))
def test_sample_on_the_border_outside_the_map_and_in_the_group_tail(shape):
    """All 23 edge points at once (five groups of four keypoints and a tail of three), then N = 1, 2, 3, 5 at every offset into the list
    that the point set allows in steps of 3: a keypoint's bits depend neither on its place in the group nor on N.  NCHW against
    oracle.sample, channels-last against oracle.sample_hwc."""
    C, Hd, Wd = shape
    d, p = mc.sample_map(*shape), mc.sample_points()
    hwc = np.ascontiguousarray(d.transpose(1, 2, 0))
    maps = {"chw": (_t(d[None]), oracle.sample(d, p)), "hwc": (_t(hwc[None]), oracle.sample_hwc(hwc, p))}
    assert np.array_equal(maps["chw"][1].view(np.uint32), maps["hwc"][1].view(np.uint32))
    for layout, (dev, want) in maps.items():
        got = _sample(dev, layout, C, Hd, Wd, _t(p[None]), len(p))[0]
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg="%s %s all points" % (shape, layout))
        for N in mc.SAMPLE_COUNTS:
            for o in range(0, len(p) - N + 1, 3):
                got = _sample(dev, layout, C, Hd, Wd, _t(p[None, o:o + N]), N)[0]
                np.testing.assert_array_equal(got.view(np.uint32), want[o:o + N].view(np.uint32), err_msg="%s %s N %d from %d" % (shape, layout, N, o))


@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_sample_batched_with_ragged_counts_and_three_point_columns(layout):
    """One call of B = 3 maps of 65 x 4 x 5 with n_dev = (0, 3, max_n = 6) and pts_cols = 3 (x, y, score): image b's rows are those of
    ITS map at ITS points; rows beyond n[b] of out_dev keep the sentinel; the points beyond n[b] (far off the map) are never used."""
    C, Hd, Wd = 65, 4, 5
    B, max_n = 3, 6
    n = np.array([0, 3, max_n], np.int32)
    p = mc.sample_points()
    d = np.stack([mc.sample_map(C, Hd, Wd, seed=b) for b in range(B)])
    pts = np.full((B, max_n, 3), 77.0, np.float32)
    for b in range(B):
        pts[b, : n[b], :2] = p[3 + 7 * b: 3 + 7 * b + n[b]]
        pts[b, : n[b], 2] = 0.25 + b
    src = d if layout == "chw" else np.ascontiguousarray(d.transpose(0, 2, 3, 1))
    got = _sample(_t(src), layout, C, Hd, Wd, _t(pts), max_n, _t(n))
    for b in range(B):
        want = oracle.sample(d[b], pts[b, : n[b]]) if layout == "chw" else oracle.sample_hwc(src[b], pts[b, : n[b]])
        np.testing.assert_array_equal(got[b, : n[b]].view(np.uint32), want.view(np.uint32), err_msg="image %d" % b)
        assert (got[b, n[b]:] == SENTINEL).all(), "image %d: rows beyond its count were written" % b
    assert np.abs(got[1, :3]).max() > 0 and not np.array_equal(got[1, :3], got[2, :3])
