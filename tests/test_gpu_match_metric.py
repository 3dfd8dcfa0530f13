"""KPB_OPT_MATCH_METRIC (csrc/match.hip): kpb_match_ratio on sqeuclidean, cityblock, chebyshev and cosine distances, from every path --
match_tile<.., METRIC> on everything, euclidean's prefilter shared by sqeuclidean, cosine's own prefilter (match_approx<.., COS> on the split-f16
dot products, match_exact<true>) -- with match_finalize<.., false> ordering and filtering on the metric's value.

Every comparison is BIT FOR BIT with `expect` of tests/match_metric_cases.py (numpy; pinned on the live scipy cdist by
tests/test_match_metric_cpu.py without a GPU): index pairs, float64 distance bits, out_k_dev and the pinned host counts of kpb_match_counts; rows
beyond a count keep their sentinel; no pair of a case is left out.  One thing is compared by kind, not by bits: a NaN distance (a zero row under
cosine survives max_distance = inf) must be a NaN -- the sign of a generated NaN (0 / 0) is the processor's.
A call of 8 pairs or more takes the prefilter by default where the metric has one; tests/test_gpu_match_metric_variants.py runs this file again in
fresh child processes under KPB_MATCH_PREFILTER=0 (match_tile on everything), =2 and KPB_FP32_MATRIX=1: all are held to the same expectation."""
import ctypes
import os

import numpy as np
import pytest
import torch

import match_cases as mc
import match_metric_cases as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PREFILTER = os.environ.get("KPB_MATCH_PREFILTER", "1").strip()
C0 = 64
ID = {k: i for i, k in enumerate(mm.METRICS)}
# about the value of a noisy copy (match_cases.noisy_pair, sigma 0.05) under each metric at C = 64: the filter keeps some and drops some
MAXD = {"euclidean": 0.4, "sqeuclidean": 0.16, "cityblock": 2.55, "chebyshev": 0.125, "cosine": 0.00125}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ctx():
    from keypoint_bench_amd._lib import Context
    return Context.get(torch.device(DEV))


_CASES, _DIST = {}, {}


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


def _want(case, p, metric, maxd, cc, ratio):
    """The expectation of one pair: its distance matrix is computed once per metric and left unchanged."""
    key = (case["key"], case["src"][p], metric)
    if key not in _DIST:
        _DIST[key] = mm.distances(*mc.pair_inputs(case, p), metric)
    return mm.glue(_DIST[key], maxd, cc, ratio)


def _run(ctx, c, metric, maxd, cc, ratio):
    """One call: kpb_match_ratio under KPB_OPT_MATCH_METRIC = metric (a name or an id), set through the library itself and put back to euclidean
    afterwards; metric = None: the option is not touched.  Raw outputs over sentinels, device counts, host counts."""
    from keypoint_bench_amd._lib import Context, MatchParams, ptr
    B, max_n = c["B"], c["max_n"]
    a, b, n, m = c["dev"]
    pairs = torch.full((B, max_n, 2), -1, dtype=torch.int32, device=DEV)
    dist = torch.full((B, max_n), -1.0, dtype=torch.float64, device=DEV)
    k = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    prm = MatchParams(float(maxd), 1 if cc else 0)
    head = (ctx.handle, ptr(a), ptr(b), B, c["C"], max_n, c["max_m"], ptr(n), ptr(m), ctypes.byref(prm))
    try:
        if metric is not None:
            ctx.set_option(Context.OPT_MATCH_METRIC, metric if isinstance(metric, int) else ID[metric])
        ctx.check(ctx.lib.kpb_match_ratio(*head, float(ratio), ptr(pairs), ptr(dist), ptr(k)))
    finally:
        if metric is not None:
            ctx.set_option(Context.OPT_MATCH_METRIC, 0)
    host = (ctypes.c_int32 * B)()
    ctx.check(ctx.lib.kpb_match_counts(ctx.handle, host, B))
    return pairs.cpu().numpy(), dist.cpu().numpy(), k.cpu().tolist(), list(host)


def _same_values(got, want, tag):
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=tag + ": NaN positions")
    np.testing.assert_array_equal(got[~gn].view(np.uint64), want[~wn].view(np.uint64), err_msg=tag)


def _check(ctx, c, metric, maxd=np.inf, cc=True, ratio=1.0, what=""):
    """One kpb_match_ratio call under the metric on the case, every pair against the expectation.  Returns the counts."""
    pairs, dist, k, host = _run(ctx, c, metric, maxd, cc, ratio)
    want = [_want(c, p, metric, maxd, cc, ratio) for p in range(c["B"])]
    assert host == k == [len(w[0]) for w in want], (metric, what, host, k, [len(w[0]) for w in want])
    for p, (wp, wd, _) in enumerate(want):
        tag = "%s %s: pair %d (%d of its case), n %d m %d, max_distance %g, cross_check %d, max_ratio %r" % (
            metric, what, p, c["src"][p], c["n"][p], c["m"][p], maxd, cc, ratio)
        K = len(wp)
        np.testing.assert_array_equal(pairs[p, :K], wp, err_msg=tag)
        _same_values(dist[p, :K], wd, tag)
        assert (pairs[p, K:] == -1).all() and (dist[p, K:] == -1.0).all(), tag + ": rows beyond the count were written"
    return k


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


def _in_chunks(ctx, c, metric, maxd, cc, ratio, what, size=5):
    """The case in calls of fewer than 8 pairs: match_tile alone under the default."""
    k = []
    for at in range(0, c["B"], size):
        k += _check(ctx, _reordered(c, list(range(at, min(at + size, c["B"])))), metric, maxd, cc, ratio, "%s, pairs %d.." % (what, at))
    return k


# ------------------------------------------------------------------------------------------------ 1. every metric through match_tile
@pytest.mark.parametrize("metric", mm.NEW_METRICS)
def test_every_metric_through_match_tile_on_the_tile_edges_and_the_fallback_pairs(metric):
    """tile_edge_case(64) and fallback_case(64) -- counts at 0, 1, the 64-row and 128-column tiles plus or minus one, exact ties, zeros, a NaN row,
    2^15, decoys beyond the counts -- in calls of 5 pairs (match_tile under the default), with and without the cross-check and max_distance."""
    ctx = _ctx()
    for make in (mc.tile_edge_case, mc.fallback_case):
        c = _case(make, C0)
        k = _in_chunks(ctx, c, metric, np.inf, True, 1.0, make.__name__)
        kd = _in_chunks(ctx, c, metric, MAXD[metric], False, 1.0, make.__name__ + ", finite, rows")
        assert 0 < sum(k) and 0 < sum(kd), (k, kd)
    _, on = _launches(ctx, lambda: _run(ctx, _reordered(_case(mc.tile_edge_case, C0), [5, 6, 7]), metric, np.inf, True, 1.0))
    tile = {"sqeuclidean": "match_tile_sq", "cityblock": "match_tile_l1", "chebyshev": "match_tile_linf", "cosine": "match_tile_cos"}[metric]
    assert on.get(tile) == 1 and on.get("match_finalize_value") == 1 and "match_tile" not in on and "match_finalize" not in on, on


@pytest.mark.parametrize("C", [1, 3, 33, 100])
@pytest.mark.parametrize("metric", mm.NEW_METRICS)
def test_every_metric_at_the_widths_off_the_vector_path(metric, C):
    """One pair of 70 x 135 with the special rows (multiples, zero, 1e-30, NaN, inf, ulp neighbours) on both sides: an odd width and the cosine
    tail (1, 3, 33), the scalar staging (C % 4) and a KC = 16 remainder (33 = 2 x 16 + 1, 100 = 6 x 16 + 4)."""
    ctx, c = _ctx(), _case(mm.single_pair_case, C)
    _check(ctx, c, metric, np.inf, True, 1.0, "C = %d" % C)
    _check(ctx, c, metric, np.inf, False, 0.8, "C = %d, rows, ratio" % C)


# ------------------------------------------------------------------------------------------------ 2. cosine through its prefilter
@pytest.mark.parametrize("C", [32, 64, 96, 128, 160, 192, 224, 256])
def test_cosine_prefilter_on_the_tile_edges_of_every_channel_form(C):
    ctx, c = _ctx(), _case(mc.tile_edge_case, C)
    assert c["B"] == 8 and c["max_m"] == 145
    k = _check(ctx, c, "cosine", np.inf, True, 1.0, "C = %d" % C)
    kd = _check(ctx, c, "cosine", MAXD["cosine"], False, 1.0, "C = %d, finite, rows" % C)
    assert 0 < sum(kd) and 0 < sum(k) and k[0] == 0 and k[1] == 0, (k, kd)
    _, on = _launches(ctx, lambda: _run(ctx, c, "cosine", np.inf, True, 1.0))
    pre = PREFILTER != "0"
    assert on.get("match_tile_cos") == 1 and on.get("match_finalize_value") == 1, on
    assert ("match_approx_cos_min" in on) == ("match_approx_cos_cand" in on) == ("match_exact_cos" in on) == ("match_prep_cos" in on) == pre, on
    assert not any(name in on for name in ("match_approx_min", "match_approx_cand", "match_exact", "match_prep", "match_tile", "match_finalize")), on


def test_cosine_prefilter_fallbacks_mixed_with_clean_pairs_then_a_clean_call():
    """fallback_case(64) in order and reversed (list overflow, slot overflow, a NaN row, 2^15, zeros -- under cosine a zero row is a pair whose bound
    cannot be stated -- beside clean pairs), each dirty pair alone, the wave-buffer flushes, the control pairs on the workspace all that left."""
    ctx, c = _ctx(), _case(mc.fallback_case, C0)
    k = _check(ctx, c, "cosine", np.inf, True, 1.0, "in order")
    kr = _check(ctx, _reordered(c, list(range(12, -1, -1))), "cosine", np.inf, True, 1.0, "reversed")
    assert kr == k[::-1] and 0 < k[mc.FB_CONTROL] and k[11] == 0
    for p in (1, 2, 3, 4, 5, 7, 8, 9, 10):
        kp = _check(ctx, _reordered(c, [p] * 8), "cosine", MAXD["cosine"], False, 1.0, "pair %d alone" % p)
        assert len(set(kp)) == 1
    for order, what in (([2, 0, 0, 0, 0, 0, 0, 0], "zeros first"), ([0, 0, 0, 0, 0, 0, 0, 8], "NaN row last")):
        ko = _check(ctx, _reordered(c, order), "cosine", np.inf, True, 1.0, what)
        assert ko.count(k[mc.FB_CONTROL]) >= 7
    _check(ctx, _case(mc.wave_flush_case, C0), "cosine", np.inf, True, 1.0, "wave flush")
    kc = _check(ctx, _case(mc.control_case, C0), "cosine", np.inf, True, 1.0, "8 x control after the dirty calls")
    assert kc == [k[mc.FB_CONTROL]] * 8


@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
def test_cosine_near_ties_multiples_clipping_zero_and_tiny_rows(cc):
    """match_metric_cases.cosine_near_tie_case: columns 1e-9 .. 1e-12 apart in cosine (below the filter's resolution: both must survive as
    candidates), exact ties between positive multiples, |c| > 1 by an ulp, a zero row and a 1e-30-scaled row -- clean pairs and fallback pairs in
    one call, then the same pairs the other way round."""
    ctx, c = _ctx(), _case(mm.cosine_near_tie_case, C0)
    k = _check(ctx, c, "cosine", np.inf, cc, 1.0, "near ties")
    assert _check(ctx, _reordered(c, list(range(7, -1, -1))), "cosine", np.inf, cc, 1.0, "near ties, reversed") == k[::-1]
    _check(ctx, c, "cosine", np.inf, cc, 0.8, "near ties, ratio")
    # the near-tie rows are decided by float64 both ways: some prefer the higher index, some the lower
    D = mm.distances(*mc.pair_inputs(c, 0), "cosine")
    first = [int(np.argmin(D[i])) == 2 * i for i in range(mm.CN_ROWS)]
    gaps = [abs(D[i, 2 * i] - D[i, 2 * i + 1]) for i in range(mm.CN_ROWS)]
    assert any(first) and not all(first) and all(set(np.argsort(D[i])[:2].tolist()) == {2 * i, 2 * i + 1} for i in range(mm.CN_ROWS))
    assert min(gaps) < 1e-10 and max(gaps) < 1e-8, (min(gaps), max(gaps))
    # clipping: some of the identical columns give exactly 0 because c was cut back to 1
    Dc = mm.distances(*mc.pair_inputs(c, 2), "cosine")
    zeros = sum(Dc[i, 5 * i] == 0.0 for i in range(mm.CN_ROWS))
    assert 4 <= zeros < mm.CN_ROWS and all(Dc[i, 5 * i + 1] == 2.0 for i in range(mm.CN_ROWS) if Dc[i, 5 * i] == 0.0)


# ------------------------------------------------------------------------------------------------ 3. sqeuclidean through the shared prefilter
def near_tie_case(C):
    """8 pairs of match_cases.near_ties at 150 x 300: columns one fp32 ulp of one component apart."""
    return mc._pack([mc.near_ties(np.random.default_rng(9500 + C + p), mc.FB_N, mc.FB_M, C) for p in range(8)], C, mc.FB_N, mc.FB_M)


@pytest.mark.parametrize("C", [64, 256])
def test_sqeuclidean_through_the_shared_prefilter(C):
    ctx = _ctx()
    for make in (mc.tile_edge_case, near_tie_case):
        c = _case(make, C)
        k = _check(ctx, c, "sqeuclidean", np.inf, True, 1.0, "%s C = %d" % (make.__name__, C))
        _check(ctx, c, "sqeuclidean", MAXD["sqeuclidean"] * C / 64.0, False, 0.8, "%s C = %d, finite, rows, ratio" % (make.__name__, C))
        assert 0 < sum(k)
    _, on = _launches(ctx, lambda: _run(ctx, c, "sqeuclidean", np.inf, True, 1.0))
    assert on.get("match_tile_sq") == 1 and on.get("match_finalize_value") == 1 and ("match_approx_min" in on) == ("match_exact" in on) == (PREFILTER != "0"), on


def test_the_root_merges_what_the_sum_keeps_apart():
    """root_merge_case: sums 1 + 2^-52 and 1 in columns 40 and 133 of row 21.  Euclidean (the option set to id 0) matches the row with column
    40, the first of two equal roots; sqeuclidean with column 133, the smaller sum -- from the prefilter (8 pairs) and from match_tile (3 pairs)."""
    ctx, c = _ctx(), _case(mm.root_merge_case, C0)
    for case in (c, _reordered(c, [0, 1, 2])):
        pe, _, ke, _ = _run(ctx, case, "euclidean", np.inf, True, 1.0)
        _check(ctx, case, "euclidean", np.inf, True, 1.0, "root merge")
        ps, ds, ks, _ = _run(ctx, case, "sqeuclidean", np.inf, True, 1.0)
        _check(ctx, case, "sqeuclidean", np.inf, True, 1.0, "root merge")
        for p in range(case["B"]):
            assert [mm.ROOT_ROW, mm.ROOT_COLS[0]] in pe[p, :ke[p]].tolist() and [mm.ROOT_ROW, mm.ROOT_COLS[1]] in ps[p, :ks[p]].tolist(), p
            at = ps[p, :ks[p], 0].tolist().index(mm.ROOT_ROW)
            assert ds[p, at] == 1.0


# ------------------------------------------------------------------------------------------------ 4. the ratio test on the value
@pytest.mark.parametrize("cc", [True, False], ids=["cross", "rows"])
@pytest.mark.parametrize("metric", ["cosine", "cityblock"])
def test_the_ratio_test_on_the_value(metric, cc):
    ctx, c = _ctx(), _case(mc.tile_edge_case, C0)
    kept = _check(ctx, c, metric, np.inf, cc, 0.8, "ratio")
    every = _check(ctx, c, metric, np.inf, cc, 1.0, "ratio off")
    assert 0 < sum(kept) < sum(every), (kept, every)
    _check(ctx, c, metric, MAXD[metric], cc, 0.8, "ratio, finite")
    _in_chunks(ctx, c, metric, np.inf, cc, 0.8, "ratio, match_tile")
    _, on = _launches(ctx, lambda: _run(ctx, c, metric, np.inf, cc, 0.8))
    assert on.get("match_finalize_value_ratio") == 1 and on.get({"cosine": "match_tile_cos2", "cityblock": "match_tile_l12"}[metric]) == 1, on
    assert ("match_approx_cos_min2" in on) == (metric == "cosine" and PREFILTER != "0"), on


# ------------------------------------------------------------------------------------------------ 5. id 0, refusals
@pytest.mark.parametrize("ratio", [1.0, 0.8])
def test_metric_0_is_the_untouched_context_launch_for_launch(ratio):
    ctx, c = _ctx(), _case(mc.tile_edge_case, C0)
    plain, launched = _launches(ctx, lambda: _run(ctx, c, None, np.inf, True, ratio))
    got, same = _launches(ctx, lambda: _run(ctx, c, 0, np.inf, True, ratio))
    assert same == launched, (same, launched)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got[:2], plain[:2])) and got[2:] == plain[2:]
    assert ("match_tile" if ratio == 1.0 else "match_tile2") in launched and not any("cos" in name or "value" in name for name in launched), launched


def test_refusals_on_a_live_context_and_the_counts_go_with_them():
    """An unknown metric id (5, -1) is KPB_E_UNSUPPORTED at kpb_ctx_set_option and a NaN ratio KPB_E_INVALID at kpb_match_ratio; after each,
    kpb_match_counts has nothing to report, the context's metric is what it was, and the context is usable."""
    from keypoint_bench_amd._lib import Context, KpbError
    ctx, c = _ctx(), _case(mc.tile_edge_case, C0)
    host = (ctypes.c_int32 * c["B"])()
    ctx.set_option(Context.OPT_MATCH_METRIC, ID["cosine"])
    try:
        for bad in (5, -1):
            _run(ctx, c, None, np.inf, True, 1.0)
            assert ctx.lib.kpb_match_counts(ctx.handle, host, c["B"]) == 0
            assert ctx.lib.kpb_ctx_set_option(ctx.handle, Context.OPT_MATCH_METRIC, bad) == -7
            assert ("unknown metric id %d" % bad).encode() in ctx.lib.kpb_last_error(ctx.handle)
            assert ctx.lib.kpb_match_counts(ctx.handle, host, c["B"]) == -1      # no completed match: the refused request's counts are nobody's
            pairs, dist, k, _ = _run(ctx, c, None, np.inf, True, 1.0)           # the metric is still cosine
            assert k == [len(_want(c, p, "cosine", np.inf, True, 1.0)[0]) for p in range(c["B"])]
    finally:
        ctx.set_option(Context.OPT_MATCH_METRIC, 0)
    _run(ctx, c, "cosine", np.inf, True, 1.0)
    assert ctx.lib.kpb_match_counts(ctx.handle, host, c["B"]) == 0
    with pytest.raises(KpbError) as e:
        _run(ctx, c, "cosine", np.inf, True, float("nan"))
    assert e.value.code == -1 and "max_ratio is NaN" in str(e.value), e.value
    assert ctx.lib.kpb_match_counts(ctx.handle, host, c["B"]) == -1
    _check(ctx, c, "cosine", np.inf, True, 1.0, "after the refusals")
    # back on euclidean: the call is kpb_match_ratio as it has always been
    assert _run(ctx, c, None, np.inf, True, 1.0)[2] == _run(ctx, c, "euclidean", np.inf, True, 1.0)[2]


def test_the_python_layers_leave_the_context_on_euclidean():
    """match_descriptors(metric="cosine") sets the option for its call only, also when the call raises."""
    from keypoint_bench_amd.utils.matcher import match_descriptors
    ctx, c = _ctx(), _case(mc.tile_edge_case, C0)
    a, b = (torch.from_numpy(v).to(DEV) for v in mc.pair_inputs(c, 7))
    got = match_descriptors(a, b, metric="cosine").cpu().numpy()
    np.testing.assert_array_equal(got, _want(c, 7, "cosine", np.inf, True, 1.0)[0])
    assert ctx._match_metric == 0
    with pytest.raises(ValueError):
        match_descriptors(a, b, metric="cosine", max_ratio=float("nan"))
    assert ctx._match_metric == 0
    np.testing.assert_array_equal(match_descriptors(a, b).cpu().numpy(), _want(c, 7, "euclidean", np.inf, True, 1.0)[0])


def test_calling_twice_gives_the_same_bits():
    ctx = _ctx()
    for metric, c in (("cosine", _case(mm.cosine_near_tie_case, C0)), ("sqeuclidean", _case(mc.fallback_case, C0)), ("chebyshev", _case(mc.tile_edge_case, C0))):
        first = _run(ctx, c, metric, np.inf, True, 1.0)
        again = _run(ctx, c, metric, np.inf, True, 1.0)
        assert first[2:] == again[2:]
        for p in range(c["B"]):
            K = first[2][p]
            assert np.array_equal(first[0][p, :K], again[0][p, :K]) and np.array_equal(first[1][p, :K].view(np.uint64), again[1][p, :K].view(np.uint64))


# ------------------------------------------------------------------------------------------------ 6. the Python layers
EP = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
COS = dict(metric="cosine", max_distance=float("inf"), cross_check=True)
PIPE_B, PIPE_H, PIPE_W, PIPE_SEED = 8, 64, 96, 300


def test_python_layers_read_the_metric():
    """ALIKE-t at 64 x 96: match_descriptors(metric="cosine") is the expectation on the sampled descriptors, brute_force_matcher returns those rows,
    a PairPipeline of 8 pairs gives what eight single-pair calls give -- and not what euclidean gives, on at least one pair."""
    from keypoint_bench_amd import synthetic
    from keypoint_bench_amd.models.ALike import alike_t
    from keypoint_bench_amd.pipeline import PairPipeline
    from keypoint_bench_amd.utils.extracter import detection
    from keypoint_bench_amd.utils.matcher import brute_force_matcher, match_descriptors, sample_descriptors
    B, H, W = PIPE_B, PIPE_H, PIPE_W
    v = [synthetic.image_pair(PIPE_SEED + i, H, W) for i in range(B)]
    i0, i1 = np.stack([a for a, _ in v]), np.stack([b for _, b in v])
    net = alike_t(dense_descriptors=True).eval()
    pipe = PairPipeline(net, EP, COS, B, H, W, device=DEV)
    pipe.run(torch.from_numpy(np.concatenate([i0, i1])).to(DEV))
    single = alike_t(dense_descriptors=True).eval()
    differ = 0
    for b in range(B):
        s0, d0 = single(torch.from_numpy(i0[b])[None].to(DEV))
        k0 = detection(s0, EP)
        f0 = sample_descriptors(k0, d0)
        s1, d1 = single(torch.from_numpy(i1[b])[None].to(DEV))
        k1 = detection(s1, EP)
        f1 = sample_descriptors(k1, d1)
        wp, wd, _ = mm.expect(f0.cpu().numpy(), f1.cpu().numpy(), "cosine")
        assert 0 < len(wp), b
        pairs, dist = match_descriptors(f0, f1, metric="cosine", return_distance=True)
        np.testing.assert_array_equal(pairs.cpu().numpy(), wp)
        _same_values(dist.cpu().numpy(), wd, "match_descriptors, pair %d" % b)
        m0, m1 = brute_force_matcher(k0, k1, d0, d1, COS)
        np.testing.assert_array_equal(m0.cpu().numpy(), k0.cpu().numpy()[wp[:, 0]])
        np.testing.assert_array_equal(m1.cpu().numpy(), k1.cpu().numpy()[wp[:, 1]])
        got = pipe.pair(b)
        np.testing.assert_array_equal(got["pairs"], wp)
        _same_values(got["dist"], wd, "pipeline, pair %d" % b)
        np.testing.assert_array_equal(got["m0"], m0.cpu().numpy())
        np.testing.assert_array_equal(got["m1"], m1.cpu().numpy())
        eu = match_descriptors(f0, f1, metric="euclidean").cpu().numpy()
        np.testing.assert_array_equal(eu, mm.expect(f0.cpu().numpy(), f1.cpu().numpy(), "euclidean")[0])
        differ += int(eu.shape != wp.shape or not np.array_equal(eu, wp))
        for metric in ("sqeuclidean", "cityblock", "chebyshev"):
            np.testing.assert_array_equal(match_descriptors(f0, f1, metric=metric).cpu().numpy(), mm.expect(f0.cpu().numpy(), f1.cpu().numpy(), metric)[0])
    print("cosine and euclidean matches differ on %d of %d pairs" % (differ, B))
    assert differ >= 1
