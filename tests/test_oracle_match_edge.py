"""M2 edge semantics of the oracle against scipy.cdist + skimage's documented glue (tests/golden/skimage_standin.py):
NaN descriptors (numpy.argmin: the first NaN wins), infinite distances, and the `max_distance < inf` guard.  Then the families of
tests/match_cases.py, on which tests/test_gpu_match_prefilter.py compares kpb_match with this oracle bit for bit."""
import os
import sys

import numpy as np
import pytest

import match_cases as mc
import oracle
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import skimage_standin  # noqa: E402


def cases():
    rng = np.random.default_rng(21)
    a = rng.normal(size=(40, 8)).astype(np.float32)
    b = (a[rng.permutation(40)][:33] + 0.05 * rng.normal(size=(33, 8))).astype(np.float32)
    yield "plain", a, b
    a2, b2 = a.copy(), b.copy()
    a2[[3, 17]] = np.nan
    b2[5] = np.nan
    yield "nan_rows", a2, b2
    a3, b3 = a.copy(), b.copy()
    a3[7, 0] = np.inf
    yield "inf_row", a3, b3


@pytest.mark.parametrize("maxd", [np.inf, 1.0])
@pytest.mark.parametrize("cc", [True, False])
def test_match_edges_equal_scipy_glue(maxd, cc):
    for name, a, b in cases():
        with np.errstate(invalid="ignore"):
            want = skimage_standin.match_descriptors(a, b, metric="euclidean", max_distance=maxd, cross_check=cc)
            wd = skimage_standin.distances_of(a, b, want)
        got, gd = oracle.match(a, b, maxd, cc)
        assert np.array_equal(got, want), (name, maxd, cc, got.tolist(), want.tolist())
        assert np.array_equal(gd, wd, equal_nan=True), (name, maxd, cc)


# ------------------------------------------------------------------------------------------------ the families of tests/match_cases.py
# What tests/test_gpu_match_prefilter.py feeds kpb_match, at its sizes: the oracle it compares with is itself right on them.
def _families():
    for C in (64, 160):
        case = mc.fallback_case(C)
        for p, f in enumerate(mc.FALLBACK_PAIRS):
            yield "%s C=%d" % (f.__name__, C), C, mc.pair_inputs(case, p)
    yield "wave_flush", 64, mc.pair_inputs(mc.wave_flush_case(), 0)
    yield "top_of_range", 64, mc.pair_inputs(mc.top_of_range_case(), 0)
    for C in (32, 256):
        yield "tile_edge ties C=%d" % C, C, mc.pair_inputs(mc.tile_edge_case(C), mc.TIE_PAIR)


FAMILIES = list(_families())


@pytest.mark.parametrize("finite", [False, True])
@pytest.mark.parametrize("cc", [True, False])
def test_match_families_equal_scipy_glue(cc, finite):
    for name, C, (a, b) in FAMILIES:
        maxd = (0.5 * float(np.sqrt(C)) * (4096.0 if name == "top_of_range" else 1.0)) if finite else np.inf
        got, gd = oracle.match(a, b, maxd, cc)
        if len(a) == 0:     # (argmin of an empty axis raises in numpy; the reference's matcher returns no match before it gets there)
            assert len(got) == 0 and len(gd) == 0, name
            continue
        with np.errstate(invalid="ignore"):
            want = skimage_standin.match_descriptors(a, b, metric="euclidean", max_distance=maxd, cross_check=cc)
            wd = skimage_standin.distances_of(a, b, want)
        assert np.array_equal(got, want), (name, maxd, cc)
        assert np.array_equal(gd.view(np.uint64), wd.view(np.uint64)), (name, maxd, cc)
        if finite and "control" in name:     # the finite bound cuts: copies stay, chance neighbours go
            assert 60 < len(got) < len(oracle.match(a, b, np.inf, cc)[0]), (name, len(got))


def test_near_tie_family_is_decided_by_float64_alone():
    """Both columns of a near-tie are distinct in float64 and the true nearest is the odd (perturbed) one in about half of the rows --
    while their float32 distances are within an ulp or two: a filter that kept one column of the two could not know which."""
    from scipy.spatial.distance import cdist
    for C in (64, 160):
        a, b = mc.pair_inputs(mc.fallback_case(C), mc.FB_NEAR)
        d = cdist(a[: mc.NEAR_ROWS], b[: 2 * mc.NEAR_ROWS])
        r = np.arange(mc.NEAR_ROWS)
        even, odd = d[r, 2 * r], d[r, 2 * r + 1]
        assert (even != odd).all() and (np.argmin(d, axis=1) // 2 == r).all()
        frac = float((odd < even).mean())
        print("C = %d: the odd column is the nearest in %.0f %% of the rows; largest relative gap %.2g" % (C, 100 * frac, (np.abs(even - odd) / even).max()))
        assert 0.3 <= frac <= 0.7
        assert (np.abs(even - odd) <= 2.5e-7 * even).all()      # two fp32 ulps of the distance
        got, _ = oracle.match(a, b, np.inf, False)
        assert np.array_equal(got[: mc.NEAR_ROWS, 1], 2 * r + (odd < even))
        g = np.arange(mc.NEAR_ROWS, 2 * mc.NEAR_ROWS)       # the graded ties behind them: 1 .. 2048 ulps, still one or the other
        dg = cdist(a[g], b)
        assert np.array_equal(np.argmin(dg, axis=1) // 2, g) and np.array_equal(got[g, 1], np.argmin(dg, axis=1))
        assert 0.3 <= float((got[g, 1] % 2).mean()) <= 0.7
        gap = np.abs(dg[g - g[0], 2 * g] ** 2 - dg[g - g[0], 2 * g + 1] ** 2)
        print("C = %d: graded ties, squared distances %.2g .. %.2g apart" % (C, gap.min(), gap.max()))
        assert 0 < gap.min() and gap.max() < 1e-3


def test_at_the_limit_family_has_its_triples():
    """Ten rows with three exactly equal nearest columns, ten columns with three exactly equal nearest rows; the lowest index wins."""
    from scipy.spatial.distance import cdist
    a, b = mc.pair_inputs(mc.fallback_case(64), mc.FB_LIMIT)
    d = cdist(a, b)
    # (a chance neighbour of a tripled column or row is a three-way tie as well; the planted ones are the copies, at ~0.05 sqrt(C))
    rows3 = [i for i in range(len(a)) if (d[i] == d[i].min()).sum() == 3 and d[i].min() < 1.0]
    cols3 = [j for j in range(len(b)) if (d[:, j] == d[:, j].min()).sum() == 3 and d[:, j].min() < 1.0]
    assert len(rows3) == 10 and len(cols3) == 10
    assert max((d[i] == d[i].min()).sum() for i in range(len(a))) == 3 and max((d[:, j] == d[:, j].min()).sum() for j in range(len(b))) == 3
    got = dict(oracle.match(a, b, np.inf, True)[0].tolist())
    for i in rows3:
        assert got[i] == int(np.flatnonzero(d[i] == d[i].min())[0])
    firsts = [int(np.flatnonzero(d[:, j] == d[:, j].min())[0]) for j in cols3]
    assert [got[i] for i in firsts] == cols3
    assert any(np.flatnonzero(d[i] == d[i].min())[0] > 128 for i in rows3)      # ties that live in later slot tiles only


def test_own_count_family_prefers_the_later_of_two_columns_in_one_row():
    """Row 33 has an exact duplicate of its nearest column (the first wins), row 90 a near-duplicate in FRONT of its nearest column."""
    for C in (64, 160):
        a, b = mc.pair_inputs(mc.fallback_case(C), mc.FALLBACK_PAIRS.index(mc.fb_own_count))
        assert len(b) == mc.FB_OWN_M
        got = dict(oracle.match(a, b, np.inf, False)[0].tolist())
        assert got[33] == 20 and np.array_equal(b[20], b[61])
        assert got[90] == 70 and np.abs(b[70] - b[15]).max() < 1e-6
