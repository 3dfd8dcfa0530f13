"""Inputs of the match-prefilter and descriptor-sampling edge tests, built with numpy alone from fixed seeds.  tests/test_oracle_match_edge.py
and tests/test_oracle_sample_edge.py check the oracle on them without a GPU, tests/test_gpu_match_prefilter.py hands the same arrays to
kpb_match / kpb_sample: the oracle is pinned on exactly what the kernels see.

A match case is a dict: a [B, max_n, C] and b [B, max_m, C] float32, n and m [B] int32 (each pair's own counts), B, C, max_n, max_m.
Rows beyond a pair's counts are DECOYS: exact copies of rows of the other side, so a kernel that read one would find a distance of
zero and a match the oracle (which is handed a[p, :n[p]], b[p, :m[p]] only) does not have.

The numbers quoted in the docstrings are those of csrc/match.hip: MTI = 64 rows and MTJ = 128 columns per slot tile (a row has
ceil(m / 128) slots for its candidates, a column ceil(n / 64), both from the pair's OWN counts), 16 RT rows per wave and 64 RT per
workgroup of match_approx<KB, RT>, a candidate list of cap = 8 (max_n + max_m) entries per pair, a wave buffer of CBUF = 192 entries flushed
above 128, and match_margin(na, nb, C) = (7.5e-6 + 6e-7 C)(na + nb) + 5e-6 (sqrt na + sqrt nb) on SQUARED distances, evaluated for a
row with the largest column norm of the pair and for a column with the largest row norm."""
import numpy as np

RT_OF = {32: 4, 64: 4, 96: 2, 128: 2, 160: 1, 192: 1, 224: 1, 256: 1}      # kpb_match's launch table: KB = C / 32 -> RT
SIGMA = 0.05


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def noisy_pair(rng, n, m, C, sigma=SIGMA):
    """a [n, C] normal; b [m, C] normal with its first min(n, m) // 2 rows noisy copies (sigma) of distinct, permuted rows of a.  A copy
    lies at a squared distance of ~C sigma^2 = 0.0025 C, every other column at ~2 C."""
    a = rng.normal(size=(n, C)).astype(np.float32)
    b = rng.normal(size=(m, C)).astype(np.float32)
    k = min(n, m) // 2
    if k:
        b[:k] = a[rng.permutation(n)[:k]] + sigma * rng.normal(size=(k, C)).astype(np.float32)
    return a, b


def _pack(pairs, C, max_n, max_m):
    """[(a_p, b_p)] with their own row counts -> a case; decoys beyond the counts."""
    B = len(pairs)
    a = np.zeros((B, max_n, C), np.float32)
    b = np.zeros((B, max_m, C), np.float32)
    n = np.array([len(x) for x, _ in pairs], np.int32)
    m = np.array([len(y) for _, y in pairs], np.int32)
    for p, (x, y) in enumerate(pairs):
        assert x.dtype == np.float32 and y.dtype == np.float32 and len(x) <= max_n and len(y) <= max_m
        a[p, : n[p]], b[p, : m[p]] = x, y
        fill = np.random.default_rng(1000 + p).normal(size=(max(max_n, max_m), C)).astype(np.float32)
        srcb = y if m[p] and np.isfinite(y).all() else fill      # a's spare rows copy b's rows and the reverse
        srca = x if n[p] and np.isfinite(x).all() else fill
        a[p, n[p]:] = srcb[np.arange(max_n - n[p]) % len(srcb)]
        b[p, m[p]:] = srca[np.arange(max_m - m[p]) % len(srca)]
    return dict(a=a, b=b, n=n, m=m, B=B, C=C, max_n=max_n, max_m=max_m)


def reorder(case, order):
    """The same pairs in another order (new arrays: the case is shared and stays as it is)."""
    order = np.asarray(order)
    out = dict(case)
    out.update(a=_f32(case["a"][order]), b=_f32(case["b"][order]), n=case["n"][order].copy(), m=case["m"][order].copy(), B=len(order))
    return out


def pair_inputs(case, p):
    """What pair p really consists of: the oracle's arguments."""
    return case["a"][p, : case["n"][p]], case["b"][p, : case["m"][p]]


# ------------------------------------------------------------------------------------------------ every channel form at its tile edges
TIE_PAIR = 6        # the pair of tile_edge_case that is rounded to integers


def tile_edge_counts(C):
    """n and m of the 8 pairs.  n takes each of {0, 1, 16 RT - 1, 16 RT, 16 RT + 1, 64 RT, 64 RT + 1, max_n} once (a wave's rows and a
    workgroup's rows, plus or minus one), m every one of {0, 1, 128, 129, 143, 144, 145} (the slot tile and the 16-column block, plus or
    minus one).  The pairs whose n is past one slot tile (n >= 65) all get m >= 129: four of them at RT = 4; at RT = 2 and RT = 1 the n
    set itself holds only three (33, 128, 129, 145 -> 128, 129, 145) and two (65, 81) such values in 8 pairs."""
    RT = RT_OF[C]
    max_n, max_m = 64 * RT + 17, 145
    n = np.array([0, 1, 16 * RT - 1, 16 * RT, 16 * RT + 1, 64 * RT, 64 * RT + 1, max_n], np.int32)
    m = np.array([129, 0, 128, 1, 143, 144, 145, 129], np.int32)
    assert set(m.tolist()) == {0, 1, 128, 129, 143, 144, 145} and len(set(n.tolist())) == 8
    assert int(((n >= 65) & (m >= 129)).sum()) == min(4, int((n >= 65).sum())) >= 2
    return n, m, max_n, max_m


def tile_edge_case(C):
    n, m, max_n, max_m = tile_edge_counts(C)
    rng = np.random.default_rng(4000 + C)
    pairs = [noisy_pair(rng, int(n[p]), int(m[p]), C) for p in range(8)]
    pairs[TIE_PAIR] = tuple(np.round(v) for v in pairs[TIE_PAIR])       # integer components: exact ties between distances
    return _pack(pairs, C, max_n, max_m)


# ------------------------------------------------------------------------------------------------ the fallbacks, alone and mixed
FB_N, FB_M = 150, 300       # 3 x 3 slot tiles, cap = 8 * 450 = 3600


def fb_control(rng, C):
    """Noisy copies.  NO fallback: components of a few units (far below 2^15, finite); a row's margin is ~(7.5e-6 + 6e-7 C) 2 C
    (0.006 at C = 64, 0.03 at C = 160) on squared distances of 0.0025 C for its copy against ~2 C (least of 300: ~C) for every other
    column, so a row or a column lists one candidate, rarely two: ~450 entries against the cap of 3600, at most 2 against 3 slots."""
    return noisy_pair(rng, FB_N, FB_M, C)


def fb_same_vector(rng, C):
    """Every row of both sides is one vector.  LIST OVERFLOW: all approximate distances are the same number, so each of the 150 x 300 =
    45 000 entries is a row and a column candidate -- 12.5 times cap = 3600; flush() raises the flag for what does not fit."""
    v = rng.normal(size=(1, C)).astype(np.float32)
    return np.repeat(v, FB_N, 0), np.repeat(v, FB_M, 0)


def fb_zeros(rng, C):
    """All-zero descriptors.  LIST OVERFLOW: norms 0, so match_margin is 0, and every approximate distance is +0 <= rowmin + 0: 45 000
    candidates against 3600, without any margin's help."""
    return np.zeros((FB_N, C), np.float32), np.zeros((FB_M, C), np.float32)


def fb_common_offset(rng, C):
    """Every row is one shared vector of components ~8 plus 1e-4 x normal (un-normalised descriptors riding on a large common part).
    LIST OVERFLOW: squared norms are ~64 C, the margin (7.5e-6 + 6e-7 C) 128 C is 0.38 at C = 64 and 2.1 at C = 160, while all true squared
    distances are ~2e-8 C: every entry lies within the margin (45 000 against 3600).  float64 separates them all (one fp32 ulp of 8 is 1e-6,
    a hundredth of the perturbation)."""
    v = (8.0 + 0.25 * rng.normal(size=(1, C))).astype(np.float32)
    return (_f32(v + 1e-4 * rng.normal(size=(FB_N, C))), _f32(v + 1e-4 * rng.normal(size=(FB_M, C))))


FB_ROW_OVER = (7, (3, 40, 170, 290))        # row, its four identical columns (16-column blocks 0, 2, 10, 18; slot tiles 0, 0, 1, 2)


def fb_row_slots(rng, C):
    """Ordinary pair in which four columns are the SAME noisy copy of a[7].  SLOT OVERFLOW: the four approximate distances of row 7 are
    equal, so match_exact files four row candidates under row 7: rcnt reaches 4 > slots_r = ceil(300 / 128) = 3."""
    a, b = noisy_pair(rng, FB_N, FB_M, C)
    i, cols = FB_ROW_OVER
    b[list(cols)] = a[i] + SIGMA * rng.normal(size=C).astype(np.float32)
    return a, b


FB_COL_OVER = (9, (5, 30, 70, 140))         # column, its four identical rows (16-row tiles 0, 1, 4, 8)


def fb_col_slots(rng, C):
    """Four identical rows of A near b[9].  SLOT OVERFLOW: four column candidates under column 9: ccnt reaches 4 > slots_c =
    ceil(150 / 64) = 3."""
    a, b = noisy_pair(rng, FB_N, FB_M, C)
    j, rows = FB_COL_OVER
    a[list(rows)] = b[j] + SIGMA * rng.normal(size=C).astype(np.float32)
    return a, b


def fb_at_the_limit(rng, C):
    """Ten rows with exactly 3 identical nearest columns each, ten columns with exactly 3 identical nearest rows each, all at scattered
    indices.  NO fallback: rcnt and ccnt reach 3 = slots_r = slots_c, the last value `t < slots` admits (4.0 C sigma^2 apart from
    everything else: no fourth candidate within the margin).  The three slots are filled in the order of the atomics, not of the
    indices: match_finalize must still return the lowest index of the tie."""
    a = rng.normal(size=(FB_N, C)).astype(np.float32)
    b = rng.normal(size=(FB_M, C)).astype(np.float32)
    rows, cols = rng.permutation(FB_N), rng.permutation(FB_M)
    for k in range(10):
        b[cols[3 * k: 3 * k + 3]] = a[rows[k]] + SIGMA * rng.normal(size=C).astype(np.float32)
    for k in range(10):
        a[rows[10 + 3 * k: 13 + 3 * k]] = b[cols[30 + k]] + SIGMA * rng.normal(size=C).astype(np.float32)
    return a, b


FB_OWN_M = 100


def fb_own_count(rng, C):
    """n = 150, m = 100 inside max_m = 300; columns 20 and 61 are the same noisy copy of a[33].  SLOT OVERFLOW: match_exact takes slots_r
    from the pair's own m, ceil(100 / 128) = 1 (match_finalize reads no more for it), not from max_m (3): row 33's second candidate
    raises the flag.  From max_m it would be filed in a slot nobody reads, and which of the two columns wins would be the order of two
    atomics.  That order usually follows the list, which a wave fills in ascending j -- so row 90 has a second pair of columns where
    it must not: column 70 is a noisy copy of a[90] and column 15 the same copy with one component moved 4 ulps AWAY from a[90].  Both are
    candidates (the filter cannot tell them apart), float64 prefers the later one."""
    a, b = noisy_pair(rng, FB_N, FB_OWN_M, C)
    for i in (33, 90):          # (the copies noisy_pair may have made of these two rows go)
        near = np.flatnonzero(((b - a[i]) ** 2).sum(1) < 0.1 * C)
        b[near] = rng.normal(size=(len(near), C)).astype(np.float32)
    b[[20, 61]] = a[33] + SIGMA * rng.normal(size=C).astype(np.float32)
    c = (a[90] + SIGMA * rng.normal(size=C)).astype(np.float32)
    far = c.copy()
    far[0] = c[0] + np.float32(4.0 if c[0] > a[90, 0] else -4.0) * np.spacing(np.abs(c[0]))
    b[70], b[15] = c, far
    return a, b


def fb_nan_row(rng, C):
    """A NaN row in A.  FALLBACK (non-finite): its squared norm is NaN, `!(nn < 3.0e38f)` in match_prep raises the flag; match_approx and
    match_exact return at once for the pair.  numpy.argmin: the NaN row is every column's arg-minimum."""
    a, b = noisy_pair(rng, FB_N, FB_M, C)
    a[12] = np.nan
    return a, b


FB_BIG = (40, 5)


def fb_two_to_15(rng, C, value=np.float32(32768.0)):
    """One component exactly 32768.0.  FALLBACK (range): `big >= 32768.0f` in match_prep, the half-precision hi piece would saturate."""
    a, b = noisy_pair(rng, FB_N, FB_M, C)
    a[FB_BIG] = value
    return a, b


def fb_below_two_to_15(rng, C):
    """The same pair (same seed) with that component at nextafter(32768, 0) = 32767.998.  match_prep raises NO flag: big < 32768, the
    norm 1.07e9 is far below 3e38, and the split is exact to 2^-20 (hi 32752, lo 15.99).  The pair still ends on match_tile, through the
    list: row 40's norm is the pair's largest row norm, which enters EVERY column's margin -- match_margin(1.07e9, nb, C) is 5e4 at
    C = 64 against squared distances of ~2 C -- so all 149 x 300 other entries are column candidates: 44 700 against 3600.  (That costs time
    on such a pair, never bits: what this pair checks is that neither path is wrong one ulp below the range test.  The filter itself at
    the top of its range is top_of_range_case below.)"""
    return fb_two_to_15(rng, C, np.nextafter(np.float32(32768.0), np.float32(0.0)))


def fb_empty(rng, C):
    """n = 0.  Empty result: match_prep touches no row of A, match_approx's workgroups return on `i0 >= n`, match_finalize writes 0."""
    return np.zeros((0, C), np.float32), noisy_pair(rng, FB_N, FB_M, C)[1]


NEAR_ROWS = 60


def near_ties(rng, n, m, C, rows=NEAR_ROWS):
    """For `rows` rows, columns 2i and 2i+1 are a noisy copy of a[i] and the same copy with component i % C moved by one fp32 ulp, up for
    even i and down for odd i.  The two squared distances differ by ~2 sigma ulp = 1e-8 relative: float64 tells them apart, the fp32
    approximate distance (and the 22-bit split operands) cannot.  The next `rows` rows hold graded ties (below)."""
    a = rng.normal(size=(n, C)).astype(np.float32)
    b = rng.normal(size=(m, C)).astype(np.float32)
    for i in range(rows):
        c = (a[i] + SIGMA * rng.normal(size=C)).astype(np.float32)
        d = c.copy()
        k = i % C
        d[k] = np.nextafter(c[k], np.float32(np.inf if i % 2 == 0 else -np.inf))
        b[2 * i], b[2 * i + 1] = c, d
    # graded ties behind them: the same with a move of 2^(i % 12) ulps, 1 .. 2048: squared distances 1e-8 .. 2e-5 apart (C = 64), from
    # far below the filter's actual error (an fp32 ulp of na + nb - 2 ab is 1.5e-5) to about it and always far inside its margin (6e-3)
    for i in range(rows, min(2 * rows, n, m // 2)):
        c = (a[i] + SIGMA * rng.normal(size=C)).astype(np.float32)
        d = c.copy()
        k = i % C
        step = np.float32(2.0 ** (i % 12)) * np.spacing(np.abs(c[k]))
        d[k] = c[k] + (step if i % 2 == 0 else -step)
        b[2 * i], b[2 * i + 1] = c, d
    return a, b


def fb_near_ties(rng, C):
    """Near-ties below the filter's resolution (near_ties).  NO fallback: two candidates per row against 3 slots, ~600 entries in all.
    BOTH columns must survive as row candidates: a filter that kept its own arg-minimum alone, or a margin below the filter's error, returns
    the lower index where float64 prefers the higher one (about half of the 60 rows, and of the 60 graded ones behind them)."""
    return near_ties(rng, FB_N, FB_M, C)


FALLBACK_PAIRS = [fb_control, fb_same_vector, fb_zeros, fb_common_offset, fb_row_slots, fb_col_slots, fb_at_the_limit, fb_own_count,
                  fb_nan_row, fb_two_to_15, fb_below_two_to_15, fb_empty, fb_near_ties]
FB_CONTROL, FB_LIMIT, FB_NEAR = 0, 6, 12


def fallback_case(C):
    """The 13 pairs in the order of FALLBACK_PAIRS.  Pairs 9 and 10 share a seed: they differ in the one component."""
    seeds = [5000 + C + 17 * p for p in range(13)]
    seeds[10] = seeds[9]
    return _pack([f(np.random.default_rng(s), C) for f, s in zip(FALLBACK_PAIRS, seeds)], C, FB_N, FB_M)


def control_case(C, copies=8):
    """`copies` times the control pair of fallback_case(C), alone: the call that follows the dirty ones."""
    return _pack([fb_control(np.random.default_rng(5000 + C), C)] * copies, C, FB_N, FB_M)


def top_of_range_case(C=64):
    """8 pairs of 70 x 140 whose descriptors are noisy copies times 2^12 with one component of each side set to nextafter(32768, 0): the
    whole pair sits at the top of the range match_prep admits, so the margins (which scale with the norms) stay small against the
    distances and the FILTER decides these pairs, one ulp below the saturation of its hi pieces."""
    top = np.nextafter(np.float32(32768.0), np.float32(0.0))
    pairs = []
    for p in range(8):
        rng = np.random.default_rng(5500 + p)
        a, b = noisy_pair(rng, 70, 140, C)
        a, b = a * np.float32(4096.0), b * np.float32(4096.0)
        assert max(np.abs(a).max(), np.abs(b).max()) < 32768.0
        a[3 + p, p] = top
        b[9 * p, C - 1 - p] = -top
        pairs.append((a, b))
    return _pack(pairs, C, 70, 140)


# ------------------------------------------------------------------------------------------------ the wave buffer flushes mid-loop
WF_N, WF_M, WF_ROWS = 130, 520, 64


def wave_flush_case(C=64):
    """8 pairs of 130 x 520 (5 row slots, cap = 5200).  Rows 0..63 -- ONE wave of match_approx<2, 4> -- have 4 identical nearest
    columns each, at j, j + 130, j + 260, j + 390: 256 candidates in that wave's buffer, which is flushed whenever it holds more than
    128, so twice inside the column loop and once after it.  4 <= 5 slots and ~600 entries in all: no fallback."""
    pairs = []
    for p in range(8):
        rng = np.random.default_rng(6000 + p)
        a = rng.normal(size=(WF_N, C)).astype(np.float32)
        b = rng.normal(size=(WF_M, C)).astype(np.float32)
        for j in range(WF_ROWS):
            b[[j, j + 130, j + 260, j + 390]] = a[j] + SIGMA * rng.normal(size=C).astype(np.float32)
        pairs.append((a, b))
    return _pack(pairs, C, WF_N, WF_M)


# ------------------------------------------------------------------------------------------------ kpb_sample at its edges
SAMPLE_MAPS = [(5, 1, 7), (3, 6, 1), (2, 1, 1), (65, 4, 5), (512, 3, 4), (1, 9, 9)]        # (C, Hd, Wd)
SAMPLE_COUNTS = (1, 2, 3, 5)        # the four-keypoint group of sample_bilinear and its tail


def sample_points():
    """[23, 2] normalised (x, y): the four corners, then 1 - 1e-7 (the last texel from below), -0.01 and 1.02 (one tap off the map), -0.2,
    1.3 and 2.5 (all taps off the map on most maps: zero padding) on either axis and on both, then interior points.  23 = 5 groups
    of four and a tail of three."""
    pts = [(0, 0), (1, 1), (0, 1), (1, 0)]
    for v in (1 - 1e-7, -0.01, 1.02, -0.2, 1.3, 2.5):
        pts += [(v, 0.37), (0.61, v), (v, v)]
    pts += [(0.5, 0.5)]
    p = np.array(pts, np.float32)
    assert p.shape == (23, 2) and p[4, 0] < 1.0
    return p


def sample_map(C, Hd, Wd, seed=0):
    return np.random.default_rng(7000 + seed + C + 31 * Hd + 7 * Wd).normal(size=(C, Hd, Wd)).astype(np.float32)
