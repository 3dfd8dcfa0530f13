"""The expectation of the brute-force matcher's metrics (KPB_OPT_MATCH_METRIC, the metric key of brute_force_params) and the inputs that belong
to the new metrics alone.  A helper, not a test: tests/test_match_metric_cpu.py pins `distances` on the live scipy.spatial.distance.cdist and
`expect` on tests/golden/skimage_standin without a GPU; tests/test_gpu_match_metric.py holds the kernels to `expect`, bit for bit.

`distances` restates each metric in numpy, float64, round to nearest, one operation at a time (x = (double)a_i[k], y = (double)b_j[k]):

    sqeuclidean   s = sum_k (x - y)(x - y), ONE accumulator, ascending k (numpy.cumsum is that loop); no root
    cityblock     s = sum_k |x - y|, one accumulator, ascending k
    chebyshev     acc = 0; ascending k: if |x - y| > acc: acc = |x - y| -- a NaN term is skipped, inf wins: numpy.fmax, not numpy.maximum
    cosine        TWO accumulators: even k into e, odd k into o, each ascending, over k < 2 floor(C / 2); sum = e + o; an odd C adds its last
                  term.  That sum three times: dot = sum x y (the product rounded, then added), |a|^2, |b|^2.  c = dot / (sqrt |a|^2 sqrt |b|^2),
                  c = copysign(1, c) where |c| > 1, D = 1 - c.  A zero or non-finite row gives NaN.
    euclidean     sqrt of sqeuclidean's sum (what oracle.match has always pinned; here for the comparison of the two orders)

scipy's cosine bits depend on how scipy was built (the x86-64 wheel of 1.15.3 runs the two lanes above; a single accumulator differs from it from
C = 32 on), so the definition stands in its own terms and the CPU test says how it compares with the scipy at hand."""
import numpy as np

import match_cases as mc

METRICS = ("euclidean", "sqeuclidean", "cityblock", "chebyshev", "cosine")
NEW_METRICS = METRICS[1:]
EPS = float(np.finfo(np.double).eps)


def _sum1(t):
    """One accumulator over the last axis, ascending."""
    if t.shape[-1] == 0:
        return np.zeros(t.shape[:-1], np.float64)
    return np.cumsum(t, axis=-1)[..., -1]


def _sum2(t):
    """Two lanes over the last axis (even k, odd k), e + o, then the last term of an odd width."""
    C = t.shape[-1]
    h = C // 2 * 2
    s = _sum1(t[..., 0:h:2]) + _sum1(t[..., 1:h:2])
    if C % 2:
        s = s + t[..., -1]
    return s


def distances(a, b, metric):
    """[n, m] float64: the metric's value for every pair of rows of a [n, C] and b [m, C]."""
    assert metric in METRICS, metric
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n, m = a.shape[0], b.shape[0]
    D = np.empty((n, m), np.float64)
    with np.errstate(all="ignore"):
        if metric == "cosine":
            na, nb = np.sqrt(_sum2(a * a)), np.sqrt(_sum2(b * b))
        for i0 in range(0, n, 32):          # (blocks of rows: [32, m, C] float64 at a time)
            x = a[i0:i0 + 32, None, :]
            if metric == "cosine":
                c = _sum2(x * b[None]) / (na[i0:i0 + 32, None] * nb[None, :])
                c = np.where(np.abs(c) > 1.0, np.copysign(1.0, c), c)
                D[i0:i0 + 32] = 1.0 - c
                continue
            d = x - b[None]
            if metric == "chebyshev":
                D[i0:i0 + 32] = np.fmax.reduce(np.abs(d), axis=-1, initial=0.0)
            elif metric == "cityblock":
                D[i0:i0 + 32] = _sum1(np.abs(d))
            else:
                s = _sum1(d * d)
                D[i0:i0 + 32] = np.sqrt(s) if metric == "euclidean" else s
    return D


def glue(D, max_distance=np.inf, cross_check=True, max_ratio=1.0):
    """skimage.feature.match_descriptors (>= 0.16) after its cdist call, on a given distance matrix: (pairs int64 [K, 2], values float64 [K],
    ratios float64 [K'] of the rows that reached the ratio step).  The steps are those of `expect` in tests/test_match_ratio_cpu.py."""
    if D.shape[0] == 0 or D.shape[1] == 0:
        return np.zeros((0, 2), np.int64), np.zeros((0,), np.float64), np.zeros((0,), np.float64)
    i1 = np.arange(D.shape[0])
    i2 = np.argmin(D, axis=1)
    if cross_check:
        mask = i1 == np.argmin(D, axis=0)[i2]
        i1, i2 = i1[mask], i2[mask]
    if max_distance < np.inf:
        mask = D[i1, i2] < max_distance
        i1, i2 = i1[mask], i2[mask]
    best = D[i1, i2].copy()
    modified = D.copy()
    modified[i1, i2] = np.inf
    second = modified[i1, np.argmin(modified[i1], axis=1)] if len(i1) else np.zeros((0,), np.float64)
    second[second == 0] = EPS
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = best / second
    if max_ratio < 1.0:
        mask = ratio < max_ratio
        i1, i2, best = i1[mask], i2[mask], best[mask]
    return np.stack([i1, i2], 1).astype(np.int64), best, ratio


def expect(a, b, metric, max_distance=np.inf, cross_check=True, max_ratio=1.0):
    return glue(distances(a, b, metric), max_distance, cross_check, max_ratio)


# ------------------------------------------------------------------------------------------------ rows that are special for cosine
def special_rows(C, seed=0):
    """[12, C] float32: two ordinary rows, a positive and a negative multiple of the first (an exact tie / c = -1, either may clip), a zero
    row, a row scaled by 1e-30, a NaN and an inf component, a row of one large component, the first row moved by one fp32 ulp, a constant
    row and its negation."""
    rng = np.random.default_rng(9000 + 31 * C + seed)
    v = rng.normal(size=(2, C)).astype(np.float32)
    nan, inf, big, ulp = v[1].copy(), v[1].copy(), 0.01 * v[1], v[0].copy()
    nan[C // 2], inf[0], big[C - 1] = np.nan, np.inf, 3.0e4
    ulp[C // 3] = np.nextafter(ulp[C // 3], np.float32(np.inf))
    one = np.full(C, 0.1, np.float32)
    return mc._f32(np.stack([v[0], v[1], 2.0 * v[0], -3.0 * v[0], np.zeros(C), v[0] * np.float32(1e-30), nan, inf, big, ulp, one, -one]))


# ------------------------------------------------------------------------------------------------ cosine near-ties
CN_N, CN_M = 80, 145            # two 64-row tiles, two 128-column slot tiles
CN_ROWS = 24


def _perp(rng, c, a):
    """A vector orthogonal to c and to a (in float64) of c's length: moving c along it changes cos(a, c) in the second order only."""
    p = rng.normal(size=c.shape)
    c64, a64 = c.astype(np.float64), a.astype(np.float64)
    a64 = a64 - (a64 @ c64) / (c64 @ c64) * c64
    p -= (p @ c64) / (c64 @ c64) * c64
    p -= (p @ a64) / (a64 @ a64) * a64
    return p * np.sqrt((c64 @ c64) / (p @ p))


def cos_near(rng, C, n=CN_N, m=CN_M):
    """Rows i < 24: columns 2 i and 2 i + 1 are a noisy copy c of a[i] and b' = c + eps perp in fp32, perp orthogonal to c and a[i], eps graded
    1e-4 .. 1e-6: the two cosines differ by ~1e-9 .. 1e-12 (eps^2 / 2 and the fp32 rounding of b'), which float64 tells apart and an fp32 filter cannot."""
    a = rng.normal(size=(n, C)).astype(np.float32)
    b = rng.normal(size=(m, C)).astype(np.float32)
    for i in range(CN_ROWS):
        c = (a[i] + mc.SIGMA * rng.normal(size=C)).astype(np.float32)
        eps = 10.0 ** (-4.0 - 2.0 * (i % 8) / 7.0)
        b[2 * i], b[2 * i + 1] = (c, (c + eps * _perp(rng, c, a[i])).astype(np.float32)) if i % 2 == 0 else ((c + eps * _perp(rng, c, a[i])).astype(np.float32), c)
    return a, b


def cos_multiples(rng, C, n=CN_N, m=CN_M):
    """Rows i < 24: columns 140 - 5 i and 3 i + 1 (two slot tiles for most) are c and a positive multiple of c: 2 c and c / 4 tie exactly (every sum
    scales by a power of two), 3 c and 1.7 c tie to the last bits.  The first index wins an exact tie."""
    a = rng.normal(size=(n, C)).astype(np.float32)
    b = rng.normal(size=(m, C)).astype(np.float32)
    for i in range(CN_ROWS):
        c = (a[i] + mc.SIGMA * rng.normal(size=C)).astype(np.float32)
        b[140 - 5 * i], b[3 * i + 1] = c, (np.float32((2.0, 0.25, 3.0, 1.7)[i % 4]) * c).astype(np.float32)
    return a, b


def cos_clip(rng, C, n=CN_N, m=CN_M):
    """Rows i < 24: a column that is a[i] itself, or a positive multiple of it (c = dot / (na nb) lands on 1 or an ulp either side of it: above,
    it is clipped and D = 0 exactly), next to the same for -a[i] (c = -1, D = 2: the farthest column) and a near copy that must not win."""
    a = rng.normal(size=(n, C)).astype(np.float32)
    b = rng.normal(size=(m, C)).astype(np.float32)
    for i in range(CN_ROWS):
        b[5 * i] = (np.float32((1.0, 3.0, 0.7, 1.1)[i % 4]) * a[i]).astype(np.float32)
        b[5 * i + 1] = -b[5 * i]
        b[5 * i + 2] = (a[i] + 1e-3 * rng.normal(size=C)).astype(np.float32)
    return a, b


def cos_zero_and_tiny(rng, C, n=CN_N, m=CN_M):
    """An ordinary pair of noisy copies with a zero row on either side (its whole row / column of D is NaN: numpy's argmin takes the first NaN) and
    a copy pair scaled by 1e-30 on either side (cosine does not see the scale; the squares, 1e-60, are far below fp32's range)."""
    a, b = mc.noisy_pair(rng, n, m, C)
    a[17], b[70] = 0.0, 0.0
    a[3], b[9] = a[3] * np.float32(1e-30), b[9] * np.float32(1e-30)
    return a, b


def cosine_near_tie_case(C=64):
    """8 pairs of 80 x 145: near-ties, multiples, clipping rows, a zero and a tiny row -- each twice, from two seeds."""
    makers = [cos_near, cos_multiples, cos_clip, cos_zero_and_tiny] * 2
    return mc._pack([f(np.random.default_rng(9100 + C + 13 * p), C) for p, f in enumerate(makers)], C, CN_N, CN_M)


# ------------------------------------------------------------------------------------------------ where the root merges what the sum keeps apart
ROOT_ROW, ROOT_COLS = 21, (40, 133)


def root_merge_pair(rng, C, n=CN_N, m=CN_M):
    """Row 21 is zero; column 40 is (1, 2^-26, 0, ..) and column 133 is (1, 0, ..): the sums are 1 + 2^-52 and 1, one ulp apart, and both
    roots are 1.  Euclidean takes the first index, 40; sqeuclidean the smaller sum, 133.  Every other column is ~C away."""
    a, b = mc.noisy_pair(rng, n, m, C)
    a[ROOT_ROW] = 0.0
    b[list(ROOT_COLS)] = 0.0
    b[ROOT_COLS[0], 0], b[ROOT_COLS[0], 1], b[ROOT_COLS[1], 0] = 1.0, 2.0 ** -26, 1.0
    return a, b


def root_merge_case(C=64):
    """8 pairs of 80 x 145, each with the row above (and noisy copies elsewhere)."""
    return mc._pack([root_merge_pair(np.random.default_rng(9300 + C + p), C) for p in range(8)], C, CN_N, CN_M)


def single_pair_case(C, n=70, m=135):
    """One pair of noisy copies with the special rows on both sides: the widths off the vector path (C % 4), the cosine tail (odd C) and the
    KC = 16 remainder."""
    rng = np.random.default_rng(9400 + C)
    a, b = mc.noisy_pair(rng, n, m, C)
    s = special_rows(C)
    a[40:40 + len(s)], b[100:100 + len(s)] = s, s[::-1]
    return mc._pack([(a, b)], C, n + 3, m + 4)
