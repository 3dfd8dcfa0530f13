"""Sub-pixel refinement of the rows kpb_detect keeps (KPB_OPT_DETECT_REFINE): the numpy restatement of the definition, the maps and
the case list the CPU and GPU tests share (tests/test_detect_refine_cpu.py, tests/test_gpu_detect_refine.py).

refine_np is the definition itself, vectorised over the rows: every numpy operation on float32 arrays is one IEEE operation rounded to fp32 on its own, which
is what the device does with the __f*_rn intrinsics.  Mode 1 (quadratic) is therefore bit-exact against the device.  Mode 2 (soft-argmax) is not: its weights
are exp() values.  Here the weight is the CORRECTLY ROUNDED fp32 exponential (evaluated in float64, rounded once), the device's is expf, within an ulp of it.
With dtype=np.float64 the same steps run in float64 on the same fp32 map and the same fp32 temperature: the yardstick mode 2 is compared against.
"""
import numpy as np

from keypoint_bench_amd import synthetic

RADIUS = 2
TEMP = np.float32(0.1)


def bumps(H, W, centres, sigma, amp):
    """s[r][c] = amp exp(-((c + 0.5 - u)^2 + (r + 0.5 - v)^2) / (2 sigma^2)), summed over the centres (u, v) in pixels; float64, rounded once to fp32."""
    y, x = np.mgrid[0:H, 0:W]
    s = np.zeros((H, W), np.float64)
    for u, v in centres:
        s += amp * np.exp(-((x + 0.5 - u) ** 2 + (y + 0.5 - v) ** 2) / (2.0 * sigma * sigma))
    return s.astype(np.float32)


def _parabola(a, m, e, edge, f):
    a, m, e = a.astype(f), m.astype(f), e.astype(f)
    den = (a - m) + (e - m)
    d = (a - e) / (den + den)
    d = np.where(np.isnan(d), f(0), d)
    d = np.minimum(np.maximum(d, f(-0.5)), f(0.5))
    return np.where(edge | ~(den < 0), f(0), d).astype(f)


def refine_offsets(score, idx, H, W, mode, dtype=np.float32):
    """(dx, dy) in pixels of the rows at flat indices idx of ONE [H, W] fp32 map; mode 1 = quadratic, 2 = softargmax."""
    f = dtype
    s = np.ascontiguousarray(score, dtype=np.float32).reshape(H, W)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    r, c = idx // W, idx % W
    with np.errstate(all="ignore"):
        if mode == 1:
            m = s[r, c]
            dx = _parabola(s[r, np.maximum(c - 1, 0)], m, s[r, np.minimum(c + 1, W - 1)], (c == 0) | (c == W - 1), f)
            dy = _parabola(s[np.maximum(r - 1, 0), c], m, s[np.minimum(r + 1, H - 1), c], (r == 0) | (r == H - 1), f)
            return dx, dy
        assert mode == 2
        taps, mx = [], np.full(idx.shape, -np.inf, f)
        for oy in range(-RADIUS, RADIUS + 1):           # row-major, ascending
            for ox in range(-RADIUS, RADIUS + 1):
                rr, cc = r + oy, c + ox
                inside = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
                v = np.where(inside, s[np.clip(rr, 0, H - 1), np.clip(cc, 0, W - 1)], np.float32(np.nan)).astype(f)    # out of the map: no weight, never the maximum
                mx = np.where(v > mx, v, mx)
                taps.append((ox, oy, v))
        sw, sx, sy = np.zeros(idx.shape, f), np.zeros(idx.shape, f), np.zeros(idx.shape, f)
        for ox, oy, v in taps:
            t = (v - mx) / f(TEMP)
            w = np.where(np.isnan(t), f(0), np.exp(t.astype(np.float64)).astype(f))
            sw = sw + w
            sx = sx + w * f(ox)
            sy = sy + w * f(oy)
        out = []
        for num in (sx, sy):
            d = num / sw
            d = np.where(np.isnan(d), f(0), d)
            out.append(np.minimum(np.maximum(d, f(-RADIUS)), f(RADIUS)).astype(f))
        return out[0], out[1]


def refine_np(score, idx, H, W, mode, dtype=np.float32):
    """[n, 2] (x, y) of the refined rows, normalised as kpb_detect returns them: x = ((col + 0.5) + dx) / W, y = ((row + 0.5) + dy) / H; mode 0: the pixel centres."""
    f = dtype
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    r, c = idx // W, idx % W
    if mode == 0:
        dx = dy = np.zeros(idx.shape, f)
    else:
        dx, dy = refine_offsets(score, idx, H, W, mode, f)
    x = ((c.astype(f) + f(0.5)) + dx) / f(W)
    y = ((r.astype(f) + f(0.5)) + dy) / f(H)
    return np.stack([x, y], axis=1).astype(f)


def pixels(xy, H, W):
    """Normalised (x, y) rows in pixels, float64."""
    return np.asarray(xy, dtype=np.float64) * np.array([W, H], np.float64)


# ------------------------------------------------------------------------------------------------ the bumps of the 0.25 condition
BUMP_SHAPE = (64, 96)
BUMP_SIGMA, BUMP_AMP, BUMP_PITCH = 1.5, 1.0, 13


def bump_centres(seed=7):
    """One bump per 13-pixel cell of a 64 x 96 map (24 bumps, centres >= 11 px from every edge and >= 12 px apart), each offset from the centre of its pixel by
    0.1 .. 0.5 px in the larger coordinate; returns (centres [n, 2] = (u, v), flat index of each bump's pixel)."""
    H, W = BUMP_SHAPE
    rng = np.random.default_rng(seed)
    cen, idx = [], []
    for pr in range(11, H - 11, BUMP_PITCH):
        for pc in range(11, W - 11, BUMP_PITCH):
            o = rng.uniform(-0.5, 0.5, 2)
            o *= rng.uniform(0.1, 0.5) / np.abs(o).max()
            cen.append((pc + 0.5 + o[0], pr + 0.5 + o[1]))
            idx.append(pr * W + pc)
    return np.array(cen, np.float64), np.array(idx, np.int64)


def bump_map(seed=7):
    H, W = BUMP_SHAPE
    return bumps(H, W, bump_centres(seed)[0], BUMP_SIGMA, BUMP_AMP)


def bump_ratios(xy, idx, seed=7):
    """Per bump: |refined position - centre| / |pixel centre - centre|, rows xy normalised, idx their pixels (any order, every bump once)."""
    H, W = BUMP_SHAPE
    cen, cidx = bump_centres(seed)
    order = {int(i): k for k, i in enumerate(cidx)}
    assert sorted(int(i) for i in idx) == sorted(order), "the rows are not the bumps' pixels"
    k = np.array([order[int(i)] for i in idx])
    idx = np.asarray(idx, np.int64)
    centre = np.stack([idx % W + 0.5, idx // W + 0.5], axis=1)
    e1 = np.hypot(*(pixels(xy, H, W) - cen[k]).T)
    e0 = np.hypot(*(centre - cen[k]).T)
    return e1 / e0


# ------------------------------------------------------------------------------------------------ the GPU cases
def special_map():
    """12 x 20, finite pixels uniform in (0.1, 1) but for: a NaN, a +inf, and a two-pixel plateau above everything finite around it.  Detected with nms_dist 0
    (the NMS kernels are not pinned on NaN maps): every finite pixel is a row, so rows beside the NaN, beside and on the inf, and on the plateau all occur."""
    s = (0.1 + 0.9 * synthetic.score_uniform(31, 12, 20)).astype(np.float32)
    s[3, 4] = np.nan
    s[7, 11] = np.inf
    s[5, 15] = s[5, 16] = np.float32(2.0)
    s[0, 0] = np.nan            # a corner: the window of (1, 1) holds it
    return s


def _mixed(seed, B, H, W):
    return np.stack([(synthetic.score_smooth if b % 2 else synthetic.score_uniform)(seed + b, H, W) for b in range(B)])


def _signed(B, H, W):
    return np.stack([(synthetic.score_smooth(60 + b, H, W) - np.float32(0.5)).astype(np.float32) if b % 2 else
                     np.random.default_rng(60 + b).uniform(-0.8, 0.2, (H, W)).astype(np.float32) for b in range(B)])


def _prm(nms_dist, border, top_k, threshold=0.0):
    return dict(nms_dist=nms_dist, threshold=threshold, border_dist=border, top_k=top_k, min_score=0.0)


# name -> (maps [B, H, W] builder, extractor_params, signed, environment the call needs)
CASES = {
    "raster_edges": (lambda: _mixed(40, 1, 32, 32), _prm(2, 0, 32 * 32), False, {}),                    # top_k >= N: raster order, keypoints on the map's edge
    "sorted": (lambda: _mixed(41, 5, 40, 56), _prm(4, 8, 16), False, {}),                               # top_k < N: the sorted path
    "select_scan": (lambda: _mixed(46, 2, 136, 136), _prm(6, 0, 300), False, {}),                       # two 16 384-pixel chunks, batch < 64
    "bitmap": (lambda: _mixed(100, 64, 32, 48), _prm(2, 0, 32 * 48), False, {"KPB_NMS_TILED": "0"}),    # select_topk's bitmap form (threshold 0, 64 images, the tail)
    "signed": (lambda: _signed(2, 64, 96), _prm(3, 4, 200), True, {}),
    "nms0": (lambda: _mixed(48, 1, 16, 24), _prm(0, 0, 16 * 24), False, {}),                            # the centre need not be a maximum
    "special": (lambda: special_map()[None], _prm(0, 0, 12 * 20), False, {}),
}

_MAPS = {}


def case(name):
    """(maps, params, signed, env) of a case; the maps are built once, shared, never written to."""
    build, prm, signed, env = CASES[name]
    if name not in _MAPS:
        m = build()
        m.setflags(write=False)
        _MAPS[name] = m
    return _MAPS[name], dict(prm), signed, env


def kept_rows_cpu(name):
    """Per image of a case, the flat indices of the rows the detection keeps, found on the CPU: the oracle's detection, or -- the NaN map, at nms_dist 0 --
    the pixels above the threshold."""
    import oracle
    maps, prm, _, _ = case(name)
    if name == "special":
        return [np.flatnonzero(maps[0].reshape(-1) > prm["threshold"])]
    return [oracle.detection(m, prm)[1] for m in maps]


def soft_deviation_px(name):
    """Worst |float32 restatement - float64 restatement| of mode 2 over the kept rows of a case, in pixels."""
    maps, _, _, _ = case(name)
    H, W = maps.shape[1:]
    worst = 0.0
    for m, idx in zip(maps, kept_rows_cpu(name)):
        if len(idx):
            d = pixels(refine_np(m, idx, H, W, 2, np.float32), H, W) - pixels(refine_np(m, idx, H, W, 2, np.float64), H, W)
            worst = max(worst, float(np.abs(d).max()))
    return worst


# Mode 2's tolerance.  SOFT_WORST_PX: the worst soft_deviation_px over CASES and the bump map's rows, measured on the CPU (tests/test_detect_refine_cpu.py asserts it
# still covers what it measures); it is the rounding of the coordinate itself -- (col + 0.5) + dx at col >= 128 has an fp32 spacing of 1.5e-5 px, and the
# division by W rounds once more -- not the weights.  SOFT_TOL_PX = 4 x that: the device's expf and the restatement's are each within an ulp of the true value
# and are summed in the same order, which moves dx by parts in 1e7 -- at most one more rounding step of the coordinate, with room.  Nothing here is measured
# against the device.
SOFT_WORST_PX = 1.1e-5         # measured 1.0977e-05 ("select_scan", the widest maps), rounded up to two digits
SOFT_TOL_PX = 4 * SOFT_WORST_PX
