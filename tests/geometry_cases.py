"""Inputs of the RANSAC edge tests (homography, fundamental matrix, essential matrix + recoverPose), built with numpy alone from fixed
seeds.  tests/test_oracle_geometry_edges.py checks on the CPU that every case has the property it is named for, with
oracle/geometry_ref.py alone; tests/test_gpu_geometry_edges.py hands the same arrays to csrc/geometry.hip through utils/mvg.py and
compares with the same oracle calls.  Cases and oracle results are cached: both files (and every test in them) share one instance.

A case is a dict: kind "H" / "F" / "E"; m0, m1 [n, 2] float32 NORMALISED rows, as the matcher hands them over; scale [4] float32 =
(sx0, sy0, sx1, sy1), normalised -> pixels; seed, the sampler seed; kw, the estimator's parameters where they are not the defaults
(the names of utils/mvg.py); for "E" also K0, K1 (float64 or float32 [3, 3]) and thresh; gt, what the scene was made from.
pixels(case) forms the fp32 products m * scale exactly as the kernels do: the oracle is fed those, never the scene's own float64
coordinates.

Group A ("parity"): the device must reproduce the oracle hypothesis for hypothesis.  Group B ("contract"): rank-deficient scenes on
which the minimal solver's answer is decided by rounding, and one case moved there from group A for a decision rounding makes (see
GROUP_B); only the kernel's contract is checked."""
import functools
import time

import numpy as np

from oracle import geometry_ref as g
from test_oracle_geometry import fscene, scene, synth

SC = np.array([639, 479, 639, 479], np.float32)            # both images 640 x 480
SC2 = np.array([639, 479, 719, 539], np.float32)           # image 0 640 x 480, image 1 720 x 540
SC_ONE = np.ones(4, np.float32)                            # rows already in pixels: the products are exact
K0 = np.array([[520, 0, 300.5], [0, 480, 250.25], [0, 0, 1.0]])
K1 = np.array([[610, 0, 339.0], [0, 590, 221.5], [0, 0, 1.0]])
KC = np.array([[500, 0, 319.5], [0, 500, 239.5], [0, 0, 1.0]])
TWOCAM_SEEDS = (61, 62, 63)
# three pairs, each with its own cameras and its own image sizes
VARIED = [(K0, K1, SC2),
          (np.array([[700, 0, 350.0], [0, 655, 262.5], [0, 0, 1.0]]), np.array([[455, 0, 255.5], [0, 505, 190.0], [0, 0, 1.0]]),
           np.array([799, 599, 511, 383], np.float32)),
          (np.array([[390, 0, 200.25], [0, 432, 149.5], [0, 0, 1.0]]), np.array([[560, 0, 320.0], [0, 530, 240.0], [0, 0, 1.0]]),
           np.array([399, 299, 639, 479], np.float32))]
POSE_BOUND = (6.0, 2.5)                                    # degrees (translation, rotation): test_gpu_geometry.py's own bound
ROUND_END_ITERS = (1, 255, 256, 257, 513)                  # a round is 256 hypotheses
H_FIX = np.array([[1.05, 0.04, 12.0], [-0.03, 0.97, 8.0], [2e-5, -1e-5, 1.0]])
M = {"H": 4, "F": 7, "E": 5}


def _case(kind, p0, p1, scale, seed, K0=None, K1=None, thresh=1.0, gt=None, **kw):
    scale = np.asarray(scale, np.float32)
    c = dict(kind=kind, m0=(np.asarray(p0) / scale[:2]).astype(np.float32), m1=(np.asarray(p1) / scale[2:]).astype(np.float32), scale=scale,
             seed=int(seed), kw=kw, gt=gt, n=len(p0))
    if kind == "E":
        c.update(K0=K0, K1=K1, thresh=thresh)
    return c


def _pix(x, K):
    """normalised image coordinates -> pixels of the camera K"""
    return x * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]


def _ecase(x1, x2, Ka, Kb, scale, seed, gt=None, dtype=np.float64, **kw):
    return _case("E", _pix(x1, Ka), _pix(x2, Kb), scale, seed, K0=Ka.astype(dtype), K1=Kb.astype(dtype), gt=gt, **kw)


def _twocam(seed, Ka, Kb, scale, dtype):
    x1, x2, R, t, inl = scene(300, 0.7, 0.3, seed)
    return _ecase(x1, x2, Ka, Kb, scale, seed, gt=(R, t, inl), dtype=dtype)


def _repeat(p0, p1):
    """180 of the 300 matches become copies of rows 200..204: what brute force without cross-check does to a textureless region."""
    rep = np.random.default_rng(1).integers(0, 5, 180)
    p0, p1 = p0.copy(), p1.copy()
    p0[:180], p1[:180] = p0[200 + rep], p1[200 + rep]
    return p0, p1


def _proj(H, p):
    q = np.c_[p, np.ones(len(p))] @ H.T
    return q[:, :2] / q[:, 2:]


def _collinear(off):
    """270 integer points on y = 2 x + 40 and `off` integer points off it, shuffled; dst = H_FIX(src).  SC_ONE: exact collinearity is the same
    fact in the kernel and in the oracle."""
    rng = np.random.default_rng(7)
    x = np.arange(270.0)
    extra = rng.integers(0, 600, (30, 2)).astype(np.float64)[:off]
    src = np.r_[np.c_[x, 2 * x + 40], extra][rng.permutation(270 + off)]
    return _case("H", src, _proj(H_FIX, src), SC_ONE, 70 + off, gt=H_FIX)


def _line(kind):
    src = np.stack([np.arange(40.0), 2 * np.arange(40.0) + 1], 1)
    return _case(kind, src, src + 5, SC_ONE, 3)


def _same(kind, n):
    return _case(kind, np.tile([[123.0, 77.0]], (n, 1)), np.tile([[140.0, 90.0]], (n, 1)), SC_ONE, n)


def _hard(kind, **kw):
    if kind == "H":
        src, dst, H, inl = synth(400, 0.12, 0.5, 12)
        return _case("H", src, dst, SC, 112, gt=(H, inl), **kw)
    if kind == "F":
        p1, p2, F, inl = fscene(400, 0.3, 0.5, 22)
        return _case("F", p1, p2, SC, 122, gt=(F, inl), **kw)
    x1, x2, R, t, inl = scene(400, 0.3, 0.5, 32)
    return _ecase(x1, x2, KC, KC, SC, 132, gt=(R, t, inl), **kw)


def _easy(kind, seed, **kw):
    if kind == "H":
        src, dst, H, inl = synth(300, 0.6, 0.4, seed)
        return _case("H", src, dst, SC, 1000 + seed, gt=(H, inl), **kw)
    if kind == "F":
        p1, p2, F, inl = fscene(300, 0.6, 0.4, seed)
        return _case("F", p1, p2, SC, 1000 + seed, gt=(F, inl), **kw)
    x1, x2, R, t, inl = scene(300, 0.6, 0.3, seed)
    return _ecase(x1, x2, KC, KC, SC, 1000 + seed, gt=(R, t, inl), **kw)


def _first_inliers(n):
    x1, x2, R, t, inl = scene(300, 0.7, 0.3, 31)
    i = np.flatnonzero(inl)[:n]
    return _ecase(x1[i], x2[i], KC, KC, SC, 31, gt=(R, t, inl[i]))


def _two_sizes(kind):
    if kind == "H":
        src, dst, H, inl = synth(300, 0.6, 0.5, 14)
        return _case("H", src, dst, SC2, 14, gt=(H, inl))
    p1, p2, F, inl = fscene(300, 0.6, 0.4, 24)
    return _case("F", p1, p2, SC2, 24, gt=(F, inl))


def _repeated(kind):
    if kind == "H":
        src, dst, H, inl = synth(300, 0.7, 0.5, 13)
        return _case("H", *_repeat(src, dst), SC, 13)
    if kind == "F":
        p1, p2, F, inl = fscene(300, 0.7, 0.4, 23)
        return _case("F", *_repeat(p1, p2), SC, 23)
    x1, x2, R, t, inl = scene(300, 0.7, 0.3, 33)
    return _ecase(*_repeat(x1, x2), KC, KC, SC, 33, gt=(R, t, inl))


def _identity():
    src = synth(200, 1.0, 0.0, 15)[0]
    return _case("H", src, src, SC, 15)


ROT_ANGLE = 0.1


def _group_b(name):
    if name == "b_still_f":
        p = fscene(100, 1.0, 0.0, 41)[0]
        return _case("F", p, p, SC, 41)
    if name == "b_still_e":
        x = scene(100, 1.0, 0.0, 42)[0]
        return _ecase(x, x, KC, KC, SC, 42)
    if name == "b_same_e":
        x1, x2 = scene(8, 1.0, 0.0, 43)[:2]
        return _ecase(np.tile(x1[:1], (20, 1)), np.tile(x2[:1], (20, 1)), KC, KC, SC, 43)
    if name in ("b_planar_f", "b_planar_e"):
        src, dst, H, inl = synth(300, 0.7, 0.3, 11)
        if name == "b_planar_f":
            return _case("F", src[inl], dst[inl], SC, 44)
        Ki = np.linalg.inv(KC)
        return _ecase(_proj(Ki, src[inl]), _proj(Ki, dst[inl]), KC, KC, SC, 45)
    assert name == "b_rot_e"
    x = scene(200, 1.0, 0.0, 35)[0]
    c, s = np.cos(ROT_ANGLE), np.sin(ROT_ANGLE)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    return _ecase(x, x @ Rz[:2, :2].T, KC, KC, SC, 46, gt=Rz)


RANK_DEFICIENT = ("b_still_f", "b_still_e", "b_same_e", "b_planar_f", "b_planar_e", "b_rot_e")
# easy_e_1 (one hypothesis on an easy essential-matrix scene) was built for group A.  Its single five-point sample has five of its ten roots
# within 0.12 of z = -8.85; 40 Aberth sweeps leave the one at -8.9003 with an imaginary part of 7.99e-6 against the realness bound 1e-6 (1 + |re|)
# = 9.90e-6, and moving the polynomial's constant coefficient by ONE ulp moves that root to -8.8955 + 2.8e-8 i: whether this candidate (8
# inliers, singular values 0.93 / 0.36 / 0.001, no essential matrix) is admitted is rounding's decision.  The oracle admits it and keeps it; the
# MI355X voids it and keeps the next candidate with 8 inliers, for which its R is the oracle's.  Contract only.
#
# e_n5 / e_n6 (the first five / six inliers of scene(300, 0.7, 0.3, 31)) were built for group A too.  Counts, masks and the hypothesis count agree
# exactly, R and t only to 5.1e-3: this sample is ill-conditioned for the five-point solver itself.  The oracle's own candidates have third singular
# values of 7.9e-5 and 2.0e-3 where a sound root gives 1e-11 (easy_e_1's clean candidates: 2e-12, 7e-12), and moving the oracle's INPUT by one ulp
# moves its own R, t by 7.6e-4 .. 2.9e-2 (eight trials; tests/test_oracle_geometry_edges.py asserts it).  The n == 5 branch still runs, with its
# exact figures (one hypothesis, n inliers, every row in the mask) asserted beside the contract.
GROUP_B = RANK_DEFICIENT + ("easy_e_1", "e_n5", "e_n6")
GIVE_UP = {"H": ("line_h", "same_h_50", "same_h_20", "same_h_12"), "F": ("line_f", "same_f_50", "same_f_20", "same_f_12")}

BUILDERS = {
    "h_two_sizes": lambda: _two_sizes("H"), "f_two_sizes": lambda: _two_sizes("F"),
    "rep_h": lambda: _repeated("H"), "rep_f": lambda: _repeated("F"), "rep_e": lambda: _repeated("E"),
    "col_h_30": lambda: _collinear(30), "col_h_28": lambda: _collinear(28), "col_h_3": lambda: _collinear(3),
    "line_h": lambda: _line("H"), "line_f": lambda: _line("F"),
    "ident_h": _identity,
    "thr_h": lambda: _easy("H", 17, threshold=0.5), "noref_h": lambda: _easy("H", 18, refine=False),
    "conf_h": lambda: _easy("H", 19, confidence=0.5), "conf_f": lambda: _easy("F", 29, confidence=0.5), "conf_e": lambda: _easy("E", 39, conf=0.5),
    "easy_h_1": lambda: _easy("H", 19, max_iters=1), "easy_f_1": lambda: _easy("F", 29, max_iters=1), "easy_e_1": lambda: _easy("E", 39, max_iters=1),
    "e_n5": lambda: _first_inliers(5), "e_n6": lambda: _first_inliers(6),
    # generic neighbours of a degenerate pair in one batch
    "gen_h_a": lambda: _easy("H", 16), "gen_h_b": lambda: _easy("H", 20), "gen_f_a": lambda: _easy("F", 26), "gen_f_b": lambda: _easy("F", 27),
    "gen_e_a": lambda: _easy("E", 36), "gen_e_b": lambda: _easy("E", 37),
}
for _n in (50, 20, 12):
    BUILDERS["same_h_%d" % _n] = functools.partial(_same, "H", _n)
    BUILDERS["same_f_%d" % _n] = functools.partial(_same, "F", _n)
for _s in TWOCAM_SEEDS:
    BUILDERS["twocam64_%d" % _s] = functools.partial(_twocam, _s, K0, K1, SC2, np.float64)
    BUILDERS["twocam32_%d" % _s] = functools.partial(_twocam, _s, K0, K1, SC2, np.float32)
for _i, (_s, (_a, _b, _sc)) in enumerate(zip(TWOCAM_SEEDS, VARIED)):
    BUILDERS["varied64_%d" % _i] = functools.partial(_twocam, _s, _a, _b, _sc, np.float64)
    BUILDERS["varied32_%d" % _i] = functools.partial(_twocam, _s, _a, _b, _sc, np.float32)
for _mi in ROUND_END_ITERS:
    for _k in "HFE":
        BUILDERS["ends_%s_%d" % (_k.lower(), _mi)] = functools.partial(_hard, _k, max_iters=_mi)
for _name in RANK_DEFICIENT:
    BUILDERS[_name] = functools.partial(_group_b, _name)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def pixels(c, swap_scale=False):
    """The fp32 pixel products the kernels form (MHA.py:41-42, AUC.py:125-126, FundamentalMatrix.py:76-77).  swap_scale: what a kernel that
    read sc[2..3] for image 0 and sc[0..1] for image 1 would form."""
    s0, s1 = (c["scale"][2:], c["scale"][:2]) if swap_scale else (c["scale"][:2], c["scale"][2:])
    return (c["m0"] * s0).astype(np.float32), (c["m1"] * s1).astype(np.float32)


def normalise(px, K):
    """AUC.py:47-48 as numpy evaluates it: float32 pixels and a float32 K stay float32, a float64 K promotes."""
    return (px - K[[0, 1], [2, 2]][None]) / K[[0, 1], [0, 1]][None]


def norm_thresh(c, Ka=None, Kb=None):
    """AUC.py:44-45 (f_mean as written there), in K's dtype"""
    Ka, Kb = (c["K0"], c["K1"]) if Ka is None else (Ka, Kb)
    return c["thresh"] / np.mean([Ka[0, 0], Kb[1, 1], Ka[0, 0], Kb[1, 1]])


def run_oracle(c, swap_scale=False):
    """oracle/geometry_ref.py on the case's fp32 pixel products: dict(found, model, mask, iters, inliers, seconds) and, for "E", the
    normalised points k0 / k1, the threshold thr and recoverPose's (good, R, t, mask_pose)."""
    p0, p1 = pixels(c, swap_scale)
    kw = dict(c["kw"])
    t0 = time.perf_counter()
    if c["kind"] == "H":
        model, mask, info = g.find_homography_ransac(p0.astype(np.float64), p1.astype(np.float64), seed=c["seed"], **kw)
        out = {}
    elif c["kind"] == "F":
        with np.errstate(all="ignore"):
            model, mask, info = g.find_fundamental_ransac(p0.astype(np.float64), p1.astype(np.float64), seed=c["seed"], **kw)
        out = {}
    else:
        k0, k1 = normalise(p0, c["K0"]), normalise(p1, c["K1"])
        thr = norm_thresh(c)
        with np.errstate(all="ignore"):
            model, mask, info = g.find_essential_ransac(k0, k1, seed=c["seed"], threshold=thr, prob=kw.get("conf", 0.99999),
                                                        max_iters=kw.get("max_iters", g.E_MAX_ITERS))
        out = dict(k0=np.asarray(k0, np.float64), k1=np.asarray(k1, np.float64), thr=float(thr), good=0, R=None, t=None, mask_pose=np.zeros_like(mask))
        if model is not None:
            with np.errstate(all="ignore"):
                out["good"], out["R"], out["t"], out["mask_pose"] = g.recover_pose(model, out["k0"], out["k1"], mask)
    out.update(found=int(model is not None), model=model, mask=mask, iters=info["iters"], inliers=info["inliers"], seconds=time.perf_counter() - t0)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, swap_scale=False):
    return run_oracle(case(name), swap_scale)


def errors(kind, model, o_or_pts):
    """The oracle's error of every match under `model`: reproj_err2 / fm_error on pixel pairs (p0, p1), sampson_err on normalised ones."""
    a, b = (np.asarray(v, np.float64) for v in o_or_pts)
    with np.errstate(all="ignore"):
        if kind == "H":
            return g.reproj_err2(model[None], a, b)[0]
        if kind == "F":
            return g.fm_error(model, a, b)
        return g.sampson_err(model, a, b)


def threshold2(c, o=None):
    """The squared threshold the inlier test compares with, in the type it is compared in."""
    if c["kind"] == "H":
        return c["kw"].get("threshold", g.H_THRESHOLD) ** 2
    if c["kind"] == "F":
        return np.float32(c["kw"].get("threshold", g.F_THRESHOLD) ** 2)
    return o["thr"] ** 2


def pose_error(c, R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = c["gt"][0], c["gt"][1]
    return g.compute_pose_error(T, R, t)


def pack(names, extra=13, kw=None):
    """The cases as ONE batch, the way the pipeline hands pairs over: m0 / m1 [B, K, 3] float32 (x, y, score) with K larger than every n
    and the rows beyond a pair's count NaN, counts [B] int32, seeds [B], scale [B, 4] and, for "E", K0 / K1 [B, 3, 3].  A launch has ONE set of
    estimator parameters: the cases' own, which must agree, or `kw` for all of them."""
    cs = [case(nm) for nm in names]
    assert len({c["kind"] for c in cs}) == 1 and (kw is not None or all(c["kw"] == cs[0]["kw"] for c in cs)), names
    B, K = len(cs), max(c["n"] for c in cs) + extra
    m0 = np.full((B, K, 3), np.nan, np.float32)
    m1 = np.full((B, K, 3), np.nan, np.float32)
    for b, c in enumerate(cs):
        m0[b, :c["n"], :2], m1[b, :c["n"], :2] = c["m0"], c["m1"]
        m0[b, :c["n"], 2] = m1[b, :c["n"], 2] = 0.5
    out = dict(m0=m0, m1=m1, k=np.array([c["n"] for c in cs], np.int32), seeds=np.array([c["seed"] for c in cs], np.int64),
               scale=np.stack([c["scale"] for c in cs]), kw=dict(cs[0]["kw"] if kw is None else kw), kind=cs[0]["kind"])
    if cs[0]["kind"] == "E":
        assert len({c["K0"].dtype for c in cs}) == 1 and len({c["thresh"] for c in cs}) == 1
        out.update(K0=np.stack([c["K0"] for c in cs]), K1=np.stack([c["K1"] for c in cs]), thresh=cs[0]["thresh"])
    return out


# ------------------------------------------------------------------------------------------------ the two rules the tests apply
def default_max_iters(c):
    return c["kw"].get("max_iters", {"H": g.H_MAX_ITERS, "F": g.F_MAX_ITERS, "E": g.E_MAX_ITERS}[c["kind"]])


def parity(c, o, got):
    """Group A.  `got`: found, inliers, iters, mask [n] and model ("H" / "F") or R, t, good ("E": mask is recoverPose's), from the device --
    or from another oracle run, which is how the CPU file shows that a wrong kernel would be noticed.  The bounds are those of
    tests/test_gpu_geometry.py.  Returns (figures, failures): a line of what was compared, and what missed its bound."""
    kind, n, bad = c["kind"], c["n"], []
    fig = "hypotheses %d / %d, inliers %d / %d" % (got["iters"], o["iters"], got["inliers"], o["inliers"])
    if got["mask"][n:].any():
        bad.append("mask set beyond the pair's %d rows" % n)
    if got["found"] != o["found"] or got["iters"] != o["iters"]:
        bad.append("found / hypotheses %d %d, oracle %d %d" % (got["found"], got["iters"], o["found"], o["iters"]))
    mask_e = o["mask_pose"] if kind == "E" else o["mask"]
    if not o["found"]:
        model = got["model"] if kind != "E" else np.r_[got["R"].ravel(), got["t"]]
        if got["inliers"] != 0 or np.any(model != 0) or got["mask"].any() or (kind == "E" and got["good"] != 0):
            bad.append("nothing found, yet inliers %d, model or mask not zero" % got["inliers"])
        return fig, bad
    if not got["found"]:
        return fig, bad
    slack = 0 if kind == "H" else 1
    if int(got["mask"][:n].sum()) != (got["good"] if kind == "E" else got["inliers"]):
        bad.append("mask sum %d is not the count returned" % got["mask"][:n].sum())
    if abs(got["inliers"] - o["inliers"]) > slack:
        bad.append("inliers %d, oracle %d" % (got["inliers"], o["inliers"]))
    if got["inliers"] == o["inliers"]:
        rows = int((got["mask"][:n] != mask_e).sum())
        fig += ", mask rows that differ %d" % rows
        if rows > (0 if kind == "H" else 2):
            bad.append("mask differs in %d rows" % rows)
        if kind == "E":
            d = max(np.abs(got["R"] - o["R"]).max(), np.abs(got["t"] - o["t"]).max())
            fig += ", max |R, t - oracle| %.3g, good %d / %d" % (d, got["good"], o["good"])
            if not d <= 1e-6 or abs(got["good"] - o["good"]) > 1:
                bad.append("R, t differ by %.3g, good %d / %d" % (d, got["good"], o["good"]))
        else:
            d, tol = np.abs(got["model"] - o["model"]).max(), (2e-7 if kind == "H" else 1e-6) * np.abs(o["model"]).max()
            fig += ", max |model - oracle| %.3g (bound %.3g)" % (d, tol)
            if not d <= tol:
                bad.append("model differs by %.3g > %.3g" % (d, tol))
    return fig, bad


def near_threshold(err, t2):
    """rows whose error is within a relative 1e-9 of the squared threshold: their side of it is rounding's to decide"""
    return np.abs(np.asarray(err, np.float64) - float(t2)) <= 1e-9 * float(t2)


def contract(c, o, got):
    """Group B: what the kernel promises whatever the scene.  `got` as in parity(), with model = F, or E beside R, t, good, mask_pose ("E":
    mask is the RANSAC mask here).  o: the oracle's run of the case (only its inputs k0, k1, thr are used).  Returns (figures, failures)."""
    kind, n, bad = c["kind"], c["n"], []
    fig = "found %d, hypotheses %d, inliers %d" % (got["found"], got["iters"], got["inliers"])
    if got["found"] not in (0, 1) or not 0 <= got["iters"] <= default_max_iters(c):
        bad.append("found %d, hypotheses %d" % (got["found"], got["iters"]))
    model = got["model"]
    if not got["found"]:
        zero = not np.any(model != 0) and not got["mask"].any() and got["inliers"] == 0
        if kind == "E":
            zero = zero and got["good"] == 0 and not np.any(got["R"] != 0) and not np.any(got["t"] != 0) and not got["mask_pose"].any()
        if not zero:
            bad.append("nothing found, yet model, mask, inliers or good not zero")
        return fig, bad
    if not np.isfinite(model).all():
        bad.append("model not finite")
        return fig, bad
    if got["mask"][n:].any() or int(got["mask"][:n].sum()) != got["inliers"] or got["inliers"] < M[kind]:
        bad.append("mask sum %d, beyond n %d, inliers %d" % (got["mask"][:n].sum(), got["mask"][n:].sum(), got["inliers"]))
    pts = (o["k0"], o["k1"]) if kind == "E" else pixels(c)
    t2 = threshold2(c, o)
    err = errors(kind, model, pts)
    clear = ~near_threshold(err, t2)
    wrong = int((got["mask"][:n][clear] != (err <= t2)[clear]).sum())
    fig += ", rows near the threshold %d, mask rows the model's errors do not reproduce %d" % (int((~clear).sum()), wrong)
    if wrong:
        bad.append("%d mask rows are not what the returned model's errors give" % wrong)
    if kind == "E":
        R = got["R"]
        d = max(abs(np.linalg.det(R) - 1), np.abs(R @ R.T - np.eye(3)).max())
        fig += ", |det R - 1|, |R R^T - I| <= %.3g, good %d" % (d, got["good"])
        if not d <= 1e-9:
            bad.append("R is no rotation: %.3g" % d)
        if got["mask_pose"][n:].any() or int(got["mask_pose"][:n].sum()) != got["good"] or (got["mask_pose"][:n] > got["mask"][:n]).any():
            bad.append("recoverPose's mask: sum %d, good %d, or a row outside the RANSAC mask" % (got["mask_pose"][:n].sum(), got["good"]))
    return fig, bad


def as_got(o, ransac_mask=False):
    """An oracle run in the shape parity() takes, or (ransac_mask) contract()"""
    got = dict(found=o["found"], inliers=o["inliers"], iters=o["iters"], mask=o["mask"] if ransac_mask or "R" not in o else o["mask_pose"])
    z = lambda *s: np.zeros(s)
    if "R" in o:
        got.update(model=o["model"] if o["found"] else z(3, 3), R=o["R"] if o["found"] else z(3, 3), t=o["t"] if o["found"] else z(3), good=o["good"],
                   mask_pose=o["mask_pose"])
    else:
        got.update(model=o["model"] if o["found"] else z(3, 3))
    return got
