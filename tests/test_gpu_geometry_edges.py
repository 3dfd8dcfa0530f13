"""The three RANSAC kernels of csrc/geometry.hip and kpb_recover_pose on the inputs of tests/geometry_cases.py: two different cameras and
image sizes, repeated and collinear matches, input on which the sampler gives up, loops ended at, before and after a 256-hypothesis round,
the essential matrix at exactly 5 matches, and rank-deficient scenes.  tests/test_oracle_geometry_edges.py shows on the CPU that each
case has the property it is named for and that the rules applied here (geometry_cases.parity / contract) notice a swapped camera, a
swapped scale half or another kept model.

Every launch goes the way tests/test_gpu_geometry.py's do: the oracle is fed the fp32 pixel products the kernel forms, every pair has
its own sampler seed, k_dev counts with K = (largest n) + 13 rows per pair, and the rows beyond a pair's count are NaN in m0 and m1.

Group A (parity with oracle/geometry_ref.py; the bounds of tests/test_gpu_geometry.py): found and the hypothesis count info[2] exact;
homography: inlier count and mask exact, H within 2e-7 max|He|; fundamental / essential: inlier count within 1 and, when equal, the
mask off in at most 2 rows, F within 1e-6 max|Fe|, R and t within 1e-6 (recoverPose's count within 1).  Nothing found: model, mask and
counts zero.  Group B (geometry_cases.GROUP_B: no motion, 20 copies of one match, a planar scene, pure rotation): the minimal solver's
answer is rounding's to decide there, so only the contract is asserted (geometry_cases.contract): the call returns, found is 0 or 1 with
info[2] <= max_iters; nothing found: everything zero; found: a finite model, mask[n:] zero, mask[:n].sum() == info[1] >= M, the mask is
what the oracle's error function gives for the RETURNED model (rows within a relative 1e-9 of the squared threshold exempt), R a
rotation to 1e-9; and a generic pair before and after it in the batch is bit for bit its solo run.  The essential matrix and the RANSAC
mask, which utils/mvg.estimate_pose does not hand out, are fetched for group B by the same two ABI calls made here (_essential_raw).

Why every case terminates (read from csrc/geometry.hip before the first run):
  * gen_round (thread 0) makes 256 subsets per round; a subset costs at most GETSUBSET_ATTEMPTS = 10 000 whole redraws (1 000 in the
    least-median branch: the registrator rule's ATTEMPTS), after which `alive` turns false and the rest of the round, and every later round, draws nothing.  An index
    is redrawn `do .. while (dup)` until it differs from the i < M earlier ones: every case has n >= M (asserted on the CPU), so at least
    n - M + 1 of the n residues end the loop, and the draws are cv::RNG's integer stream -- the one the oracle consumes and returns from.
    Worst case here: all 10 000 attempts of the first subset (40 collinear points, 12 / 20 / 50 copies of one point), about 10 000 x (7 draws
    + 30 collinearity tests) operations of one lane: milliseconds.
  * the round loop (search for the essential and the fundamental matrix and its least-median branch, ransac_homography's own copy of it)
    advances base by 256 and goes on only while base < niters; niters starts at max_iters and RANSACUpdateNumIters never
    raises it (it returns at most the value it was given): at most ceil(max_iters / 256) rounds, 8 for the homography (2 000), 4 for the
    other two (1 000), 2 in the least-median branch (300).  scan_round stops earlier at it >= niters or at the first dead subset.
  * a hypothesis is straight-line code: Gauss-Jordan on fixed sizes, 40 Aberth sweeps and 3 Newton steps, a closed-form cubic; the refit
    is at most 10 x 6 Levenberg-Marquardt solves and recoverPose at most 30 Jacobi sweeps.  Every __syncthreads() sits on a branch taken
    from n, a kernel argument or a value thread 0 left in LDS before the preceding barrier: the same for all 256 threads.  The shared
    helpers keep to it: load_matches ends in its barrier with no return before it, search leaves its loop on ctl, read between two barriers,
    and returns the same `have` to every thread, and the kernels' early returns (n < M, nothing kept) follow from n and that value.
  * memory: points are read for i < n <= K only (the NaN rows never), s_idx holds indices < n, mask is written for i < K, the dynamic LDS is
    16 or 32 bytes x K <= 13 KB.

Figures (every test prints what it compares before it asserts; pytest -s).  Oracle, on the CPU: the two-camera scenes end after
130 / 93 / 123 hypotheses with 183 / 195 / 195 inliers and pose errors (0.77, 0.36) (1.97, 1.14) (0.81, 0.57) degrees; repeated matches
5 / 31 / 113 hypotheses, 268 / 226 / 188 inliers (H / F / E); mostly collinear 2 / 1 / 33 hypotheses after 35 / 11 / 3 938 redrawn subsets with
30 / 28 / 3 points off the line; every round-end case runs exactly max_iters hypotheses; confidence 0.5 stops after 4 / 151 / 27; n = 5 and 6:
one hypothesis; the oracle's R misses the pure rotation by 6.9e-5 degrees.

Measured on an MI355X (41 tests, 6.6 s in all, the slowest 0.9 s).  Every group A case: found, hypothesis count, inlier count and every mask row
equal to the oracle's.  Largest model differences: H 5.1e-9 (bound 4.4e-7; 5.8e-15 on the identity, 2.2e-16 with refine = False), F 0 in every
case, R, t 8.6e-8 on the repeated matches and 3.1e-10 elsewhere (bound 1e-6).  The two-camera poses are the oracle's to 7.5e-11 (float64
intrinsics) and 3.1e-10 (float32), pose errors as above, |det R - 1| <= 5.6e-16.  The give-up cases return zeros with info = (0, 0, 0, branch).
A pair's neighbours in a batch: bit-equal to their solo runs in all eleven batches.  Group B: every rank-deficient scene came out as the oracle's
run does (no motion and 20 copies: nothing in 1 000 hypotheses; planar F 1 hypothesis, 210 inliers; planar E 7 hypotheses, 209 inliers; rotation 1
hypothesis, 200 inliers, R off by 6.86e-5 degrees, the oracle's own figure), no row near a threshold, no mask row the returned model does not
reproduce, |R R^T - I| <= 6.7e-16.

Moved from group A to group B after the first run (the reasons, with their figures, stand at geometry_cases.GROUP_B):
  * easy_e_1 (max_iters = 1 on an easy essential-matrix scene): the oracle keeps candidate 4 of the one sample, admitted by an unconverged root
    whose imaginary part is at 0.81 of the realness bound; the device voids it and keeps candidate 8, equal to the oracle's candidate 8 to 1.3e-9.
    Both have 8 inliers.  The hard scene's max_iters = 1 case (ends_e_1) stays in group A and agrees.
  * e_n5, e_n6: counts, masks and recoverPose's count agree; R, t differ from the oracle's by 5.06e-3 on a sample where one ulp on the input moves the
    oracle's own answer by 7.6e-4 .. 2.9e-2.
With K0 / K1 swapped in utils/mvg.estimate_pose and sc[0] / sc[2] swapped in ransac_fundamental (the scaling has since moved to load_matches,
which it shares with ransac_essential), test_two_cameras (both) and
test_two_image_sizes_homography_and_fundamental fail; with `it > st.niters` in scan_round, 28 of the 41 tests fail, every test_round_ends case but 256 among them.
"""
import ctypes

import numpy as np
import pytest
import torch

import geometry_cases as gc
from oracle import geometry_ref as g

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _essential_raw(p, kw):
    """kpb_find_essential + kpb_recover_pose as utils/mvg.estimate_pose calls them (float64 intrinsics), keeping E and the RANSAC mask."""
    from keypoint_bench_amd._lib import Context, ptr
    a, b = _t(p["m0"]), _t(p["m1"])
    B, K = a.shape[0], a.shape[1]
    k0, k1 = p["K0"].astype(np.float64), p["K1"].astype(np.float64)
    cam = np.stack([k0[:, 0, 2], k0[:, 1, 2], k0[:, 0, 0], k0[:, 1, 1], k1[:, 0, 2], k1[:, 1, 2], k1[:, 0, 0], k1[:, 1, 1]], 1)
    thr = p["thresh"] / np.mean(np.stack([k0[:, 0, 0], k1[:, 1, 1], k0[:, 0, 0], k1[:, 1, 1]], 1), axis=1)
    sd = _t((p["seeds"] & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
    sc, cam_d, thr_d, kk = _t(p["scale"]), _t(cam), _t(thr), _t(p["k"])
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    E, mask, mask2, info = z((B, 9), torch.float64), z((B, K), torch.uint8), z((B, K), torch.uint8), z((B, 4), torch.int32)
    pts, rt, good = z((B, K, 4), torch.float64), z((B, 12), torch.float64), z((B,), torch.int32)
    ctx = Context.get(torch.device(DEV))
    ctx.check(ctx.lib.kpb_find_essential(ctx.handle, ptr(a), 3, ptr(b), 3, B, K, ptr(kk), ptr(sc), ptr(cam_d), 0, ptr(thr_d), ptr(sd), ctypes.c_uint32(0),
                                         float(kw.get("conf", 0.99999)), int(kw.get("max_iters", 1000)), ptr(E), ptr(mask), ptr(info), ptr(pts)))
    ctx.check(ctx.lib.kpb_recover_pose(ctx.handle, ptr(E), ptr(pts), ptr(mask), B, K, ptr(kk), ptr(info), 1e9, ptr(rt), ptr(mask2), ptr(good)))
    return E.reshape(B, 3, 3), mask, rt, mask2, good, info


def device(names, shared_scale=False, raw=False, kw=None):
    """One launch (two for "E") of the named cases as a batch -> one `got` dict per pair, numpy (geometry_cases.parity / contract).
    kw: the launch's estimator parameters where they are not the cases' own (a generic pair beside one with max_iters = 1)."""
    from keypoint_bench_amd.utils.mvg import estimate_pose, find_fundamental, find_homography
    p = gc.pack(names, kw=kw)
    kind, kw = p["kind"], p["kw"]
    scale = p["scale"][0] if shared_scale else p["scale"]          # [4] for the whole batch, or [B, 4]
    assert not shared_scale or (p["scale"] == p["scale"][0]).all()
    n = lambda v: v.cpu().numpy()
    if kind in "HF":
        fn = find_homography if kind == "H" else find_fundamental
        model, mask, info = fn(_t(p["m0"]), _t(p["m1"]), scale, k_dev=_t(p["k"]), seeds=p["seeds"], **kw)
        model, mask, info = n(model), n(mask), n(info)
        return [dict(found=int(info[b, 0]), inliers=int(info[b, 1]), iters=int(info[b, 2]), model=model[b], mask=mask[b], info=info[b]) for b in range(len(names))]
    if raw:
        E, mask, rt, mask2, good, info = (n(v) for v in _essential_raw(p, kw))
        return [dict(found=int(info[b, 0]), inliers=int(info[b, 1]), iters=int(info[b, 2]), model=E[b], mask=mask[b], mask_pose=mask2[b], R=rt[b, :9].reshape(3, 3),
                     t=rt[b, 9:], good=int(good[b]), info=info[b]) for b in range(len(names))]
    K0, K1 = (p["K0"][0], p["K1"][0]) if shared_scale else (p["K0"], p["K1"])
    rt, mask, good, info = (n(v) for v in estimate_pose(_t(p["m0"]), _t(p["m1"]), scale, K0, K1, thresh=p["thresh"], k_dev=_t(p["k"]), seeds=p["seeds"], **kw))
    return [dict(found=int(info[b, 0]), inliers=int(info[b, 1]), iters=int(info[b, 2]), mask=mask[b], R=rt[b, :9].reshape(3, 3), t=rt[b, 9:], good=int(good[b]),
                 info=info[b]) for b in range(len(names))]


def check_parity(names, gots):
    """Prints every pair's figures, then asserts that none missed a bound."""
    failures = []
    for name, got in zip(names, gots):
        fig, bad = gc.parity(gc.case(name), gc.oracle(name), got)
        print("%s: %s%s" % (name, fig, "  MISSED: %s" % bad if bad else ""))
        failures += [(name, b) for b in bad]
    assert not failures, failures


def same_bits(a, b, n):
    """two runs of one pair: every output bit for bit (masks over the pair's own rows; the padding is checked by parity / contract)"""
    keys = [k for k in ("model", "R", "t", "info") if k in a]
    return all(np.array_equal(a[k], b[k]) for k in keys) and np.array_equal(a["mask"][:n], b["mask"][:n]) and a.get("good") == b.get("good") and \
        ("mask_pose" not in a or np.array_equal(a["mask_pose"][:n], b["mask_pose"][:n]))


def between_neighbours(name, raw=False):
    """The pair between two generic ones in a batch.  The neighbours must come out bit for bit as in their solo runs with the same seeds."""
    k, kw = gc.case(name)["kind"].lower(), gc.case(name)["kw"]
    nb = ["gen_%s_a" % k, "gen_%s_b" % k]
    batch = device([nb[0], name, nb[1]], raw=raw, kw=kw)
    for i, j in ((0, 0), (1, 2)):
        solo = device([nb[i]], raw=raw, kw=kw)[0]
        ok = same_bits(solo, batch[j], gc.case(nb[i])["n"])
        print("%s beside %s: solo and batched runs %s (found %d, hypotheses %d, inliers %d)" % (nb[i], name, "equal" if ok else "DIFFER", solo["found"],
                                                                                                  solo["iters"], solo["inliers"]))
        assert ok and (solo["found"] == 1 or kw)
    return batch[1]


# ------------------------------------------------------------------------------------------------ group A
@pytest.mark.parametrize("bits", [64, 32])
def test_two_cameras(bits):
    """K0 != K1, fx != fy, 640 x 480 against 720 x 540: cam[0..3] / cam[4..7] and sc[0..1] / sc[2..3] each read for their own image.  32: float32
    intrinsics, the cam_f32 branch (numpy normalises in float32 there, as AUC.py does with MegaDepth's K)."""
    names = ["twocam%d_%d" % (bits, s) for s in gc.TWOCAM_SEEDS]
    varied = ["varied%d_%d" % (bits, i) for i in range(3)]
    runs = [(names, device(names, shared_scale=True)), (names[1:2], device(names[1:2])), (varied, device(varied))]      # [4], [1, 4], [3, 4] scales
    failures = []
    for nms, gots in runs:
        for name, got in zip(nms, gots):
            et, eR = gc.pose_error(gc.case(name), got["R"], got["t"])
            detR = abs(np.linalg.det(got["R"]) - 1)
            print("%s (batch of %d): pose error (%.2f, %.2f) degrees, |det R - 1| %.2g" % (name, len(nms), et, eR, detR))
            if not (et < gc.POSE_BOUND[0] and eR < gc.POSE_BOUND[1] and detR < 1e-9):
                failures.append((name, et, eR, detR))
    for nms, gots in runs:
        check_parity(nms, gots)
    assert not failures, failures


def test_two_image_sizes_homography_and_fundamental():
    for name in ("h_two_sizes", "f_two_sizes"):
        check_parity([name], device([name]))


@pytest.mark.parametrize("name", ["rep_h", "rep_f", "rep_e"])
def test_repeated_matches(name):
    check_parity([name], device([name]))


def test_mostly_collinear_homography():
    names = ["col_h_30", "col_h_28", "col_h_3"]
    gots = device(names)
    check_parity(names, gots)
    for name, got in zip(names, gots):
        assert got["inliers"] == gc.case(name)["n"] and np.abs(got["model"] - gc.H_FIX).max() < 1e-4 * np.abs(gc.H_FIX).max()


@pytest.mark.parametrize("kind", ["H", "F"])
def test_sampler_gives_up(kind):
    names = list(gc.GIVE_UP[kind])
    gots = device(names)
    check_parity(names, gots)
    for name, got in zip(names, gots):
        assert got["found"] == 0 and got["inliers"] == 0 and got["iters"] == 0 and not got["model"].any() and not got["mask"].any(), name
        assert got["info"][3] == (1 if name == "same_f_12" else 0)             # the least-median branch gives up too
    got = between_neighbours(names[0])
    check_parity(names[:1], [got])


def test_identity():
    got = device(["ident_h"])[0]
    check_parity(["ident_h"], [got])
    d = np.abs(got["model"] - np.eye(3)).max()
    print("ident_h: max |H - I| %.3g" % d)
    assert got["iters"] == 1 and got["inliers"] == gc.case("ident_h")["n"] and d <= 2e-7


@pytest.mark.parametrize("kind", "hfe")
@pytest.mark.parametrize("max_iters", gc.ROUND_END_ITERS)
def test_round_ends(kind, max_iters):
    """max_iters ends the loop inside a round, at its last hypothesis, and at the first of the next: info[2] is exactly max_iters and the
    kept model the oracle's (`it >= st.niters` in scan_round)."""
    name = "ends_%s_%d" % (kind, max_iters)
    got = device([name])[0]
    check_parity([name], [got])
    assert got["iters"] == max_iters == gc.oracle(name)["iters"]


@pytest.mark.parametrize("name", ["easy_h_1", "easy_f_1", "conf_h", "conf_f", "conf_e", "thr_h", "noref_h"])
def test_early_stops_and_parameters(name):
    """max_iters = 1 on an easy scene (the essential-matrix one is in group B: geometry_cases.GROUP_B says why), confidence 0.5 (the loop ends
    early and inside the first round), threshold 0.5, refine = False (H is the kept hypothesis itself, as the oracle's refine=False returns it)."""
    got = device([name])[0]
    check_parity([name], [got])
    if name == "noref_h":
        err = np.sort(gc.errors("H", got["model"], gc.pixels(gc.case(name))))
        print("noref_h: the four smallest squared errors of the returned H: %s" % err[:4])
        assert (err[:4] < 1e-12).all()


# ------------------------------------------------------------------------------------------------ group B
@pytest.mark.parametrize("name", gc.GROUP_B)
def test_group_b_keeps_the_contract(name):
    """The rank-deficient scenes, and easy_e_1, whose one hypothesis has a candidate that rounding admits or voids (geometry_cases.GROUP_B)."""
    c, o = gc.case(name), gc.oracle(name)
    got = between_neighbours(name, raw=True)
    fig, bad = gc.contract(c, o, got)
    print("%s: %s (oracle: found %d, hypotheses %d, inliers %d)%s" % (name, fig, o["found"], o["iters"], o["inliers"], "  MISSED: %s" % bad if bad else ""))
    solo = device([name], raw=True)[0]
    assert same_bits(solo, got, c["n"])
    assert not bad, bad
    if name in ("e_n5", "e_n6"):
        # the `n == 5` branch (one sample, niters = 1, no generator) and its neighbour: what does not hang on the ill-conditioned sample is exact
        d = max(np.abs(got["R"] - o["R"]).max(), np.abs(got["t"] - o["t"]).max())
        print("%s: max |R, t - oracle| %.3g, good %d / %d" % (name, d, got["good"], o["good"]))
        assert got["found"] == 1 and got["iters"] == 1 == o["iters"] and got["inliers"] == c["n"] == o["inliers"]
        assert got["mask"][:c["n"]].all() and abs(got["good"] - o["good"]) <= 1 and (got["mask_pose"][:c["n"]] != o["mask_pose"]).sum() <= 2      # group A's slack
    if name == "easy_e_1":
        # one sample, the same solver: whichever candidate the device keeps is one of the oracle's ten, to group A's 1e-6
        idx = g.get_subset(g.CvRNG(g.rng_state(c["seed"])), c["n"], 5, None, o["k0"], o["k1"])
        E, valid = g.essential_5pt(o["k0"][idx][None], o["k1"][idx][None])
        d = np.minimum(np.abs(E[0] - got["model"]).max((1, 2)), np.abs(E[0] + got["model"]).max((1, 2)))
        kept = int(np.argmin(np.abs(E[0] - o["model"]).max((1, 2))))
        print("easy_e_1: the device keeps the oracle's candidate %d (max difference %.3g, admitted by the oracle: %s); the oracle keeps candidate %d" % (
            int(np.argmin(d)), d.min(), bool(valid[0, np.argmin(d)]), kept))
        assert got["found"] == 1 and got["iters"] == 1 and d.min() <= 1e-6
    if name == "b_rot_e" and got["found"]:
        e_ref, e_dev = g.angle_error_mat(o["R"], c["gt"]), g.angle_error_mat(got["R"], c["gt"])
        print("b_rot_e: R misses the rotation by %.3g degrees, the oracle's by %.3g" % (e_dev, e_ref))
        assert got["inliers"] == c["n"] and e_dev <= 4 * e_ref
