"""The pipeline at the benchmark's own batch sizes: bench.py builds PairPipeline on 256 pairs (512 images) for ALIKE and XFeat and 16 pairs
for SuperPoint and DISK, with and without LightGlue, and at those sizes the library takes branches no smaller test reaches -- the sparse NMS
tail with its top-K pruning and select_topk reading the bitmap of confirmed maxima (from 192 maps of 480 x 640; one workgroup per image from
64 images), ALIKE's large-batch block 3 / 4 forms and head layout (16 images and more), the match prefilter (8 pairs and more), the
placement of a descriptor map of 4 GB and more (PairPipeline._place_map), and offsets past 2^31 / 2^32 bytes (images 27, 54) and
2^31 / 2^32 / 2^33 elements (images 109, 218, 436) of the 40 GB ALIKE map.

Each configuration, built the way bench.py builds it (same weights, same images, same batch):
  - every image and every pair against the oracle chain on the GPU's OWN maps, bit for bit: keypoints and flat indices, sampled
    descriptors, match indices and float64 distances, gathered rows (test_gpu_configs.py's pattern over the whole batch);
  - the net's maps in the batch against the same net on each image alone, and a few images against the float64 oracle forward;
  - with LightGlue: every pair against the single-pair drop-in, bit for bit, and one pair against oracle/lightglue_ref.py;
  - the state a pipeline carries from step to step: the same batch again, then the pairs in reverse order."""
import gc
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import oracle
from bench import BRUTE_FORCE, EXTRACTOR, H, W
from keypoint_bench_amd import synthetic, weights
from oracle import alike_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# pairs per step and GPU: the inline table of bench.py main() (`B = args.pairs_per_step or {...}[args.model]`)
PAIRS = {"alike": 256, "xfeat": 256, "superpoint": 16, "disk": 16}
LIGHTGLUE = {"disk": (128, 1), "superpoint": (256, 8)}     # bench.py main(): LightGlue's input width and desc_scale per net
# images of a 512-image ALIKE batch whose 78.6 MB slice of the map holds byte offset 2^31 (27) or 2^32 (54), element offset 2^31 (109),
# 2^32 (218) or 2^33 (436), their successors, the seam between the two views (255 | 256) and the ends
BOUNDARY = (0, 27, 28, 54, 55, 109, 110, 218, 219, 255, 256, 436, 437, 511)
# float64 oracle forward: ((rtol, atol) of the score map, atol of the descriptors).  SuperPoint, XFeat and DISK: the per-net bounds of
# test_gpu_superpoint / xfeat / disk.py.  ALIKE: test_gpu_alike.py's 7e-6 bounds the GPU against the torch-fp32 chain (F32_ATOL_SCORE below,
# checked as well); an fp32 evaluation's own distance from the float64 result is larger -- the torch-fp32 chain on the CPU is 1.65e-5 .. 1.77e-5
# from it on images 0, 27 and 511 -- so the float64 bound of the score is 2.5e-5.
F64_TOL = {"alike": ((0, 2.5e-5), 1e-4), "superpoint": ((2e-3, 1e-6), 1e-4), "xfeat": ((2e-3, 1e-7), 1e-4), "disk": ((0, 2e-5), 1e-4)}
F32_ATOL_SCORE, F32_ATOL_DESC = 7e-6, 1e-4      # ALIKE against oracle/alike_ref.py in fp32 (test_gpu_alike.py, test_gpu_parity_sweep.py)

_HOST_IMAGES = {}


def _images(B):
    """bench.py's images: synthetic.image_pair(i, H, W) for i < B from a 16-thread pool, all view-0 images first, then all view-1 images."""
    if B not in _HOST_IMAGES:
        with ThreadPoolExecutor(16) as ex:
            v0s, v1s = zip(*ex.map(lambda i: synthetic.image_pair(i, H, W), range(B)))
        _HOST_IMAGES[B] = np.stack(v0s + v1s)
    return _HOST_IMAGES[B]


def _net(name, dense=True):
    """bench.py's nets and seeds."""
    if name == "alike":
        from keypoint_bench_amd.models.ALike import alike_t
        return alike_t(dense_descriptors=dense).eval()
    if name == "superpoint":
        from keypoint_bench_amd.models.SuperPoint import superpoint_random
        return superpoint_random(7).eval()
    if name == "xfeat":
        from keypoint_bench_amd.models.XFeat import xfeat_random
        return xfeat_random(9).eval()
    from keypoint_bench_amd.models.disk import disk_random
    return disk_random(5).eval()


def _lightglue_state_dict(name):
    return weights.random_lightglue_state_dict(31, LIGHTGLUE[name][0], "plain")


def _pipeline(name, matcher="brute_force", dense=True):
    from keypoint_bench_amd.pipeline import PairPipeline
    lg = None
    if matcher == "lightglue":
        from keypoint_bench_amd.models.lightglue import LightGlue
        lg = LightGlue(features=None, desc_scale=LIGHTGLUE[name][1])
        lg.load_state_dict(_lightglue_state_dict(name))
    net = _net(name, dense)
    B = PAIRS[name]
    pipe = PairPipeline(net, EXTRACTOR, BRUTE_FORCE, B, H, W, device=DEV, lightglue=lg)    # map placement at its default
    images = torch.from_numpy(_images(B)).to(DEV).contiguous()
    pipe.run(images)
    return pipe, net, images


def _release(pipe):
    """Drop the pipeline's device buffers now (a failed test's traceback keeps the object itself alive) and return them to the driver."""
    if pipe is not None:
        for k, v in list(vars(pipe).items()):
            if torch.is_tensor(v) or isinstance(v, dict):
                setattr(pipe, k, None)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _what(pipe, name, matcher):
    return "%s + %s, %d pairs, placement %r" % (name, matcher, pipe.B, pipe.placement)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check_against_oracle(pipe, what):
    """Every image: oracle.detection on pipe.score[i] and oracle.sample on pipe.desc[i]; every pair: oracle.match on those, and the gathered
    rows.  Bit for bit.  The maps go to the host 32 images at a time; the oracle runs in a 16-thread pool (its C calls release the GIL)."""
    B, B2 = pipe.B, 2 * pipe.B
    bf = pipe.lg is None
    n, kps, idx = pipe.n.cpu().numpy(), pipe.kps.cpu().numpy(), pipe.idx.cpu().numpy()
    sdesc = pipe.sdesc.cpu().numpy() if bf else None
    okps, osd = [None] * B2, [None] * B2

    def image(i, score, desc):
        k, ix = oracle.detection(score, EXTRACTOR)
        assert n[i] == len(k), "%s: image %d: %d keypoints, the oracle %d" % (what, i, n[i], len(k))
        assert np.array_equal(_bits(kps[i, : n[i]]), _bits(k)), "%s: image %d: keypoints differ from the oracle's" % (what, i)
        assert np.array_equal(idx[i, : n[i]], ix), "%s: image %d: flat indices differ from the oracle's" % (what, i)
        okps[i] = k
        if bf:
            d = oracle.sample_hwc(desc, k)
            assert np.array_equal(_bits(sdesc[i, : n[i]]), _bits(d)), "%s: image %d: sampled descriptors differ from the oracle's" % (what, i)
            osd[i] = d

    kk, pairs, dist = pipe.k.cpu().numpy(), pipe.pairs.cpu().numpy(), (pipe.dist.cpu().numpy() if bf else None)
    m0, m1 = pipe.m0.cpu().numpy(), pipe.m1.cpu().numpy()

    def pair(b):
        k = int(kk[b])
        if bf:
            p, d = oracle.match(osd[b], osd[B + b], BRUTE_FORCE["max_distance"], BRUTE_FORCE["cross_check"])
            assert k == len(p), "%s: pair %d: %d matches, the oracle %d" % (what, b, k, len(p))
            assert np.array_equal(pairs[b, :k], p), "%s: pair %d: match indices differ from the oracle's" % (what, b)
            assert np.array_equal(_bits(dist[b, :k]), _bits(d)), "%s: pair %d: distances differ from the oracle's" % (what, b)
        p = pairs[b, :k]
        assert np.array_equal(_bits(m0[b, :k]), _bits(okps[b][p[:, 0]])), "%s: pair %d: gathered rows of image 0 differ" % (what, b)
        assert np.array_equal(_bits(m1[b, :k]), _bits(okps[B + b][p[:, 1]])), "%s: pair %d: gathered rows of image 1 differ" % (what, b)

    with ThreadPoolExecutor(16) as ex:
        for c0 in range(0, B2, 32):
            jobs = [ex.submit(image, i, pipe.score[i, 0].cpu().numpy(), pipe.desc[i].cpu().numpy() if bf else None)
                    for i in range(c0, min(c0 + 32, B2))]
            for j in jobs:
                j.result()
        list(ex.map(pair, range(B)))


def _check_lightglue(pipe, name, what):
    """Every pair through the single-pair drop-in on the same keypoints and maps: the same matches, scores and stop layer, bit for bit
    (test_gpu_lightglue.py's claim for a batch); the last pair against the fp32 oracle with test_gpu_configs.py's rules."""
    from oracle import lightglue_ref as R
    from test_gpu_configs import _compare_lightglue
    B, lg = pipe.B, pipe.lg
    n = pipe.n.cpu().numpy()
    for b in range(B):
        n0, n1 = int(n[b]), int(n[B + b])
        dm0, dm1 = pipe.desc[b].permute(2, 0, 1)[None], pipe.desc[B + b].permute(2, 0, 1)[None]
        pairs, scores, stop = lg.match_indices(pipe.kps[b, :n0], pipe.kps[B + b, :n1], dm0, dm1, {"w": W, "h": H})
        k = int(pipe.k[b])
        assert stop == int(pipe.lg_stop[b]), "%s: pair %d: stop layer %d in the batch, %d alone" % (what, b, int(pipe.lg_stop[b]), stop)
        assert torch.equal(pipe.pairs[b, :k].long(), pairs), "%s: pair %d: matches differ from the single-pair run" % (what, b)
        assert torch.equal(pipe.lg_scores[b, :k].view(torch.int32), scores.view(torch.int32)), \
            "%s: pair %d: scores differ from the single-pair run" % (what, b)
    t = {k: torch.from_numpy(v) for k, v in weights.tensors_lightglue(_lightglue_state_dict(name)).items()}
    b = B - 1
    n0, n1, k = int(n[b]), int(n[B + b]), int(pipe.k[b])
    d0 = pipe.desc[b].permute(2, 0, 1)[None].cpu().contiguous()
    d1 = pipe.desc[B + b].permute(2, 0, 1)[None].cpu().contiguous()
    with torch.no_grad():
        _, _, out = R.match(t, pipe.kps[b, :n0].cpu(), pipe.kps[B + b, :n1].cpu(), d0, d1, {"w": W, "h": H}, LIGHTGLUE[name][1])
    assert int(pipe.lg_stop[b]) == out["stop"], what
    _compare_lightglue(pipe.pairs[b, :k].cpu().numpy(), pipe.lg_scores[b, :k].cpu().numpy(), out)


def _f64_forward(name, img):
    """oracle/*_ref.py on a float64 image with float64 weights."""
    from oracle import disk_ref, superpoint_ref, xfeat_ref
    if name == "alike":
        fwd, t = alike_ref.alnet_forward, weights.load_alike_t()
    elif name == "superpoint":
        fwd, t = superpoint_ref.superpoint_forward, weights.random_superpoint(7)
    elif name == "xfeat":
        fwd, t = xfeat_ref.xfeat_forward, weights.fold_xfeat(weights.random_xfeat_state_dict(9))
    else:
        fwd, t = disk_ref.disk_forward, weights.tensors_disk(weights.random_disk_state_dict(5))
    t = {k: torch.as_tensor(np.asarray(v)).double() for k, v in t.items()}
    with torch.no_grad():
        return fwd(torch.from_numpy(img)[None].double(), t)


def _check_f64(pipe, name, which, what):
    (rt, at), ad = F64_TOL[name]
    imgs = _images(pipe.B)
    for i in which:
        score, desc = pipe.score[i, 0].cpu().double().numpy(), pipe.desc[i].permute(2, 0, 1).cpu().double().numpy()
        so, do = _f64_forward(name, imgs[i])
        np.testing.assert_allclose(score, so[0, 0].numpy(), rtol=rt, atol=at, err_msg="%s: image %d: score map against the float64 oracle" % (what, i))
        np.testing.assert_allclose(desc, do[0].numpy(), rtol=0, atol=ad, err_msg="%s: image %d: descriptor map against the float64 oracle" % (what, i))
        if name == "alike":
            t = {k: torch.from_numpy(v) for k, v in weights.load_alike_t().items()}
            with torch.no_grad():
                so, do = alike_ref.alnet_forward(torch.from_numpy(imgs[i])[None], t)
            np.testing.assert_allclose(score, so[0, 0].numpy(), rtol=0, atol=F32_ATOL_SCORE, err_msg="%s: image %d: score map against the fp32 oracle" % (what, i))
            np.testing.assert_allclose(desc, do[0].numpy(), rtol=0, atol=F32_ATOL_DESC, err_msg="%s: image %d: descriptor map against the fp32 oracle" % (what, i))


def _check_batch_against_single(pipe, net, images, which, what):
    """The same net on image i alone (its own launch shapes) against slot i of the batch, bit for bit: test_gpu_alike.py and
    test_gpu_superpoint.py claim it; XFeat and DISK (whose tests bound the score maps by 1e-5 relative / 2e-6 absolute) hold it as well."""
    for i in which:
        s1, d1 = net(images[i:i + 1])
        s1, d1 = s1[0], d1[0].permute(1, 2, 0)           # [1, H, W] and the [Hd, Wd, C] storage of the [C, Hd, Wd] view
        assert torch.equal(s1, pipe.score[i]), "%s: image %d: score map differs from the single-image forward" % (what, i)
        assert torch.equal(d1, pipe.desc[i]), "%s: image %d: descriptor map differs from the single-image forward" % (what, i)


def _snapshot(pipe):
    """Host copies of what a step leaves; rows past each image's keypoint count / each pair's match count (never written) zeroed."""
    B = pipe.B
    n, k = pipe.n.cpu().numpy(), pipe.k.cpu().numpy()
    out = {"n": n, "k": k, "score": pipe.score.cpu().numpy()}
    per_image = ["kps", "idx"] + (["sdesc"] if pipe.lg is None else [])
    per_pair = ["pairs", "m0", "m1"] + (["dist"] if pipe.lg is None else ["lg_scores"])
    for names, cnt in ((per_image, n), (per_pair, k)):
        for name in names:
            a = getattr(pipe, name).cpu().numpy().copy()
            for r in range(a.shape[0]):
                a[r, cnt[r]:] = 0
            out[name] = a
    if pipe.lg is not None:
        out["lg_stop"] = pipe.lg_stop.cpu().numpy()
    return out


def _check_steps(pipe, images, keep, what):
    """The benchmark runs one pipeline for hundreds of steps: the same batch again gives the same outputs, and the pairs in reverse order
    give the first step's outputs in reverse order (descriptor maps: the images in `keep`)."""
    B = pipe.B
    first = _snapshot(pipe)
    maps = {i: pipe.desc[i].clone() for i in keep} if pipe.desc is not None else {}
    pipe.run(images)
    again = _snapshot(pipe)
    for name, a in first.items():
        assert np.array_equal(_bits(again[name]), _bits(a)), "%s: %s differs on the second step" % (what, name)
    for i, d in maps.items():
        assert torch.equal(pipe.desc[i], d), "%s: image %d: descriptor map differs on the second step" % (what, i)
    rev = np.arange(B - 1, -1, -1)
    perm = np.concatenate([rev, rev + B])
    pipe.run(images[torch.from_numpy(perm).to(images.device)].contiguous())
    third = _snapshot(pipe)
    for name, a in first.items():
        want = a[perm] if a.shape[0] == 2 * B else a[rev]
        assert np.array_equal(_bits(third[name]), _bits(want)), "%s: %s differs with the pairs in reverse order" % (what, name)
    for i, d in maps.items():
        j = int(np.nonzero(perm == i)[0][0])
        assert torch.equal(pipe.desc[j], d), "%s: image %d (slot %d): descriptor map differs with the pairs in reverse order" % (what, i, j)


CONFIGS = [("alike", "brute_force"), ("xfeat", "brute_force"), ("superpoint", "brute_force"), ("disk", "brute_force"),
           ("superpoint", "lightglue"), ("disk", "lightglue")]


_DENSE_ALIKE = {}      # the first step's outputs of the dense ALIKE configuration, for the keypoint-only test


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("name,matcher", CONFIGS, ids=[n if m == "brute_force" else n + "_lightglue" for n, m in CONFIGS])
def test_bench_configuration_against_the_oracle_at_the_benchmark_batch(name, matcher):
    pipe = None
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    try:
        pipe, net, images = _pipeline(name, matcher)
        what = _what(pipe, name, matcher)
        B2 = 2 * pipe.B
        if name == "alike":
            _DENSE_ALIKE["first"] = _snapshot(pipe)
        _check_against_oracle(pipe, what)
        if matcher == "lightglue":
            _check_lightglue(pipe, name, what)
        few = BOUNDARY if name == "alike" else (0, B2 - 1)
        _check_f64(pipe, name, few, what)
        _check_batch_against_single(pipe, net, images, range(B2), what)
        _check_steps(pipe, images, few, what)
        print("%s: %.1f s, torch peak %.1f GB" % (what, time.time() - t0, torch.cuda.max_memory_allocated() / 1e9))
    finally:
        _release(pipe)


@pytest.mark.timeout(900)
def test_keypoint_only_alike_gives_the_dense_runs_keypoints_and_matches():
    """bench.py --sparse (and the `variant` leg of --full): ALNet(dense_descriptors=False) on the same 256 pairs -- the 40 GB map is never
    written, descriptors are computed at the keypoints.  Exactly the dense run's: every image's keypoint count and keypoint pixels (flat indices
    and the (x, y) columns, bit for bit), every pair's match count and matches as pixel pairs.  Not bit for bit: the score-only head evaluates the
    score row in its linear form (test_gpu_alike.py: within 2e-6 of the dense map) -- so rows of near-equal score may come out in another order
    -- and the descriptors at the keypoints re-associate the same sums (within 2e-5 per channel), so a distance is within 2 * sqrt(64) * 2e-5."""
    pipe = None
    try:
        if "first" not in _DENSE_ALIKE:         # (this test run on its own)
            pipe, _, _ = _pipeline("alike")
            _DENSE_ALIKE["first"] = _snapshot(pipe)
            _release(pipe)
        dense = _DENSE_ALIKE["first"]
        pipe, _, _ = _pipeline("alike", dense=False)
        assert pipe.placement is None and pipe.desc is None
        sparse = _snapshot(pipe)
        B = pipe.B
        assert np.array_equal(sparse["n"], dense["n"]), "keypoint-only ALIKE: keypoint counts differ from the dense run"
        assert np.array_equal(sparse["k"], dense["k"]), "keypoint-only ALIKE: match counts differ from the dense run"
        rows, reordered, dscore, ddist = [], 0, 0.0, 0.0
        for i in range(2 * B):
            n = int(dense["n"][i])
            di, si = dense["idx"][i, :n], sparse["idx"][i, :n]
            assert set(di.tolist()) == set(si.tolist()), "keypoint-only ALIKE: image %d: keypoint pixels differ from the dense run" % i
            reordered += int((di != si).any())
            od, os_ = np.argsort(di, kind="stable"), np.argsort(si, kind="stable")      # rows by pixel
            kd, ks = dense["kps"][i, od], sparse["kps"][i, os_]
            assert np.array_equal(_bits(kd[:, :2]), _bits(ks[:, :2])), "keypoint-only ALIKE: image %d: keypoint positions differ" % i
            np.testing.assert_allclose(ks[:, 2], kd[:, 2], rtol=0, atol=2e-6, err_msg="keypoint-only ALIKE: image %d: scores" % i)
            dscore = max(dscore, float(np.abs(ks[:, 2] - kd[:, 2]).max()))
        for b in range(B):
            sets = []
            for r in (dense, sparse):
                p = r["pairs"][b, : int(r["k"][b])]
                sets.append(dict(zip(zip(r["idx"][b][p[:, 0]].tolist(), r["idx"][B + b][p[:, 1]].tolist()), r["dist"][b, : len(p)].tolist())))
            assert sets[0].keys() == sets[1].keys(), "keypoint-only ALIKE: pair %d: matches differ from the dense run" % b
            d = max((abs(sets[0][m] - sets[1][m]) for m in sets[0]), default=0.0)
            assert d <= 2 * 8 * 2e-5, "keypoint-only ALIKE: pair %d: a distance differs from the dense run's by %.3g" % (b, d)
            ddist = max(ddist, d)
        print("keypoint-only ALIKE against the dense run: %d of %d images list their keypoints in another order; largest differences %.3g (score), "
              "%.3g (distance)" % (reordered, 2 * B, dscore, ddist))
    finally:
        _release(pipe)
