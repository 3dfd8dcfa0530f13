"""Drop-in for the brute-force branch of the reference's utils/matcher.py (lines 206-234), computed by
csrc/match.hip through libkpb.so; its two trackers: OpticalFlow / optical_flow_tensor (7-142, 188-203: csrc/lk.hip) and
optical_flow_cv (145-185: csrc/pyrlk.hip -- restated, cv2 parity unpinned)."""
import ctypes

import torch

from .._lib import Context, LkParams, MatchParams, metric_id, ptr


def sample_descriptors(pts: torch.Tensor, desc_map, n=None) -> torch.Tensor:
    """utils/matcher.py:221-226: bilinear grid_sample(align_corners=True) of desc_map [1,C,Hd,Wd] at
    pts [N, >=2] (x, y normalised) -> [N, C].  desc_map may be a LazyDescriptors handle (models/)."""
    if hasattr(desc_map, "sample"):
        return desc_map.sample(pts)
    if not desc_map.is_cuda:
        raise RuntimeError("keypoint_bench_amd needs CUDA/HIP tensors; there is no CPU path")
    d = desc_map.detach()
    if d.dtype != torch.float32:
        d = d.float()
    p = pts.detach().to(torch.float32).contiguous()
    _, C, Hd, Wd = d.shape
    N = p.shape[0]
    out = torch.empty((N, C), dtype=torch.float32, device=d.device)
    if N:
        ctx = Context.get(d.device)
        sb, sc, sh, sw = d.stride()
        ctx.check(ctx.lib.kpb_sample(ctx.handle, ptr(d), 1, C, Hd, Wd, sb, sc, sh, sw, ptr(p), p.shape[1], N,
                                     ptr(None), ptr(out)))
    return out


def match_ratio_of(params):
    """The optional max_ratio key of brute_force_params (skimage's Lowe ratio test; absent = 1.0 = off).  NaN is refused here as the library refuses it."""
    r = float((params or {}).get("max_ratio", 1.0))
    if r != r:
        raise ValueError("max_ratio is NaN")
    return r


def _match32(desc0: torch.Tensor, desc1: torch.Tensor, max_distance, cross_check, want_dist=False, max_ratio=1.0, metric=0):
    """kpb_match_ratio (kpb_match itself while max_ratio >= 1), under KPB_OPT_MATCH_METRIC = metric for a KPB_METRIC_* id other than euclidean's 0, for one pair: (pairs int32 [n, 2] -- the first K rows are the matches --, dist float64 [n] or None, K device
    tensor [1], K as a host integer).  K comes from pinned host memory the kernel wrote (kpb_match_counts): one stream
    synchronisation, no read-back of its own."""
    a = desc0.detach().to(torch.float32).contiguous()
    b = desc1.detach().to(torch.float32).contiguous()
    n, m = a.shape[0], b.shape[0]
    dev = a.device
    ctx = Context.get(dev)
    pairs = torch.empty((n, 2), dtype=torch.int32, device=dev)
    dist = torch.empty((n,), dtype=torch.float64, device=dev) if want_dist else None
    k = torch.empty((1,), dtype=torch.int32, device=dev)
    prm = MatchParams(float(max_distance), 1 if cross_check else 0)
    with ctx.match_metric(metric):
        ctx.check(ctx.lib.kpb_match_ratio(ctx.handle, ptr(a), ptr(b), 1, a.shape[1], n, m, ptr(None), ptr(None),
                                          ctypes.byref(prm), float(max_ratio), ptr(pairs), ptr(dist), ptr(k)))
    kk = (ctypes.c_int32 * 1)()
    ctx.check(ctx.lib.kpb_match_counts(ctx.handle, kk, 1))
    return pairs, dist, k, int(kk[0])


def match_descriptors(desc0: torch.Tensor, desc1: torch.Tensor, metric="euclidean", max_distance=float("inf"),
                      cross_check=True, return_distance=False, max_ratio=1.0):
    """skimage.feature.match_descriptors as the reference calls it (matcher.py:227-230), on device.
    metric: "euclidean", "sqeuclidean", "cityblock", "chebyshev" or "cosine", each scipy cdist's float64 value (include/kpb.h, KPB_OPT_MATCH_METRIC).
    Returns int64 [K, 2] (and float64 [K] distances when asked).  max_ratio < 1: skimage's ratio test on the exact float64 second nearest
    (include/kpb.h, kpb_match_ratio); 1.0 and above: off."""
    metric = metric_id(metric)
    dev = desc0.device
    max_ratio = match_ratio_of({"max_ratio": max_ratio})
    if desc0.shape[0] == 0 or desc1.shape[0] == 0:
        e = torch.zeros((0, 2), dtype=torch.int64, device=dev)
        return (e, torch.zeros((0,), dtype=torch.float64, device=dev)) if return_distance else e
    pairs, dist, _, kk = _match32(desc0, desc1, max_distance, cross_check, want_dist=True, max_ratio=max_ratio, metric=metric)
    pairs = pairs[:kk].to(torch.int64)
    return (pairs, dist[:kk].clone()) if return_distance else pairs


def brute_force_matcher(pts0: torch.Tensor, pts1: torch.Tensor, desc_map_0, desc_map_1, params=None):
    """utils/matcher.py:206-234.  pts0 (n, >=2), pts1 (m, >=2) in [0,1]; returns the matched rows of pts0 and
    pts1 (all columns kept), ordered by ascending index into pts0.  An optional params["max_ratio"] < 1 adds skimage's ratio test (the reference's own
    function does not read that key)."""
    metric = metric_id(params["metric"])
    max_ratio = match_ratio_of(params)
    desc0 = sample_descriptors(pts0, desc_map_0)
    desc1 = sample_descriptors(pts1, desc_map_1)
    if desc0.shape[0] == 0 or desc1.shape[0] == 0:
        return pts0[:0], pts1[:0]
    # the int32 pairs and the device count feed the row gather as they are (r03 converted to int64 and back and uploaded K again)
    m32, _, k_dev, k = _match32(desc0, desc1, params["max_distance"], params["cross_check"], max_ratio=max_ratio, metric=metric)
    if k == 0:
        return pts0[:0], pts1[:0]
    ctx = Context.get(pts0.device)
    outs = []
    for col, pts in ((0, pts0), (1, pts1)):
        p = pts.detach().to(torch.float32).contiguous()
        out = torch.empty((k, p.shape[1]), dtype=torch.float32, device=p.device)
        ctx.check(ctx.lib.kpb_gather_rows(ctx.handle, ptr(p), 1, p.shape[0], p.shape[1], ptr(m32), k, 2, col, ptr(k_dev),
                                          ptr(out)))
        outs.append(out)
    return outs[0], outs[1]


class OpticalFlow(object):
    """utils/matcher.py:7-142: pyramidal Lucas-Kanade on win_size x win_size x C windows, computed by csrc/lk.hip (one
    wave per keypoint, nothing unfolded).  Same constructor keys, same call, same return: (points [1,N,2] in PIXELS of
    the full image, error [1,N])."""

    def __init__(self, params=None):
        if params is None:
            params = {"distance": 3, "win_size": 3, "levels": 1, "interation": 40, "gray": False}      # matcher.py:9-16
        self.distance, self.win_size, self.levels = params["distance"], params["win_size"], params["levels"]
        self.interation, self.gray = params["interation"], params["gray"]

    def __call__(self, img1, img2, pts1, pts2, random_angle=None):
        if not img1.is_cuda:
            raise RuntimeError("keypoint_bench_amd needs CUDA/HIP tensors; there is no CPU path")
        N, C, H, W = img1.shape
        if N != 1:
            raise ValueError("one image pair per call (the reference indexes batch element 0, matcher.py:60)")
        if C != (1 if self.gray else 3):        # the reference's Sobel weight is [C,C,3,3] with C fixed by `gray` (26-36)
            raise ValueError("images must have %d channel(s) for gray=%s" % (1 if self.gray else 3, self.gray))
        dev = img1.device
        a = img1.detach().to(torch.float32).contiguous()
        b = img2.detach().to(torch.float32).contiguous()
        if pts1.shape[-1] < 2 or pts2.shape[-1] < 2:
            raise ValueError("points need (x, y) columns")
        # the kernel takes one stride for both arrays: hand it the (x, y) columns of each, whatever else the rows carry
        p1 = pts1.detach()[:, :2].to(torch.float32).contiguous()
        p2 = pts2.detach()[:, :2].to(torch.float32).contiguous()
        n = p1.shape[0]
        if p2.shape[0] != n:
            raise ValueError("pts1 and pts2 must have one row per track")
        if random_angle is None:
            random_angle = torch.randn(n, device=dev) * 6.28                                             # 55
        unit = torch.stack([torch.cos(random_angle), torch.sin(random_angle)], dim=1).to(torch.float32).contiguous()   # 56
        out = torch.empty((n, 2), dtype=torch.float32, device=dev)
        err = torch.empty((n,), dtype=torch.float32, device=dev)
        if n:
            ctx = Context.get(dev)
            prm = LkParams(float(self.distance), int(self.win_size), int(self.levels), int(self.interation))
            ctx.check(ctx.lib.kpb_lk_track(ctx.handle, ptr(a), ptr(b), C, H, W, ptr(p1), ptr(p2), 2, ptr(unit), n,
                                           ctypes.byref(prm), ptr(out), ptr(err)))
        return out.unsqueeze(0), err.unsqueeze(0)


def optical_flow_tensor(pts0, pts1, img0, img1, params=None, random_angle=None):
    """utils/matcher.py:186-203.  random_angle [n]: the tracker's start angles (drawn as the reference draws them when missing)."""
    pts1_, _ = OpticalFlow(params)(img0, img1, pts0, pts1, random_angle=random_angle)
    return pts1_


def track_error(kps01, tracked, scale, n=None):
    """tasks/VisualizeTrackingError.py:45-46 for B pairs in one kpb_track_error call: kps01 [B,K,>=2] normalised warped keypoints, tracked [B,K,2] pixels (what
    optical_flow_batch returns), scale [B,2] = (w - 1, h - 1), n [B] int32 on the device or None (= K).  Returns (error [B,K] fp32, mean [B] float64); rows past
    n[j] are left as allocated, a pair without rows has a NaN mean."""
    if not tracked.is_cuda:
        raise RuntimeError("keypoint_bench_amd needs CUDA/HIP tensors; there is no CPU path")
    if kps01.dim() != 3 or kps01.shape[-1] < 2 or tracked.shape != kps01.shape[:2] + (2,) or scale.shape != (kps01.shape[0], 2):
        raise ValueError("kps01 [B,K,>=2], tracked [B,K,2], scale [B,2]")
    dev = tracked.device
    a = kps01.detach().to(torch.float32).contiguous()
    b = tracked.detach().to(torch.float32).contiguous()
    s = scale.detach().to(torch.float32).contiguous()
    B, K = a.shape[:2]
    err = torch.empty((B, K), dtype=torch.float32, device=dev)
    mean = torch.empty((B,), dtype=torch.float64, device=dev)
    if B:
        ctx = Context.get(dev)
        ctx.check(ctx.lib.kpb_track_error(ctx.handle, ptr(a), a.shape[2], ptr(b), B, K, ptr(n), ptr(s), ptr(err), ptr(mean)))
    return err, mean


def optical_flow_batch(maps1, maps2, pts1, pts2, n, params, random_angle=None):
    """The tracker for B pairs in one kpb_lk_track_batch call: pair j follows pts (normalised rows, as OpticalFlow takes them) from maps1[j] into
    maps2[j].  maps1 / maps2 [B,C,H,W] fp32 of ANY strides, both with the same ones -- a planar stack of frames, the channels-last storage behind a
    net's [B,C,H,W] descriptor view, or two shifted views of one buffer (maps[:-1], maps[1:]): the strides are passed on, nothing is copied.
    pts1 / pts2 [B,K,>=2] (the same tensor is fine), n [B] int32 on the device or None (= K), random_angle [B,K] (drawn as the reference draws them,
    matcher.py:55, when missing).  Returns (points [B,K,2] in PIXELS, error [B,K]); rows past n[j] are left as allocated.  Every pair's rows are the
    bits of OpticalFlow(params) on that pair."""
    if params is None:
        params = {"distance": 3, "win_size": 3, "levels": 1, "interation": 40, "gray": False}
    if not maps1.is_cuda:
        raise RuntimeError("keypoint_bench_amd needs CUDA/HIP tensors; there is no CPU path")
    B, C, H, W = maps1.shape
    if maps1.dtype != torch.float32 or maps2.dtype != torch.float32:
        raise ValueError("maps must be float32")
    if maps2.shape != maps1.shape or maps2.stride() != maps1.stride():
        raise ValueError("maps1 and maps2 must have one shape and one set of strides")
    if C != (1 if params["gray"] else 3):
        raise ValueError("maps must have %d channel(s) for gray=%s" % (1 if params["gray"] else 3, params["gray"]))
    if pts1.shape[-1] < 2 or pts2.shape[-1] < 2 or pts1.shape != pts2.shape or pts1.stride() != pts2.stride() or pts1.shape[0] != B:
        raise ValueError("points need (x, y) columns, one [B,K,cols] layout for both arrays")
    p1, p2 = pts1.detach(), pts2.detach()
    if p1.dtype != torch.float32 or not p1.is_contiguous() or not p2.is_contiguous():
        p1, p2 = p1.to(torch.float32).contiguous(), p2.to(torch.float32).contiguous()
    K, dev = p1.shape[1], maps1.device
    if random_angle is None:
        random_angle = torch.randn((B, K), device=dev) * 6.28                                            # 55
    unit = torch.stack([torch.cos(random_angle), torch.sin(random_angle)], dim=2).to(torch.float32).contiguous()   # 56
    out = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
    err = torch.empty((B, K), dtype=torch.float32, device=dev)
    if K:
        ctx = Context.get(dev)
        sb, sc, sh, sw = maps1.stride()
        prm = LkParams(float(params["distance"]), int(params["win_size"]), int(params["levels"]), int(params["interation"]))
        ctx.check(ctx.lib.kpb_lk_track_batch(ctx.handle, ptr(maps1), ptr(maps2), B, C, H, W, sb, sc, sh, sw, ptr(p1), ptr(p2), p1.shape[2], ptr(unit), K,
                                             ptr(n), ctypes.byref(prm), ptr(out), ptr(err)))
    return out, err


PYRLK_DEFAULTS = {"win_size": 15, "levels": 3}      # matcher.py:158-162


def optical_flow_cv_batch(maps1, maps2, pts1, pts2, n=None, params=None):
    """The pyramidal tracker behind optical_flow_cv for B pairs in ONE kpb_lk_track_batch call under KPB_OPT_LK_PYRLK (csrc/pyrlk.hip; RESTATED, cv2 parity unpinned: include/kpb.h): pair j
    follows pts1[j] (normalised rows) from maps1[j] into maps2[j], starting at pts2[j].  maps1 / maps2 [B,C,H,W] fp32 of ANY strides, both with the same ones, C 1 or 3
    -- planar frames, the channels-last storage behind a net's map, or two shifted views of one buffer; pts1 / pts2 [B,K,>=2] (one tensor is fine); n [B] int32 on
    the device or None (= K).  Returns (points [B,K,2] NORMALISED, status [B,K] uint8, 1 = tracked); rows past n[j] are left as allocated.  Every pair's rows are the
    bits of optical_flow_cv on that pair."""
    if params is None:
        params = PYRLK_DEFAULTS
    if not (maps1.is_cuda and maps2.is_cuda and pts1.is_cuda and pts2.is_cuda):
        raise RuntimeError("keypoint_bench_amd needs CUDA/HIP tensors; there is no CPU path")
    if maps1.dim() != 4 or maps1.dtype != torch.float32 or maps2.dtype != torch.float32:
        raise ValueError("maps must be float32 [B,C,H,W]")
    if maps2.shape != maps1.shape or maps2.stride() != maps1.stride():
        raise ValueError("maps1 and maps2 must have one shape and one set of strides")
    B, C, H, W = maps1.shape
    if pts1.dim() != 3 or pts1.shape[-1] < 2 or pts1.shape != pts2.shape or pts1.stride() != pts2.stride() or pts1.shape[0] != B:
        raise ValueError("points need (x, y) columns, one [B,K,cols] layout for both arrays")
    p1, p2 = pts1.detach(), pts2.detach()
    if p1.dtype != torch.float32 or p2.dtype != torch.float32 or not p1.is_contiguous() or not p2.is_contiguous():
        p1, p2 = p1.to(torch.float32).contiguous(), p2.to(torch.float32).contiguous()
    K, dev = p1.shape[1], maps1.device
    out = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
    flag = torch.empty((B, K), dtype=torch.float32, device=dev)        # the status as the entry writes it: 1.0 / 0.0 where the tensor tracker's error column stands
    if B and K:
        ctx = Context.get(dev)
        sb, sc, sh, sw = maps1.stride()
        prm = LkParams(0.0, int(params["win_size"]), int(params["levels"]), 0)         # distance and iterations are not read under the option
        with ctx.lk_pyrlk():
            ctx.check(ctx.lib.kpb_lk_track_batch(ctx.handle, ptr(maps1), ptr(maps2), B, C, H, W, max(sb, 1), sc, sh, sw, ptr(p1), ptr(p2), p1.shape[2], ptr(None), K,
                                                 ptr(n), ctypes.byref(prm), ptr(out), ptr(flag)))
    status = (flag == 1.0).to(torch.uint8)       # rows past n[j] hold whatever the buffer held
    return out, status


def optical_flow_cv(pts0, pts1, img0, img1, params=None):
    """utils/matcher.py:145-185 on the device: pts0 (n, >=2) in [0, 1] are followed from img0 into img1 [1,C,H,W], starting at pts1; params: win_size / levels
    (15 / 3 when None).  Returns (points [n,2] fp32 normalised, status [n,1] uint8) ON THE DEVICE (the reference hands the status back as cv2's numpy array; the
    shim's wrapper does that conversion).  RESTATED, cv2 parity unpinned: what is computed is the definition in DESIGN.md section 7a, bit for bit."""
    if not (torch.is_tensor(img0) and img0.is_cuda):
        raise RuntimeError("keypoint_bench_amd needs CUDA/HIP tensors; there is no CPU path")
    if img0.dim() != 4 or img0.shape[0] != 1 or pts0.shape[0] != pts1.shape[0]:
        raise ValueError("one image pair per call, one guess per point (matcher.py:166)")
    a = img0.detach().to(torch.float32)
    b = img1.detach().to(torch.float32)
    if b.stride() != a.stride():
        a, b = a.contiguous(), b.contiguous()
    p0 = pts0.detach()[:, :2].to(torch.float32).contiguous()
    p1 = pts1.detach()[:, :2].to(torch.float32).contiguous()
    out, status = optical_flow_cv_batch(a, b, p0[None], p1[None], None, params)
    return out[0], status[0].unsqueeze(1)
