"""The LETNet fixtures of tests/golden/make_golden_letnet.py: the shapes of letnet*.npz, the reference checkpoint, the tracking-error chain, the net restated
as a few lines of torch.nn.functional over the folded tensors (for the test that needs no GPU), and kpb_track_error restated in numpy."""
import numpy as np

from r2d2_fixtures import load_parts  # noqa: F401  (stem-generic: load_parts("letnet"), load_parts("letnet_track"))

SHAPES = ((32, 32), (32, 64), (64, 96), (96, 160), (480, 640))
PLAN = dict(c1=8, c2=16, grayscale=False)
TRACK_HW = (96, 128)
TRACK_CASES = (("shift", 300, 222, 222), ("warped", 1, 221, 217))       # name, pair seed, keypoints the reference detects, keypoints its warp keeps
TRACK_SETS = ("defaults", "fund")       # the class defaults (3, 3, 1, 40) and config_fund.yaml's (10, 21, 3, 40)
TRACK_DETECT = dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
CAP_PERCENT = 5                         # at most this share of a tracking case's points may be unstable


def checkpoint():
    """{name: torch tensor} as torch.load of the reference's weights/letnet.pth gives it (without num_batches_tracked)."""
    import torch
    return {k: torch.from_numpy(v) for k, v in load_parts("letnet_state_dict").items()}


def track_params(g, case, name):
    d, w, lv, it = (int(v) for v in g["%s.%s_prm" % (case, name)])
    return {"distance": d, "win_size": w, "levels": lv, "interation": it, "gray": False}


def track_views(case):
    """(view 0, view 1, h01) of a tracking case, as the generator made them."""
    from keypoint_bench_amd import synthetic
    H, W = TRACK_HW
    if case == "shift":
        v0, v1 = synthetic.image_pair(300, H, W)
        return v0, v1, np.array([[1, 0, -3], [0, 1, -2], [0, 0, 1]], np.float32)
    return synthetic.warped_pair(1, H, W, strength=1.0)


def chain(t, img):
    """(score [B,1,H,W], desc [B,3,H,W]) from the folded tensors `t` (weights.fold_letnet): LETNet.py:46-52."""
    import torch
    import torch.nn.functional as F
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    x1 = F.relu(F.conv2d(F.relu(F.conv2d(img, tt(t["b1c1.w"]), tt(t["b1c1.b"]), padding=1)), tt(t["b1c2.w"]), tt(t["b1c2.b"]), padding=1))
    z = F.conv2d(F.relu(F.conv2d(x1, tt(t["let.conv1.w"])[:, :, None, None])), tt(t["let.head.w"])[:, :, None, None])
    return torch.sigmoid(z[:, 3:4]), torch.sigmoid(z[:, :3])


def track_error64(kps01, tracked, scale):
    """tasks/VisualizeTrackingError.py:45-46 in float64 numpy: kps01 [n,>=2] normalised, tracked [n,2] pixels, scale (w - 1, h - 1) -> errors [n]."""
    d = np.asarray(kps01, np.float64)[:, :2] * np.asarray(scale, np.float64) - np.asarray(tracked, np.float64)
    return np.sqrt((d * d).sum(1))


def track_error32(kps01, tracked, scale):
    """The same as kpb_track_error states it: every operation rounded to fp32 on its own (include/kpb.h)."""
    k, t, s = np.asarray(kps01, np.float32)[:, :2], np.asarray(tracked, np.float32), np.asarray(scale, np.float32)
    dx, dy = k[:, 0] * s[0] - t[:, 0], k[:, 1] * s[1] - t[:, 1]
    return np.sqrt(dx * dx + dy * dy)


def wave_mean64(err):
    """kpb_track_error's mean of fp32 errors: float64, lane l of 64 sums rows l, l + 64, ... ascending, then the butterfly over the distances 32 .. 1."""
    e = np.asarray(err, np.float64)
    if e.size == 0:
        return np.float64("nan")
    s = np.zeros(64, np.float64)
    for i in range(e.size):         # ascending within every lane
        s[i % 64] += e[i]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[lanes ^ o]
    return s[0] / np.float64(e.size)
