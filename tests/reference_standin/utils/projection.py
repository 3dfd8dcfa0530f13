"""Host warps.  `warp` dispatches through this module's globals."""
import torch


def warp_homography(kpts0, params):
    """kpts0 [N, 2] in pixels -> (covisible kpts0, their warped positions, covisible ids, the other ids)."""
    xy1 = torch.cat([kpts0, torch.ones_like(kpts0[:, :1])], dim=1) @ params["homography_matrix"].float().t()
    xy = xy1[:, :2] / xy1[:, 2:]
    w, h = float(params["width"]), float(params["height"])
    ok = (xy[:, 0] >= 0) & (xy[:, 0] <= w - 1) & (xy[:, 1] >= 0) & (xy[:, 1] <= h - 1)
    ids = torch.arange(kpts0.shape[0])
    return kpts0[ok], xy[ok], ids[ok], ids[~ok]


def warp_se3(kpts0, params):
    raise NotImplementedError("the stand-in has no depth warp")


def warp(kpts0, params):
    if params["mode"] == "homo":
        return warp_homography(kpts0[:, 0:2], params)
    if params["mode"] == "se3":
        return warp_se3(kpts0[:, 0:2], params)
    raise ValueError("unknown mode")
