"""Host matchers: mutual nearest neighbours on descriptors sampled at the keypoints; optical flow is not part of the stand-in."""
import torch


class OpticalFlow(object):
    def __init__(self, params=None):
        self.params = params

    def __call__(self, img1, img2, pts1, pts2, *a, **k):
        raise NotImplementedError("the stand-in has no optical flow")


def optical_flow_tensor(pts0, pts1, img0, img1, params=None):
    raise NotImplementedError("the stand-in has no optical flow")


def brute_force_matcher(pts0, pts1, desc_map_0, desc_map_1, params=None):
    """desc_map_* [1, C, H, W]: mutual nearest neighbours within max_distance -> (matched pts0, matched pts1)."""
    d0 = desc_map_0[0][:, pts0[:, 1].long(), pts0[:, 0].long()].t()
    d1 = desc_map_1[0][:, pts1[:, 1].long(), pts1[:, 0].long()].t()
    dist = torch.cdist(d0.double(), d1.double())
    i01, i10 = dist.argmin(1), dist.argmin(0)
    keep = (i10[i01] == torch.arange(len(i01))) & (dist.min(1).values <= (params or {}).get("max_distance", float("inf")))
    return pts0[keep], pts1[i01[keep]]
