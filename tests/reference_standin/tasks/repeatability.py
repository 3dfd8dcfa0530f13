"""Repeatability of two keypoint sets under a known warp (names imported at module level, as task modules do)."""
import torch
from utils.projection import warp
from utils.extracter import detection  # noqa: F401  (re-bound by install())


def val_key_points(kps0, kps1, warp01, warp10, th: int = 3):
    num_feat = min(kps0.shape[0], kps1.shape[0])
    k0, k01, _, _ = warp(kps0, warp01)
    k1, k10, _, _ = warp(kps1, warp10)
    if k0.shape[0] == 0 or k1.shape[0] == 0:
        return {"num_feat": 0, "repeatability": 0}
    dist = (torch.cdist(k0, k10) + torch.cdist(k01, k1)) / 2
    mutual = (dist.argmin(1)[dist.argmin(0)] == torch.arange(dist.shape[1]))
    close = dist.min(0).values[mutual] <= th
    return {"num_feat": num_feat, "repeatability": close.sum() / num_feat}
