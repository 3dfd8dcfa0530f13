"""Host detector: NMS by a max filter, border removal, score threshold, top-k.  `detection` reaches `fast_nms` through this module's globals."""
import torch
import torch.nn.functional as F


def fast_nms(image_probs, nms_dist=4, max_iter=-1, min_value=0.0):
    """Keeps each value that is the maximum of the (nms_dist + 1)-wide window around it, zeroes the rest."""
    k = nms_dist + 1
    peak = F.max_pool2d(F.pad(image_probs, (k // 2, (k - 1) // 2, k // 2, (k - 1) // 2), value=float("-inf")), k, stride=1)
    return torch.where(image_probs == peak, image_probs, torch.zeros_like(image_probs))


def detection(score_map, params=None):
    """score_map [1, 1, H, W] -> [N, 3] rows (x, y, score), highest scores first."""
    p = params or dict(nms_dist=4, threshold=0.0, border_dist=8, top_k=300, min_score=0.0)
    nms = fast_nms(score_map.detach(), nms_dist=p["nms_dist"])[0, 0]
    b = p["border_dist"]
    inner = torch.zeros_like(nms)
    inner[b:nms.shape[0] - b, b:nms.shape[1] - b] = nms[b:nms.shape[0] - b, b:nms.shape[1] - b]
    ys, xs = torch.nonzero(inner > p["threshold"], as_tuple=True)
    pts = torch.stack([xs.float(), ys.float(), inner[ys, xs]], dim=1)
    pts = pts[torch.argsort(pts[:, 2], descending=True, stable=True)[:p["top_k"]]]
    return pts[pts[:, 2] > p["min_score"]] if p["min_score"] > 0 else pts
