"""The Key.Net fixtures of tests/golden/make_golden_keynet.py: the shapes of keynet*.npz, the reference checkpoint, the detection cases, the net restated as a
few lines of torch.nn.functional over the folded tensors (for the test that needs no GPU), and the two tolerance multipliers the GPU test holds the kernels to."""
import numpy as np

from r2d2_fixtures import load_parts  # noqa: F401  (stem-generic: load_parts("keynet"), load_parts("keynet_detect"))

SHAPES = ((16, 16), (30, 50), (37, 61), (96, 160), (480, 640))
LEVELS = {(16, 16): ((13, 13), (10, 10)), (30, 50): ((25, 41), (20, 34)), (37, 61): ((30, 50), (25, 41)), (96, 160): ((80, 133), (66, 110)),
          (480, 640): ((400, 533), (333, 444))}
PLAN = dict(num_filters=8, num_levels=3, kernel_size=5)
DETECT_SHAPES = ((96, 160), (37, 61))
# (nms_dist, top_k) of every detection case; border_dist 8, threshold 0, min_score 0
DETECT_CASES = ((2, 5000), (4, 5000), (2, 100))
DETECT_CAP_PERCENT = 2          # the device map's keypoints may differ from the reference's by at most this share of the reference count (as a set of pixels)
BORDER = 8                      # the ring the GPU test checks apart from the interior

# max |device - reference| <= M x ref_err per golden shape (ref_err: the reference's own fp32-against-fp64 difference, stored per shape).  The multipliers are
# the smallest powers of two that are at least twice the largest ratio measured on an MI355X over the five shapes (tests/test_gpu_keynet.py has the ratios);
# the strict-fp32 kernels do the reference's arithmetic in another order, so M_FP32 above 16 would be a defect, not a tolerance.
M_H16 = 4       # measured 1.713 (37 x 61, ring)
M_FP32 = 8      # measured 2.094 (37 x 61, ring)
assert M_FP32 <= 16


def checkpoint():
    """{name: torch tensor}: the 'state_dict' entry of the reference's weights/keynet_pytorch.pth (without num_batches_tracked)."""
    import torch
    return {k: torch.from_numpy(v) for k, v in load_parts("keynet_state_dict").items()}


def detect_params(nms_dist, top_k):
    return dict(nms_dist=int(nms_dist), threshold=0.0, border_dist=8, top_k=int(top_k), min_score=0.0)


def spatial_gradient(x):
    """[B,1,h,w] -> (d/dx, d/dy): the 3 x 3 Sobel pair / 8 as correlation over the REPLICATE-padded map (KeyNet.py:17)."""
    import torch
    import torch.nn.functional as F
    kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=x.dtype) / 8
    g = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), torch.stack([kx, kx.t()])[:, None])
    return g[:, 0:1], g[:, 1:2]


def pyrdown(x):
    """KeyNet.py:85-96 with factor 1.2: 5 x 5 binomial blur over the REFLECT-padded map, then bilinear to (int(h // 1.2), int(w // 1.2))."""
    import torch
    import torch.nn.functional as F
    k1 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=x.dtype)
    blur = F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), (k1[:, None] * k1[None, :] / 256)[None, None])
    h, w = x.shape[2:]
    return F.interpolate(blur, size=(int(h // 1.2), int(w // 1.2)), mode="bilinear", align_corners=False)


def chain(t, img):
    """(score [B,1,H,W], None) from the folded tensors `t` (weights.fold_keynet): KeyNet.py:116-132."""
    import torch
    import torch.nn.functional as F
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    x = img.sum(1, keepdim=True)
    H, W = x.shape[2:]
    feats = []
    for level in range(3):
        if level:
            x = pyrdown(x)          # of the level before, not of level 0
        dx, dy = spatial_gradient(x)
        dxx, dxy = spatial_gradient(dx)
        dyy = spatial_gradient(dy)[1]
        f = torch.cat([dx, dy, dx * dx, dy * dy, dx * dy, dxy, dxy * dxy, dxx, dyy, dxx * dyy], 1)
        for i in range(3):          # zero padding of the FEATURE maps
            f = F.relu(F.conv2d(f, tt(t["l%d.w" % i]), tt(t["l%d.b" % i]), padding=2))
        feats.append(F.interpolate(f, size=(H, W), mode="bilinear", align_corners=False) if level else f)
    return F.relu(F.conv2d(torch.cat(feats, 1), tt(t["last.w"]), tt(t["last.b"]), padding=2)), None
