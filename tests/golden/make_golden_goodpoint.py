#!/usr/bin/env python3
"""Golden fixtures for GoodPoint from the REFERENCE class (models/GoodPoint.py, plan c0 = 3 / c1 = 8 of the configs) and the checkpoint its tree
ships (weights/goodpoint.pth):
  goodpoint_state_dict.npz   the checkpoint's tensors (without num_batches_tracked);
  goodpoint*.npz             the reference's fp32 CPU outputs -- the sigmoid score [H, W] and the 3-channel map [H, W, 3] -- on
                             synthetic.image_pair(0, H, W)[0] at five shapes, with the image checksum;
  goodpoint_track.npz        the tracking chain at 96 x 128 on synthetic.image_pair(300, 96, 128): the reference's maps of both views, 200 keypoints of
                             view 0 (oracle.detection on the reference's score: nms_dist 2, border_dist 12, top_k 200), seeded angles as
                             make_golden_lk.py stores them, and for two parameter sets (the class defaults; config_fund.yaml's 10 / 21 / 3 / 40) the
                             reference OpticalFlow's outputs and errors ON THE MAPS, with a `stable` flag per point by make_golden_lk_edges.py's rule:
                             the reference re-run with np.nextafter(map 2, 2) agrees within STABLE_PX.  At most CAP_PERCENT of a case's points may be
                             unstable; a case over the cap gets another point seed, never another cap.
Build container only; a no-op without the reference checkout.  Files stay under 1 MiB each (make_golden_r2d2.save_parts; tests/goodpoint_fixtures.py
joins the pieces again).
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SHAPES = ((32, 32), (32, 64), (64, 96), (96, 160), (480, 640))
PARAM = {"c0": 3, "c1": 8}
TRACK_PAIR = (300, 96, 128)
TRACK_DETECT = dict(nms_dist=2, threshold=0.0, border_dist=12, top_k=200, min_score=0.0)
TRACK_SETS = (("defaults", 2100, dict(distance=3, win_size=3, levels=1, interation=40, gray=False)),
              ("fund", 2101, dict(distance=10, win_size=21, levels=3, interation=40, gray=False)))
STABLE_PX = 2e-5
CAP_PERCENT = 5


def main():
    if not os.path.isdir(REF):
        print("reference checkout not present; nothing to do")
        return 0
    sys.dont_write_bytecode = True
    import torch
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import oracle
    from keypoint_bench_amd import synthetic
    from make_golden_r2d2 import save_parts
    # the two torchvision conv factories the reference model uses, as tests/golden/make_golden.py stands them in
    tv, tvm, tvr = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.models.resnet")
    tvr.conv3x3 = lambda i, o, stride=1, groups=1, dilation=1: nn.Conv2d(i, o, 3, stride, dilation, dilation, groups, False)
    tvr.conv1x1 = lambda i, o, stride=1: nn.Conv2d(i, o, 1, stride, bias=False)
    tv.models, tvm.resnet = tvm, tvr
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.models.resnet": tvr})
    spec = importlib.util.spec_from_file_location("ref_goodpoint", os.path.join(REF, "models", "GoodPoint.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    # the reference's tracker (utils/matcher.py imports cv2 and skimage at module level: blank modules, as make_golden_lk_edges.py)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sk = types.ModuleType("skimage"); skf = types.ModuleType("skimage.feature"); skf.match_descriptors = None
    sys.modules.setdefault("skimage", sk); sys.modules.setdefault("skimage.feature", skf)
    mspec = importlib.util.spec_from_file_location("ref_matcher", os.path.join(REF, "utils", "matcher.py"))
    M = importlib.util.module_from_spec(mspec)
    mspec.loader.exec_module(M)

    sd = torch.load(os.path.join(REF, "weights", "goodpoint.pth"), map_location="cpu")
    net = ref.GoodPoint(PARAM)
    print("  goodpoint", net.load_state_dict(sd))
    net.eval()
    save_parts("goodpoint_state_dict", {k: v.numpy() for k, v in sd.items() if not k.endswith("num_batches_tracked")})
    torch.set_num_threads(8)
    out = {}
    with torch.no_grad():
        for H, W in SHAPES:
            v0, _ = synthetic.image_pair(0, H, W)
            score, desc = net(torch.from_numpy(v0)[None])
            tag = "%dx%d" % (H, W)
            out[tag + ".img.sum"] = np.array(synthetic.checksum(v0))
            out[tag + ".score"] = score[0, 0].numpy()
            out[tag + ".desc"] = desc[0].permute(1, 2, 0).contiguous().numpy()
            print("  goodpoint", tag, tuple(score.shape), tuple(desc.shape), float(score.min()), float(score.max()), float(desc.min()), float(desc.max()))
    save_parts("goodpoint", out)

    # ---- the tracking chain
    seed, H, W = TRACK_PAIR
    v0, v1 = synthetic.image_pair(seed, H, W)
    with torch.no_grad():
        s0, d0 = net(torch.from_numpy(v0)[None])
        _, d1 = net(torch.from_numpy(v1)[None])
    m0, m1 = d0[0].contiguous().numpy(), d1[0].contiguous().numpy()      # planar [3, H, W]
    kps, _ = oracle.detection(s0[0, 0].numpy(), TRACK_DETECT)
    n = kps.shape[0]
    assert n == 200, n
    pts = np.ascontiguousarray(kps[:, :2])
    tr = {"image_pair": np.array(TRACK_PAIR, np.int64), "img0.sum": np.array(synthetic.checksum(v0)), "img1.sum": np.array(synthetic.checksum(v1)),
          "map0": m0, "map1": m1, "kps": kps, "names": np.array([t[0] for t in TRACK_SETS])}

    def reference(prm, a, b, aseed):
        torch.manual_seed(aseed)
        p, err = M.OpticalFlow(prm)(torch.from_numpy(a)[None], torch.from_numpy(b)[None], torch.from_numpy(pts.copy()), torch.from_numpy(pts.copy()))
        return p[0].numpy(), err[0].numpy()

    for name, aseed, prm in TRACK_SETS:
        torch.manual_seed(aseed)
        angle = torch.randn(n) * 6.28                            # what OpticalFlow.__call__ draws first (matcher.py:55)
        p, err = reference(prm, m0, m1, aseed)
        q, _ = reference(prm, m0, np.nextafter(m1, np.float32(2)), aseed)
        stable = np.abs(p - q).max(1) <= STABLE_PX
        unstable = int((~stable).sum())
        print("  goodpoint track %s: %d of %d points unstable, mean error %.3f px" % (name, unstable, n, float(err.mean())))
        assert 100 * unstable <= CAP_PERCENT * n, "%s: %d of %d points are unstable; change its point seed" % (name, unstable, n)
        k = name + "_"
        tr[k + "angle"] = angle.numpy()
        tr[k + "prm"] = np.array([prm["distance"], prm["win_size"], prm["levels"], prm["interation"]], np.int64)
        tr[k + "out"], tr[k + "err"], tr[k + "stable"] = p, err, stable
    save_parts("goodpoint_track", tr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
