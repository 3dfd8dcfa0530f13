#!/usr/bin/env python3
"""A/B partner for the kernels whose assembly moved when the interpolation rules went into csrc/interp.h (scripts/kernel_diff.py names them): the heads and
desc_at of ALIKE-l, Key.Net's pyrdown and head, D2-Net's d2_upsample, SFD2's sfd2_score, DISK's disk_desc_at, the tracker's lk_level.  Runs whichever library KPB_LIB_PATH names (default: the tree's
own), one process per library and call, no loop over a GPU step:

    KPB_LIB_PATH=old/libkpb.so python scripts/interp_ab.py dump old.npz      every output of the calls below, as arrays
    KPB_LIB_PATH=old/libkpb.so python scripts/interp_ab.py time old_1.json   per-kernel ms from the context's profile (kpb_prof_report), one JSON line
    python scripts/interp_ab.py compare old.npz new.npz [old_fp32.npz new_fp32.npz] old_1.json new_1.json old_2.json new_2.json ...   the verdict (no GPU)

Under KPB_FP32_MATRIX=1 (read once per process) the same two modes reach the strict-fp32 forms that moved, ALIKE-l's head and DISK's desc_at: those two nets alone then.

dump.  Each net at the shapes of tests/alike_family_shapes.py -- (96, 32), (160, 32), (32, 288), (224, 96), (96, 224): the 1/32 maps are one row or one column
there -- batch 2, its full score and descriptor maps; ALIKE-l and DISK (at the shapes it accepts) also keypoint-only (score alone) and kpb_net_desc_at at 300
points per image: the four corners, both sides just outside the map, exact integer positions and seeded positions in [-0.02, 1.02]^2.  The tracker
(utils/matcher.py OpticalFlow, 5 x 5 window, 2 levels, 10 iterations, seeded start angles) follows the same 300 points between the two images of each shape.
time.  640 x 480, 32 images (2 x 16, as the rate scripts batch them: ALIKE-l's dense map of 512 images would be 80 GB, and at 32 every kernel here still
fills the chip), desc_at at top_k = 1000 points per image, the tracker on one pair at 1000 points with the configured 21 x 21 window, 3 levels, 40 iterations:
one warm-up call, then 10 profiled calls (3 left the 36 us d2_upsample to the timer's noise), ms per call of every kernel of TIMED.
compare.  Every array of the two dumps must be numpy.array_equal (NaNs in the same places count as equal).  Per kernel the rounds alternate old, new, ...
(five each at least): the new library's median must not lie above the old library's own rounds (their minimum and maximum are printed: the spread is
measured, not assumed).  Exit status 1 if an array differs or a kernel is slower than that.  Record: profiles/interp_ab.txt"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
DEV = "cuda:0"
FP32 = os.environ.get("KPB_FP32_MATRIX") == "1"
H, W, IMAGES, TOP_K = 480, 640, 32, 1000
TIMED = {"alike_l": ("alikel_head_dense", "alikel_head_score", "alikel_desc_at"), "keynet": ("keynet_pyrdown", "keynet_head"), "d2net": ("d2_upsample",),
         "sfd2": ("sfd2_score",), "disk": ("disk_desc_at",), "lk": ("lk_level",)}
LK_DUMP = dict(distance=3, win_size=5, levels=2, interation=10, gray=False)
LK_TIME = dict(distance=10, win_size=21, levels=3, interation=40, gray=False)      # config_fund.yaml's optical_flow_params


def nets():
    """name -> net, built on first use"""
    def alike_l():
        from alike_l_fixtures import state_dict
        from keypoint_bench_amd.models.ALike import ALNet
        net = ALNet()
        net.load_state_dict(state_dict())
        return net

    def keynet():
        import keynet_fixtures
        from keypoint_bench_amd.models.KeyNet import KeyNet
        net = KeyNet(keynet_fixtures.PLAN)
        net.load_state_dict(keynet_fixtures.checkpoint())
        return net

    def d2net():
        from keypoint_bench_amd.models.D2_Net import d2net_random
        return d2net_random(0)

    def sfd2():
        from keypoint_bench_amd.models.sfd2 import sfd2_random
        return sfd2_random(0)

    def disk():
        from keypoint_bench_amd.models.disk import disk_random
        return disk_random(5)

    made = {"alike_l": alike_l, "disk": disk} if FP32 else {"alike_l": alike_l, "keynet": keynet, "d2net": d2net, "sfd2": sfd2, "disk": disk}
    return {k: f().eval() for k, f in made.items()}


def points(B, n, shape, seed):
    """[B][n][2] normalised (x, y) as kpb_sample takes them: pixel = p * (size - 1)"""
    import numpy as np
    h, w = shape
    rng = np.random.default_rng(seed)
    eps = 1e-3
    fixed = [(0, 0), (1, 0), (0, 1), (1, 1), (-eps, 0.5), (1 + eps, 0.5), (0.5, -eps), (0.5, 1 + eps), (-eps, -eps), (1 + eps, 1 + eps), (-1.5 / (w - 1), 0.3), (0.3, 1 + 1.5 / (h - 1))]
    fixed += [(x / (w - 1), y / (h - 1)) for x in (0, 1, w // 2, w - 2, w - 1) for y in (0, 1, h // 2, h - 2, h - 1)]
    p = np.concatenate([np.array(fixed, np.float64), rng.uniform(-0.02, 1.02, (n - len(fixed), 2))]).astype(np.float32)
    return np.stack([p, p[::-1]][:B] if B <= 2 else [np.roll(p, i, 0) for i in range(B)])


def desc_at(net, pts):
    """kpb_net_desc_at on the features of the net's last forward: pts [B][n][2] on the device -> [B][n][dim]"""
    import torch
    from keypoint_bench_amd._lib import ptr
    out = torch.empty(pts.shape[:2] + (net.dim,), dtype=torch.float32, device=pts.device)
    net._ctx.check(net._ctx.lib.kpb_net_desc_at(net._handles[0], ptr(pts), 2, pts.shape[1], ptr(None), ptr(out)))
    return out


def track(img1, img2, pts, params, seed):
    """OpticalFlow(params) from img1 [3][H][W] into img2 at pts [n][2] (normalised), seeded start angles: (points [n][2], error [n])"""
    import torch
    from keypoint_bench_amd.utils.matcher import OpticalFlow
    angle = torch.rand(pts.shape[0], generator=torch.Generator().manual_seed(seed)).to(pts.device) * 6.28
    out, err = OpticalFlow(params)(img1[None], img2[None], pts, pts, random_angle=angle)
    return out[0], err[0]


def dump(path):
    import numpy as np
    import torch
    from alike_family_shapes import SHAPES, images
    arrays = {}
    for name, net in nets().items():
        for shape in SHAPES:
            if name == "disk" and (shape[0] % 16 or shape[1] % 16 or shape == (16, 16)):
                continue
            x = torch.from_numpy(images(2, shape)).to(DEV)
            tag = "%s.%dx%d." % ((name,) + shape)
            score, desc = net._run(x, name != "keynet")
            arrays[tag + "score"] = score.cpu().numpy()
            if desc is not None:
                arrays[tag + "desc"] = desc.cpu().numpy()
            if name in ("alike_l", "disk"):
                arrays[tag + "score_only"] = net._run(x, False)[0].cpu().numpy()
                arrays[tag + "desc_at"] = desc_at(net, torch.from_numpy(points(2, 300, shape, shape[0] + shape[1])).to(DEV)).cpu().numpy()
    for shape in ([] if FP32 else SHAPES):
        x = torch.from_numpy(images(2, shape)).to(DEV)
        pts, err = track(x[0], x[1], torch.from_numpy(points(1, 300, shape, shape[0] + shape[1])[0]).to(DEV), LK_DUMP, shape[0])
        arrays["lk.%dx%d.pts" % shape], arrays["lk.%dx%d.err" % shape] = pts.cpu().numpy(), err.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(path, **arrays)
    print(json.dumps({"lib": os.environ.get("KPB_LIB_PATH") or "tree", "fp32": FP32, "arrays": len(arrays), "file": path}))


def time_(path, reps=10):
    import numpy as np
    import torch
    from keypoint_bench_amd import _lib, synthetic
    v = [synthetic.image_pair(5000 + i, H, W) for i in range(IMAGES // 2)]
    x = torch.from_numpy(np.concatenate([np.stack([a for a, _ in v]), np.stack([b for _, b in v])])).to(DEV)
    pts = torch.from_numpy(points(IMAGES, TOP_K, (H, W), 7)).to(DEV)
    ctx = _lib.Context.get(torch.device(DEV))
    res = {"lib": os.environ.get("KPB_LIB_PATH") or "tree", "fp32": FP32, "images": IMAGES, "reps": reps, "ms": {}}
    calls = dict(nets()) if FP32 else dict(nets(), lk=None)
    for name, net in calls.items():
        def call():
            if name == "lk":
                return track(x[0], x[IMAGES // 2], pts[0], LK_TIME, 7)
            net._run(x, name != "keynet")
            if name in ("alike_l", "disk"):
                net._run(x, False)
                desc_at(net, pts)
        call()
        torch.cuda.synchronize()
        ctx.prof_enable(True)
        try:
            ctx.prof_report()
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
            rep = ctx.prof_report()
        finally:
            ctx.prof_enable(False)
        for k in TIMED[name]:
            res["ms"][k + (".fp32" if FP32 else "")] = round(rep[k][1] / reps, 5)
    line = json.dumps(res)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


def compare(files):
    import numpy as np
    dumps, times = [f for f in files if f.endswith(".npz")], [f for f in files if f.endswith(".json")]      # each in the order old, new, old, new, ...
    differ = []
    for old, new in zip(dumps[0::2], dumps[1::2]):
        a, b = np.load(old), np.load(new)
        keys = sorted(set(a.files) | set(b.files))
        d = [k for k in keys if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k], equal_nan=True)]
        print("dumps %s / %s: %d and %d arrays; arrays that differ: %d %s" % (old, new, len(a.files), len(b.files), len(d), ", ".join(d[:40])))
        differ += d
    print("verdict: %s" % ("DIFFER" if differ else "BIT-EQUAL"))
    ms = {}
    for i, path in enumerate(times):        # rounds alternate old, new
        with open(path) as f:
            for k, v in json.load(f)["ms"].items():
                ms.setdefault(k, ([], []))[i % 2].append(v)
    print("\nms per call from kpb_prof_report (640 x 480, %d images, desc_at at %d points per image), rounds in run order" % (IMAGES, TOP_K))
    slower = []
    for k, (old, new) in sorted(ms.items()):
        med = float(np.median(new))
        ok = med <= max(old)
        slower += [] if ok else [k]
        print("%-24s old %s\n%-24s new %s\n%-24s old min %.5f median %.5f max %.5f | new median %.5f  %s"
              % (k, " ".join("%.5f" % v for v in old), "", " ".join("%.5f" % v for v in new), "", min(old), float(np.median(old)), max(old), med,
                 "within the old rounds" if ok else "SLOWER"))
    sys.exit(1 if differ or slower else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["dump", "time", "compare"])
    ap.add_argument("files", nargs="+")
    args = ap.parse_args()
    if args.mode == "compare":
        compare(args.files)
    else:
        {"dump": dump, "time": time_}[args.mode](args.files[0])


if __name__ == "__main__":
    main()
