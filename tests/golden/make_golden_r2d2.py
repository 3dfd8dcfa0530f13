#!/usr/bin/env python3
"""Golden fixtures for R2D2 from the REFERENCE class (models/r2d2.py, Quad_L2Net_ConfCFS) and the checkpoint its tree ships
(weights/r2d2_WASF_N16.pt, README row "R2D2"): the checkpoint's tensors as arrays, and the reference's fp32 CPU outputs on
synthetic.image_pair(0, H, W) at four shapes.  Build container only; a no-op without the reference checkout.

New committed files are held to 1 MiB each (the older, larger fixtures predate that limit), and a 128-channel full-resolution map passes it: the arrays are cut into pieces along their first axis and
dealt over r2d2.npz, r2d2.1.npz, ... (and r2d2_state_dict*.npz); tests/r2d2_fixtures.py puts them together again.
"""
import importlib.util
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIMIT = 1000000         # bytes of array data per file: the .npz stays below 1 MiB with its headers
SHAPES = ((64, 96), (61, 97), (24, 40), (480, 640))     # even, odd, smaller than the largest dilation's reach, the benchmark's


def save_parts(stem, arrays):
    """arrays: name -> ndarray.  Pieces `name@i` (rows of the first axis) are packed first-fit into stem.npz, stem.1.npz, ..."""
    pieces = []
    for name, a in arrays.items():
        a = np.asarray(a)
        if a.nbytes <= LIMIT // 2 or a.ndim == 0:
            pieces.append((name, a))
            continue
        rows = max(1, (LIMIT // 2) // (a.nbytes // a.shape[0]))
        assert a.nbytes // a.shape[0] <= LIMIT, name
        for i, r0 in enumerate(range(0, a.shape[0], rows)):
            pieces.append(("%s@%d" % (name, i), a[r0:r0 + rows]))
    files = []
    for name, a in pieces:
        for f in files:
            if f["bytes"] + a.nbytes <= LIMIT:
                break
        else:
            f = {"bytes": 0, "arrays": {}}
            files.append(f)
        f["arrays"][name] = a
        f["bytes"] += a.nbytes
    for old in os.listdir(HERE):
        if old == stem + ".npz" or (old.startswith(stem + ".") and old.endswith(".npz") and old[len(stem) + 1:-4].isdigit()):
            os.remove(os.path.join(HERE, old))
    for i, f in enumerate(files):
        path = os.path.join(HERE, stem + (".npz" if i == 0 else ".%d.npz" % i))
        np.savez(path, **f["arrays"])
        assert os.path.getsize(path) < (1 << 20), path
    print("  %s: %d file(s)" % (stem, len(files)))


def main():
    if not os.path.isdir(REF):
        print("reference checkout not present; nothing to do")
        return 0
    import torch
    sys.path.insert(0, ROOT)
    from keypoint_bench_amd import synthetic
    spec = importlib.util.spec_from_file_location("ref_r2d2", os.path.join(REF, "models", "r2d2.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    ck = torch.load(os.path.join(REF, "weights", "r2d2_WASF_N16.pt"), map_location="cpu", weights_only=False)
    net = getattr(ref, ck["net"].rstrip("()"))()
    print("  r2d2", ck["net"], net.load_state_dict({k.replace("module.", ""): v for k, v in ck["state_dict"].items()}))
    net.eval()
    sd = {k: v.numpy() for k, v in ck["state_dict"].items() if not k.endswith("num_batches_tracked")}
    sd["net"] = np.array(ck["net"])
    save_parts("r2d2_state_dict", sd)
    torch.set_num_threads(8)
    out = {}
    with torch.no_grad():
        for H, W in SHAPES:
            v0, _ = synthetic.image_pair(0, H, W)
            score, desc = net(torch.from_numpy(v0)[None])
            tag = "%dx%d" % (H, W)
            out[tag + ".img.sum"] = np.array(synthetic.checksum(v0))
            out[tag + ".score"] = score[0, 0].numpy()
            # [H, W, 128] rows (the pieces are cut along H); the benchmark shape keeps every eighth row and column
            d = desc[0].permute(1, 2, 0).contiguous().numpy()
            out[tag + ".desc"] = d if H < 480 else np.ascontiguousarray(d[::8, ::8])
            print("  r2d2", tag, tuple(score.shape), tuple(desc.shape), float(score.min()), float(score.max()))
    save_parts("r2d2", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
