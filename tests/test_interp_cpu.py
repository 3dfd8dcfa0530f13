"""csrc/interp.h states torch's three interpolation rules once for every kernel; this pins that one statement against torch itself, on the CPU.

A few lines of host C++ include the header (a host compiler sees plain inline functions), are compiled with the clang of the toolchain build.py finds, with
-ffp-contract=off as the library is, and loaded with ctypes.  Every comparison probes with ONE-HOT sources: the output of F.interpolate / F.grid_sample for
a source that is 1 at one sample and 0 elsewhere IS the weight that sample has, exactly, whatever torch fuses or in which order it adds (every product is
w x 1 or w x 0); the probe evaluates the same one-hot sources through kpb_tap_* / kpb_mix and kpb_grid_taps / kpb_grid_blend.  Equality is exact everywhere:
an index off by one moves a weight to another source sample, a weight off by an ulp shows as itself.

  align_corners=True    every source size in AC_SRC x every destination size in AC_DST (kpb_ac_scale gives the scale, 0 for a destination of one sample)
  align_corners=False   sources HP_SRC, destinations 1, 2, 4, 8 and 32 times as large: the ratios the kernels that use the unclamped rule rely on.  Other
                        ratios are not part of this test: torch evaluates those differently, and Key.Net keeps its own clamped statement and its own tests
  grid_sample           zeros padding, align_corners=True: maps GRID_MAPS, 200 seeded points of [-1.2, 1.2]^2 each plus the four corners, the centre and the
                        points one float step outside -1 and +1"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from keypoint_bench_amd import build

AC_SRC = (1, 2, 3, 5, 8, 15, 20, 60, 80)
AC_DST = (1, 2, 3, 8, 13, 32, 96, 160, 480, 640)
HP_SRC = (1, 2, 3, 4, 5, 8, 15, 20, 60)
HP_TIMES = (1, 2, 4, 8, 32)
GRID_MAPS = ((1, 1), (2, 3), (8, 8), (15, 20), (60, 80))       # (H, W)

PROBE = r"""
#include "interp.h"
// out[k * n_dst + o]: the weight of source sample k in output o of a one-row upsampling (the row axis is 1 -> 1: both its taps are row 0, its weight 0)
extern "C" void probe_up(int align_corners, int n_src, int n_dst, float* out)
{
    const float scale = align_corners ? kpb_ac_scale(n_src, n_dst) : (float)n_src / (float)n_dst;
    const kpb_lin ty = align_corners ? kpb_tap_ac(0, 1, kpb_ac_scale(1, 1)) : kpb_tap_hp(0, 1, 1.0f);
    for (int o = 0; o < n_dst; ++o) {
        const kpb_lin tx = align_corners ? kpb_tap_ac(o, n_src, scale) : kpb_tap_hp(o, n_src, scale);
        for (int k = 0; k < n_src; ++k)
            out[k * n_dst + o] = kpb_mix(k == tx.i0 && ty.i0 == 0, k == tx.i1 && ty.i0 == 0, k == tx.i0 && ty.i1 == 0, k == tx.i1 && ty.i1 == 0, ty.l, tx.l);
    }
}
// out[(y * W + x) * n + p]: the weight of source pixel (y, x) at grid point p
extern "C" void probe_grid(int H, int W, int n, const float* g /*[n][2]: x, y*/, float* out)
{
    for (int p = 0; p < n; ++p) {
        const kpb_grid t = kpb_grid_taps(g[2 * p], g[2 * p + 1], W, H);
        const long long x0 = (long long)t.x0, y0 = (long long)t.y0;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                out[(size_t)(y * W + x) * n + p] = kpb_grid_blend(y == y0 && x == x0, y == y0 && x == x0 + 1, y == y0 + 1 && x == x0, y == y0 + 1 && x == x0 + 1, t.w);
    }
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("interp_probe")
    src, so = str(d / "probe.cpp"), str(d / "probe.so")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call([os.path.join(build.llvm_bin(), "clang++"), "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                           "-I", build.CSRC, "-o", so, src])
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.probe_up.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, fp]
    lib.probe_grid.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, fp, fp]
    lib.probe_up.restype = lib.probe_grid.restype = None
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _up(probe, align_corners, n_src, n_dst):
    """(the header's weights, torch's) of source sample k in output o, both [n_src][n_dst]"""
    got = np.empty((n_src, n_dst), np.float32)
    probe.probe_up(int(align_corners), n_src, n_dst, _ptr(got))
    onehot = torch.eye(n_src, dtype=torch.float32).reshape(n_src, 1, 1, n_src)
    ref = F.interpolate(onehot, size=(1, n_dst), mode="bilinear", align_corners=align_corners)
    return got, ref.reshape(n_src, n_dst).numpy()


def _differing(got, ref):
    return ["source %d output %d: header %r torch %r" % (k, o, got[k, o], ref[k, o]) for k, o in zip(*np.nonzero(got != ref))]


def test_align_corners_true_taps_and_weights_are_torchs(probe):
    bad, n = [], 0
    for n_src in AC_SRC:
        for n_dst in AC_DST:
            got, ref = _up(probe, True, n_src, n_dst)
            n += got.size
            bad += ["%d -> %d %s" % (n_src, n_dst, m) for m in _differing(got, ref)]
    print("align_corners=True: %d weights compared, %d differ" % (n, len(bad)))
    assert not bad, bad[:10]


def test_align_corners_false_taps_and_weights_are_torchs(probe):
    bad, n = [], 0
    for n_src in HP_SRC:
        for times in HP_TIMES:
            got, ref = _up(probe, False, n_src, n_src * times)
            n += got.size
            bad += ["%d -> %d %s" % (n_src, n_src * times, m) for m in _differing(got, ref)]
    print("align_corners=False: %d weights compared, %d differ" % (n, len(bad)))
    assert not bad, bad[:10]


def _grid_points(seed):
    rng = np.random.default_rng(seed)
    one = np.float32(1.0)
    edge = [-np.nextafter(one, np.float32(2.0)), np.nextafter(-one, np.float32(0.0)), np.nextafter(one, np.float32(0.0)), np.nextafter(one, np.float32(2.0))]
    special = [(-1, -1), (1, -1), (-1, 1), (1, 1), (0, 0)] + [(e, 0.25) for e in edge] + [(-0.5, e) for e in edge] + [(e, e) for e in edge]
    return np.concatenate([rng.uniform(-1.2, 1.2, (200, 2)), np.array(special, np.float64)]).astype(np.float32)


@pytest.mark.parametrize("H,W", GRID_MAPS, ids=lambda v: str(v))
def test_grid_sample_weights_are_torchs(probe, H, W):
    g = _grid_points(H * 1000 + W)
    n = len(g)
    got = np.empty((H * W, n), np.float32)
    probe.probe_grid(H, W, n, _ptr(np.ascontiguousarray(g)), _ptr(got))
    onehot = torch.eye(H * W, dtype=torch.float32).reshape(1, H * W, H, W)
    ref = F.grid_sample(onehot, torch.from_numpy(g).reshape(1, 1, n, 2), mode="bilinear", padding_mode="zeros", align_corners=True).reshape(H * W, n).numpy()
    bad = ["pixel (%d, %d) point %r: header %r torch %r" % (c // W, c % W, tuple(g[p]), got[c, p], ref[c, p]) for c, p in zip(*np.nonzero(got != ref))]
    print("grid_sample %d x %d: %d weights compared, %d differ" % (H, W, got.size, len(bad)))
    assert not bad, bad[:10]
    assert got.sum() > 0        # (points inside the map: the comparison is not of zeros alone)
