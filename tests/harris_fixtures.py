"""What the Harris tests share: the numpy oracle of the response csrc/harris.hip computes ("The definition"), the shape list and the
image makers.

The oracle is the definition itself: every step before the last line is an integer (int64 arrays), the last line is float64 with one IEEE operation per
numpy operation, so the device must agree with it BIT FOR BIT -- there is no tolerance anywhere in these tests."""
import numpy as np

from keypoint_bench_amd import synthetic

TILE = (32, 64)                 # HR_TH, HR_TW of csrc/harris.hip (tests/test_harris_cpu.py reads them back from the source)
CONFIG_PLAN = (5, 3, 0.04)      # Harris_params of the reference's configs: block_size, ksize, k
BLOCK_SIZES = (2, 3, 5, 6)
KS = (0.04, 0.06)
SMALL = [(8, 8), (9, 13), (37, 61), (96, 160), (TILE[0] + 1, TILE[1] + 1), (TILE[0] - 1, TILE[1] - 1)]      # smallest; below one tile and odd; odd; several tiles; tile + 1; tile - 1
LARGE = (480, 640)
KINDS = ("frames", "thirds", "constant", "ramp", "negative", "blocks")
DX_MAX = 4 * 255                # |dx|, |dy| <= 1020


# ------------------------------------------------------------------------------------------------ the definition
def gray_plane(img):
    """[3, H, W] float32 -> int64 [H, W] in 0 .. 255: ((c0 + c1) + c2) * 255 in float32, truncated toward zero, low 8 bits."""
    x = np.asarray(img, np.float32)
    g = ((x[0] + x[1]) + x[2]) * np.float32(255.0)
    assert g.dtype == np.float32
    return g.astype(np.int64) & 255


def sobel(g):
    """Un-scaled 3 x 3 Sobel pair of an int64 plane over reflect-101 (numpy's 'reflect')."""
    p = np.pad(np.asarray(g, np.int64), 1, mode="reflect")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return dx, dy


def box_sum(plane, b):
    """Sum over rows [y - b // 2, y - b // 2 + b - 1] and the same columns, the PLANE extended by reflect-101."""
    a = b // 2
    H, W = plane.shape
    p = np.pad(np.asarray(plane, np.int64), ((a, b - 1 - a), (a, b - 1 - a)), mode="reflect")
    out = np.zeros((H, W), np.int64)
    for i in range(b):
        for j in range(b):
            out += p[i:i + H, j:j + W]
    return out


def structure_tensor(g, b):
    dx, dy = sobel(g)
    return box_sum(dx * dx, b), box_sum(dx * dy, b), box_sum(dy * dy, b)


def response64(g, b, k):
    """The float64 value before the final rounding: ((double)det - (double)float32(k) * (double)t2) * s4."""
    A, B, C = structure_tensor(g, b)
    det = A * C - B * B
    t2 = (A + C) * (A + C)
    assert max(int(np.abs(det).max()), int(t2.max())) < 2 ** 53
    k32 = np.float64(np.float32(k))
    s = np.float64(1.0) / (np.float64(4.0) * np.float64(b) * np.float64(255.0))
    s4 = (s * s) * (s * s)
    return (det.astype(np.float64) - k32 * t2.astype(np.float64)) * s4


def harris_oracle(img, block_size, k):
    """img [3, H, W] float32 -> the score map float32 [H, W]."""
    return response64(gray_plane(img), block_size, k).astype(np.float32)


# ------------------------------------------------------------------------------------------------ images
def ramp(H, W):
    """Channel 0 = v / 255 in float32 for v = 0 .. 255 in raster order (repeated), the others zero: what a decoded image's bytes look like (every one of
    them comes back as v: tests/test_harris_cpu.py)."""
    v = (np.arange(H * W) % 256).astype(np.float32).reshape(H, W)
    x = np.zeros((3, H, W), np.float32)
    x[0] = v / np.float32(255.0)
    return x


def stripes(H, W, transpose=False):
    """Two-pixel stripes of 0 / 255 gray bytes (channel 0 = byte / 255, which comes back exactly for 0 and 255): |dx| = 1020 at every pixel off the frame's edge, so A reaches
    its bound b^2 1 040 400.  (A one-pixel checkerboard would not do: the Sobel's taps two columns apart see equal values there and every gradient is 0.)"""
    y, x = np.mgrid[0:H, 0:W]
    on = ((y if transpose else x) >> 1) & 1
    out = np.zeros((3, H, W), np.float32)
    out[0] = on.astype(np.float32)
    return out


def image(kind, H, W, seed=0):
    if kind == "frames":        # channel sums up to 3: the gray cast wraps, as under the configs' gray: false
        return synthetic.image_pair(seed, H, W)[seed & 1]
    if kind == "thirds":        # nothing wraps
        return (synthetic.image_pair(seed, H, W)[seed & 1] / np.float32(3.0)).astype(np.float32)
    if kind == "constant":
        return np.full((3, H, W), 0.3, np.float32)
    if kind == "ramp":
        return ramp(H, W)
    if kind == "negative":      # sums in about (-1.5, 1.5): negative ones wrap from 256 down
        return (synthetic.image_pair(seed, H, W)[seed & 1] - np.float32(0.5)).astype(np.float32)
    if kind == "blocks":        # 12-pixel squares under a little texture, nothing wraps: long edges (negative response) and square corners (positive)
        y, x = np.mgrid[0:H, 0:W]
        sq = (((y // 12) + (x // 12)) & 1).astype(np.float32) * np.float32(0.2)
        return (synthetic.image_pair(seed, H, W)[seed & 1] * np.float32(0.1) + sq[None]).astype(np.float32)
    raise KeyError(kind)
