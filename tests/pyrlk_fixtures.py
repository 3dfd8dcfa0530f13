"""What the PyrLK tests share: the numpy oracle of "PyrLK-R" ("The definition"), the tracker csrc/pyrlk.hip computes in place of
cv2.calcOpticalFlowPyrLK as the reference's optical_flow_cv calls it (utils/matcher.py:145-185), the image makers and the point sets.

The oracle is the definition itself.  Everything up to the 2 x 2 system is integer arithmetic (int64 arrays); the window sums are exact Python / int64 integers
rounded to float32 ONCE; every float32 step after that is one numpy operation on np.float32 scalars, hence one IEEE operation.  So the device must agree with
it BIT FOR BIT -- there is no tolerance in the device tests.  Parity with cv2's own bits is NOT pinned (OpenCV is absent here): cv2 adds the window sums in
float32 in an order its SIMD build decides; the exact sum lies inside that spread."""
import numpy as np

F32 = np.float32
W_BITS = 14
FLT_SCALE = F32(1.0) / F32(1 << 20)
FLT_EPSILON = F32(np.finfo(np.float32).eps)
MIN_EIG = 1e-4                  # minEigThreshold
MAX_COUNT, EPSILON = 10, 0.03   # criteria = (COUNT | EPS, 10, 0.03)
DEFAULTS = {"win_size": 15, "levels": 3}        # matcher.py:158-162


# ------------------------------------------------------------------------------------------------ 1. input bytes, 2. pyramid, 3. derivatives
def to_bytes(img):
    """[C, H, W] float32 -> int64 [C, H, W] in 0 .. 255: x * 255 in float32, truncated toward zero, low 8 bits (harris_fixtures.gray_plane without the channel sum)."""
    x = np.asarray(img, np.float32) * F32(255.0)
    assert x.dtype == np.float32
    return x.astype(np.int64) & 255


def pyr_down(g):
    """cv::pyrDown of an int64 plane [H, W]: ((H + 1) // 2, (W + 1) // 2), separable 1-4-6-4-1 over reflect-101, (sum + 128) >> 8, output (y, x) centred on (2y, 2x)."""
    H, W = g.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    p = np.pad(np.asarray(g, np.int64), 2, mode="reflect")
    k = (1, 4, 6, 4, 1)
    rows = sum(k[a] * p[a:a + 2 * Ho:2, :] for a in range(5))           # rows 2y + a - 2 of the plane
    out = sum(k[b] * rows[:, b:b + 2 * Wo:2] for b in range(5))
    return (out + 128) >> 8


def level_sizes(H, W, win, levels):
    """[(H_l, W_l)] for the levels that are built: a level that would not be larger than the window both ways is not (nor is any above it)."""
    sizes = [(H, W)]
    while len(sizes) <= levels:
        nh, nw = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if nw <= win or nh <= win:
            break
        sizes.append((nh, nw))
    return sizes


def pyramid(planes, win, levels):
    """planes int64 [C, H, W] -> list over the levels of int64 [C, H_l, W_l]."""
    C, H, W = planes.shape
    out = [np.asarray(planes, np.int64)]
    for _ in level_sizes(H, W, win, levels)[1:]:
        out.append(np.stack([pyr_down(out[-1][c]) for c in range(C)]))
    return out


def scharr(g):
    """int64 (dx, dy) of a plane over reflect-101: dx = S(x + 1) - S(x - 1) with S the vertical 3-10-3 smooth; dy = the horizontal 3-10-3 smooth of row (y + 1) - row (y - 1)."""
    p = np.pad(np.asarray(g, np.int64), 1, mode="reflect")
    S = 3 * p[:-2, :] + 10 * p[1:-1, :] + 3 * p[2:, :]
    D = p[2:, :] - p[:-2, :]
    return S[:, 2:] - S[:, :-2], 3 * D[:, :-2] + 10 * D[:, 1:-1] + 3 * D[:, 2:]


# ------------------------------------------------------------------------------------------------ 4. the tracker
def _weights(px, py, fx, fy):
    a, b = px - fx, py - fy                     # float32
    one, s = F32(1.0), F32(1 << W_BITS)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _in_range(fx, fy, win, W, H):
    return bool(fx >= -win and fx < W and fy >= -win and fy < H)       # a NaN fails


def _window(pad, iy, ix, win, w, shift):
    """DESCALE(sum of the four taps * weights, shift) on planes padded by `win` on every side: int64 [C, win, win]."""
    y, x = iy + win, ix + win
    t = (pad[:, y:y + win, x:x + win] * w[0] + pad[:, y:y + win, x + 1:x + win + 1] * w[1]
         + pad[:, y + 1:y + win + 1, x:x + win] * w[2] + pad[:, y + 1:y + win + 1, x + 1:x + win + 1] * w[3])
    return (t + (1 << (shift - 1))) >> shift


def _f32_of_int(v):
    v = int(v)
    assert abs(v) < 2 ** 53             # a float64 holds it exactly, so the one rounding is the one to float32
    return F32(float(v))


class Prepared:
    """The pyramids of one pair: per level the reflect-101-padded planes of both images and the zero-padded derivatives of image 1, each padded by `win`."""

    def __init__(self, img1, img2, win, levels):
        b1, b2 = to_bytes(img1), to_bytes(img2)
        assert b1.shape == b2.shape and b1.shape[0] in (1, 3) and win % 2 == 1 and 3 <= win <= 31 and 0 <= levels <= 4
        assert b1.shape[1] > win and b1.shape[2] > win
        self.win, self.H, self.W = win, b1.shape[1], b1.shape[2]
        p1, p2 = pyramid(b1, win, levels), pyramid(b2, win, levels)
        self.sizes = [p.shape[1:] for p in p1]
        self.top = len(p1) - 1
        pw = ((0, 0), (win, win), (win, win))
        self.I = [np.pad(p, pw, mode="reflect") for p in p1]
        self.J = [np.pad(p, pw, mode="reflect") for p in p2]
        d = [[scharr(p[c]) for c in range(p.shape[0])] for p in p1]
        self.dx = [np.pad(np.stack([dc[0] for dc in dl]), pw) for dl in d]
        self.dy = [np.pad(np.stack([dc[1] for dc in dl]), pw) for dl in d]
        assert all(int(np.abs(a).max()) <= 4080 for a in self.dx + self.dy)


def track_point(pp, prev_xy, next_xy):
    """One point through the levels: (carried x, carried y, status) in level-0 pixels.  prev_xy / next_xy: float32 pixel positions, finite."""
    win = pp.win
    half = F32(win - 1) * F32(0.5)
    cx, cy, status = F32(next_xy[0]), F32(next_xy[1]), 1
    for level in range(pp.top, -1, -1):
        H, W = pp.sizes[level]
        scale = F32(1.0) / F32(1 << level)
        px, py = F32(prev_xy[0]) * scale - half, F32(prev_xy[1]) * scale - half
        if level == pp.top:
            cx, cy = cx * scale, cy * scale
        else:
            cx, cy = cx * F32(2.0), cy * F32(2.0)
        fx, fy = np.floor(px), np.floor(py)
        if not _in_range(fx, fy, win, W, H):
            if level == 0:
                status = 0
            continue
        w = _weights(px, py, fx, fy)
        I = _window(pp.I[level], int(fy), int(fx), win, w, W_BITS - 5)
        Ix = _window(pp.dx[level], int(fy), int(fx), win, w, W_BITS)
        Iy = _window(pp.dy[level], int(fy), int(fx), win, w, W_BITS)
        A11, A12, A22 = (_f32_of_int((Ix * Ix).sum()) * FLT_SCALE, _f32_of_int((Ix * Iy).sum()) * FLT_SCALE, _f32_of_int((Iy * Iy).sum()) * FLT_SCALE)
        D = A11 * A22 - A12 * A12
        dif = A11 - A22
        min_eig = ((A22 + A11) - np.sqrt(dif * dif + (F32(4.0) * A12) * A12)) / F32(2 * win * win)
        assert D.dtype == np.float32 and min_eig.dtype == np.float32
        if float(min_eig) < MIN_EIG or D < FLT_EPSILON:
            if level == 0:
                status = 0
            continue
        D = F32(1.0) / D
        nx, ny = cx - half, cy - half
        pdx = pdy = F32(0.0)
        for j in range(MAX_COUNT):
            fx, fy = np.floor(nx), np.floor(ny)
            if not _in_range(fx, fy, win, W, H):
                if level == 0:
                    status = 0
                break
            w = _weights(nx, ny, fx, fy)
            diff = _window(pp.J[level], int(fy), int(fx), win, w, W_BITS - 5) - I
            b1, b2 = _f32_of_int((diff * Ix).sum()) * FLT_SCALE, _f32_of_int((diff * Iy).sum()) * FLT_SCALE
            dx, dy = (A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D
            assert dx.dtype == np.float32
            nx, ny = nx + dx, ny + dy
            cx, cy = nx + half, ny + half
            if float(dx) * float(dx) + float(dy) * float(dy) <= EPSILON * EPSILON:
                break
            if j > 0 and abs(float(dx + pdx)) < 0.01 and abs(float(dy + pdy)) < 0.01:
                cx, cy = cx - dx * F32(0.5), cy - dy * F32(0.5)
                break
            pdx, pdy = dx, dy
    if status == 1 and not _in_range(np.floor(cx - half), np.floor(cy - half), win, pp.W, pp.H):
        status = 0
    return cx, cy, status


def pixels(pts, H, W):
    """Normalised [n, >= 2] -> float32 pixel positions [n, 2]: pt * (W - 1, H - 1) in float32."""
    p = np.asarray(pts, np.float32)[:, :2]
    return p * np.array([W - 1, H - 1], np.float32)


def track_pixels(img1, img2, pts1, pts2, win, levels, prepared=None):
    """(carried pixels float32 [n, 2], status uint8 [n], finite bool [n]): rows that are not finite are left as NaN with status 0."""
    pp = prepared or Prepared(img1, img2, win, levels)
    a, b = pixels(pts1, pp.H, pp.W), pixels(pts2, pp.H, pp.W)
    n = a.shape[0]
    out, status = np.full((n, 2), np.nan, np.float32), np.zeros((n,), np.uint8)
    finite = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in np.nonzero(finite)[0]:
            out[i, 0], out[i, 1], status[i] = track_point(pp, a[i], b[i])
    return out, status, finite


def pyrlk_oracle(img1, img2, pts1, pts2, win=15, levels=3, prepared=None):
    """img1 / img2 [C, H, W] float32, pts1 / pts2 [n, >= 2] normalised -> (points float32 [n, 2] normalised, status uint8 [n]).  A row whose point or guess is not
    finite comes back as given, status 0."""
    H, W = np.asarray(img1).shape[1:]
    px, status, finite = track_pixels(img1, img2, pts1, pts2, win, levels, prepared)
    out = px / np.array([W - 1, H - 1], np.float32)
    assert out.dtype == np.float32
    out[~finite] = np.asarray(pts2, np.float32)[~finite, :2]
    return out, status


# ------------------------------------------------------------------------------------------------ images and points
def shifted_pair(seed, H=120, W=160, shift=(2, 3), C=3, margin=16):
    """A pair cut from one 5 x 5-box-blurred noise canvas: image 2 shows the scene of image 1 moved by shift = (dx, dy) px, i.e. the point at p in image 1
    is at p + shift in image 2.  float32 [C, H, W] in [0, 1]."""
    rng = np.random.default_rng(seed)
    hh, ww = H + 2 * margin, W + 2 * margin
    canvas = rng.random((C, hh + 4, ww + 4))
    blur = sum(canvas[:, i:i + hh, j:j + ww] for i in range(5) for j in range(5)) / 25.0
    blur = ((blur - blur.min()) / (blur.max() - blur.min())).astype(np.float32)
    dx, dy = shift
    a = blur[:, margin:margin + H, margin:margin + W]
    b = blur[:, margin - dy:margin - dy + H, margin - dx:margin - dx + W]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def noise_pair(seed, H, W, C=3):
    """Independent 0 / 255 noise in both images (0.0 and 1.0 come back as the bytes 0 and 255): the derivatives reach their bound, and at win 31, C 3 the window sums pass 2^31."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2, (C, H, W)).astype(np.float32), rng.integers(0, 2, (C, H, W)).astype(np.float32))


def point_set(seed, H, W, win, n=200):
    """About n rows (pts1, pts2) normalised float32 [n, 2]: integer and half-pixel coordinates, the four corners and edge points, points whose window crosses the
    border, guesses displaced by up to 10 px, points outside the image, and one row that is not finite."""
    rng = np.random.default_rng(seed)
    sc = np.array([W - 1, H - 1], np.float64)
    px = [rng.uniform(0, 1, (n - 60, 2)) * sc]                                                  # anywhere inside
    px.append(np.floor(rng.uniform(0, 1, (10, 2)) * sc))                                        # integer pixels
    px.append(np.floor(rng.uniform(0, 1, (10, 2)) * (sc - 1)) + 0.5)                            # half pixels
    px.append(np.array([(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)], np.float64))           # corners
    px.append(np.array([(0, H / 2), (W - 1, H / 3), (W / 2, 0), (W / 3, H - 1)], np.float64))   # edges
    r = win // 2
    px.append(np.stack([rng.uniform(0, r, 8), rng.uniform(0, H - 1, 8)], 1))                    # the window crosses the left / top / right / bottom border
    px.append(np.stack([rng.uniform(0, W - 1, 8), rng.uniform(H - 1 - r, H - 1, 8)], 1))
    px.append(np.array([(-3.0, 5.0), (W + 2.5, H / 2), (W / 2, -win - 4.0), (W / 2, H + win + 3.0), (-win - 0.5, -win - 0.5), (W + 240.0, 7.0),
                        (-40.0, H / 2), (W - 0.25, H - 0.25)], np.float64))                       # outside (near and far)
    px = np.concatenate(px)
    disp = rng.uniform(-10, 10, px.shape)
    disp[::3] = 0.0                                                                             # a third starts where it is
    pts1 = (px / sc).astype(np.float32)
    pts2 = ((px + disp) / sc).astype(np.float32)
    bad = np.array([[np.nan, 0.5], [0.25, np.inf]], np.float32)
    pts1 = np.concatenate([pts1, bad[:1], np.float32([[0.5, 0.5]])])
    pts2 = np.concatenate([pts2, np.float32([[0.5, 0.5]]), bad[1:]])
    return pts1, pts2
