// lk.hip -- the tensor Lucas-Kanade tracker of the reference:
//   kpb_lk_track   utils/matcher.py:7-142  OpticalFlow(params)(img1, img2, pts1, pts2)
//   kpb_lk_track_batch   the same for a batch of pairs on maps of any strides: the same kernels with the pair on the grid's second axis
//
// The reference unfolds six (win*win*C)-channel patch maps per pyramid level -- 1.6 GB each at 480x640 with the
// configured 21x21 window -- and grid_samples them at the keypoints, 40 times.  Sampling an unfolded map at (px, py)
// is, for window cell (ky, kx),
//     sum over the bilinear taps (xt, yt) of (px, py) inside the image   w_t * img[c][yt + ky - r][xt + kx - r]
// (zero outside the image), so nothing is materialised here: one wave per keypoint, the window's cells strided over
// the lanes, every cell read straight from the image and the two Sobel maps (L2-resident), five butterfly
// reductions per iteration.  fp32 throughout, the reference's formulas kept as they are -- including its update
// einsum 'bik,bk->bk', which sums the inverse over its second index instead of applying it.
#include "kpb_common.h"
#include "interp.h"

namespace {

struct Taps { int x0, y0; float w[4]; bool ok[4]; };

// grid_sample(align_corners=True, bilinear, zeros) taps of pixel position (px, py), through the reference's normalise
// (matcher.py:109, 115) and kpb_grid_taps (interp.h); ok[k]: tap k lies inside the image
__device__ __forceinline__ Taps make_taps(float px, float py, int H, int W)
{
    const kpb_grid g = kpb_grid_taps(px / (float)(W - 1) * 2.0f - 1.0f, py / (float)(H - 1) * 2.0f - 1.0f, W, H);
    Taps t{(int)g.x0, (int)g.y0, {g.w[0], g.w[1], g.w[2], g.w[3]}, {}};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xt = t.x0 + (k & 1), yt = t.y0 + (k >> 1);
        t.ok[k] = xt >= 0 && xt < W && yt >= 0 && yt < H;
    }
    return t;
}

// a map, or a batch of them, through its element strides: planar [C][H][W] is (C*H*W, H*W, W, 1), channels-last [H][W][C] is (H*W*C, 1, W*C, C).
// kpb_lk_track and the tracker's own pooled / Sobel planes are the planar case; level 0 of kpb_lk_track_batch reads the caller's maps as they lie.
// Inside one pair's map the offsets are 32-bit (lk_run checks that the map spans fewer than 2^31 elements): the twelve taps of a window cell are address
// arithmetic first of all, and 64-bit multiplies there cost the single-pair entry 5 %.
struct View {
    const float* p; int64_t sb; int sc, sh, sw;
    __device__ __forceinline__ View plane(int j, int c) const { return View{p + j * sb + c * sc, sb, sc, sh, sw}; }
    __device__ __forceinline__ float at(int y, int x) const { return p[y * sh + x * sw]; }
};

__device__ __forceinline__ float sample_cell(const View& img, int H, int W, const Taps& t, int oy, int ox)
{
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = t.y0 + (k >> 1) + oy, x = t.x0 + (k & 1) + ox;
        if (t.ok[k] && y >= 0 && y < H && x >= 0 && x < W) s += img.at(y, x) * t.w[k];
    }
    return s;
}

// pair j's count: n_dev[j] held to [0, max_n], or max_n without counts
__device__ __forceinline__ int pair_n(const int32_t* n_dev, int j, int max_n) { return n_dev ? min(max(n_dev[j], 0), max_n) : max_n; }

// level images: out = avg_pool2d(img, k, k) (matcher.py:45), planar [pair][C][H/k][W/k]; k = 1 is never launched.  blockIdx.y: the pair
__global__ __launch_bounds__(256) void lk_avgpool(View img, float* __restrict__ out, int C, int H, int W, int k)
{
    const int Ho = H / k, Wo = W / k;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)C * Ho * Wo) return;
    const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho), c = (int)(i / ((size_t)Wo * Ho));
    const View p = img.plane(blockIdx.y, c);
    float s = 0.0f;
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) s += p.at(y * k + a, x * k + b);
    out[(size_t)blockIdx.y * C * Ho * Wo + i] = s / (float)(k * k);
}

// Sobel pair (matcher.py:23-24) as conv2d evaluates it: cross-correlation, zero padding 1 (87-90); dx, dy planar [pair][C][H][W]
__global__ __launch_bounds__(256) void lk_sobel(View img, float* __restrict__ dx, float* __restrict__ dy, int C, int H, int W)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)C * H * W) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), c = (int)(i / ((size_t)W * H));
    const View p = img.plane(blockIdx.y, c);
    auto at = [&](int yy, int xx) { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? p.at(yy, xx) : 0.0f; };
    float sx = 0.0f, sy = 0.0f;
    const float kx[3][3] = {{1, 0, -1}, {2, 0, -2}, {1, 0, -1}};
    const float ky[3][3] = {{1, 2, 1}, {0, 0, 0}, {-1, -2, -1}};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float v = at(y + a - 1, x + b - 1);
            sx += kx[a][b] * v; sy += ky[a][b] * v;
        }
    const size_t o = (size_t)blockIdx.y * C * H * W + i;
    dx[o] = sx; dy[o] = sy;
}

// pixel positions and the randomly displaced, clamped start (matcher.py:51-61).  Every per-point array is [pair][max_n][..]
__global__ void lk_init(const float* pts1, const float* pts2, int stride, const float* unit, const int32_t* n_dev, int max_n, int H, int W, float distance,
                        float* p1, float* p2, float* cur)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= pair_n(n_dev, j, max_n)) return;
    const size_t r = (size_t)j * max_n + i;
    p1[2 * r] = pts1[r * stride] * (float)(W - 1); p1[2 * r + 1] = pts1[r * stride + 1] * (float)(H - 1);
    const float x2 = pts2[r * stride] * (float)(W - 1), y2 = pts2[r * stride + 1] * (float)(H - 1);
    p2[2 * r] = x2; p2[2 * r + 1] = y2;
    cur[2 * r] = fminf(fmaxf(x2 + unit[2 * r] * distance, 10.0f), (float)(W - 10));
    cur[2 * r + 1] = fminf(fmaxf(y2 + unit[2 * r + 1] * distance, 10.0f), (float)(H - 10));
}

__device__ __forceinline__ float wave_sum(float v)
{
    v = kpb_wave_sum(v);
    return v;
}

struct LevelArgs {
    View img1, img2;    // the level's maps of every pair (level 0: the caller's; above: the pooled planes)
    const float* dx2; const float* dy2;     // planar [pair][C][H][W]
    const float* p1;    // [pair][max_n][2] full-resolution pixel positions in image 1
    float* cur;         // [pair][max_n][2] full-resolution estimate in image 2, updated in place
    const int32_t* n_dev;
    int max_n, C, H, W, win, iters;
    float scale;        // 2^(level index): positions are divided by it on entry and multiplied on exit (79-85)
};

// optical_flow_level (matcher.py:77-133): one wave per keypoint, blockIdx.y the pair; the patch of image 1 stays in LDS
__global__ __launch_bounds__(256) void lk_level(LevelArgs a)
{
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = blockIdx.y;
    const int i = blockIdx.x * 4 + wv;
    if (i >= pair_n(a.n_dev, j, a.max_n)) return;
    const int r = a.win / 2, WW = a.win * a.win, E = a.C * WW;
    const size_t P = (size_t)a.H * a.W, row = (size_t)j * a.max_n + i;
    const float *dx2 = a.dx2 + (size_t)j * a.C * P, *dy2 = a.dy2 + (size_t)j * a.C * P;
    float* patch = lds + (size_t)wv * E;
    {
        const Taps t1 = make_taps(a.p1[2 * row] / a.scale, a.p1[2 * row + 1] / a.scale, a.H, a.W);
        for (int e = lane; e < E; e += 64) {
            const int c = e / WW, k = e - c * WW, ky = k / a.win, kx = k - ky * a.win;
            patch[e] = sample_cell(a.img1.plane(j, c), a.H, a.W, t1, ky - r, kx - r);
        }
    }
    float px = a.cur[2 * row] / a.scale, py = a.cur[2 * row + 1] / a.scale;
    for (int it = 0; it < a.iters; ++it) {
        const Taps t = make_taps(px, py, a.H, a.W);
        float g00 = 0.f, g01 = 0.f, g11 = 0.f, b0 = 0.f, b1 = 0.f;
        for (int e = lane; e < E; e += 64) {
            const int c = e / WW, k = e - c * WW, ky = k / a.win, kx = k - ky * a.win;
            const float v = sample_cell(a.img2.plane(j, c), a.H, a.W, t, ky - r, kx - r);
            const float jx = sample_cell(View{dx2 + c * P, 0, 0, a.W, 1}, a.H, a.W, t, ky - r, kx - r);
            const float jy = sample_cell(View{dy2 + c * P, 0, 0, a.W, 1}, a.H, a.W, t, ky - r, kx - r);
            const float dI = patch[e] - v;                                  // 117
            g00 += jx * jx; g01 += jx * jy; g11 += jy * jy;                 // 121
            b0 += dI * jx; b1 += dI * jy;                                   // 122
        }
        g00 = wave_sum(g00); g01 = wave_sum(g01); g11 = wave_sum(g11); b0 = wave_sum(b0); b1 = wave_sum(b1);
        const float det = g00 * g11 - g01 * g01;                            // 123
        if (det > 1e-6f) {
            const float i00 = g11 / det, i01 = -g01 / det, i11 = g00 / det; // 124
            px = px - (i00 + i01) * b0;                                     // 125: 'bik,bk->bk' sums the inverse over i
            py = py - (i01 + i11) * b1;
        }
    }
    if (lane == 0) { a.cur[2 * row] = px * a.scale; a.cur[2 * row + 1] = py * a.scale; }
}

__global__ void lk_finish(const float* cur, const float* p2, const int32_t* n_dev, int max_n, float* out_pts, float* out_err)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= pair_n(n_dev, j, max_n)) return;
    const size_t r = (size_t)j * max_n + i;
    const float dx = cur[2 * r] - p2[2 * r], dy = cur[2 * r + 1] - p2[2 * r + 1];
    out_pts[2 * r] = cur[2 * r]; out_pts[2 * r + 1] = cur[2 * r + 1];
    out_err[r] = fminf(sqrtf(dx * dx + dy * dy), 8.0f);                     // 73
}

// Both entries: `batch` pairs of maps read through (sb, sc, sh, sw), max_n point rows a pair of which the first n_dev[j] are tracked.  `who` begins the messages.
int lk_run(kpb_ctx* ctx, const char* who, const float* map1_dev, const float* map2_dev, int batch, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh,
           int64_t sw, const float* pts1_dev, const float* pts2_dev, int pts_stride, const float* unit_dev, int max_n, const int32_t* n_dev,
           const kpb_lk_params* prm, float* out_pts_dev, float* out_err_dev)
{
    if (!map1_dev || !map2_dev || !prm || C <= 0 || H <= 20 || W <= 20 || max_n < 0 || pts_stride < 2 || batch <= 0 || sb <= 0 || sc <= 0 || sh <= 0 || sw <= 0)
        return kpb_fail(ctx, KPB_E_INVALID, "%s: bad argument", who);
    if (prm->win_size < 1 || prm->win_size > 31 || !(prm->win_size & 1) || prm->levels < 1 || prm->levels > 4 || prm->iterations < 0)
        return kpb_fail(ctx, KPB_E_UNSUPPORTED, "%s: win_size must be odd and <= 31, levels 1..4", who);
    if ((H >> (prm->levels - 1)) < 2 || (W >> (prm->levels - 1)) < 2)
        return kpb_fail(ctx, KPB_E_UNSUPPORTED, "%s: image too small for %d levels", who, prm->levels);
    if (batch > 65535) return kpb_fail(ctx, KPB_E_UNSUPPORTED, "%s: at most 65535 pairs a call (got %d)", who, batch);
    if ((C - 1) * sc + (H - 1) * sh + (W - 1) * sw >= ((int64_t)1 << 31))
        return kpb_fail(ctx, KPB_E_UNSUPPORTED, "%s: a pair's map spans 2^31 elements or more", who);
    if (max_n == 0) return KPB_OK;
    if (!pts1_dev || !pts2_dev || !unit_dev || !out_pts_dev || !out_err_dev)
        return kpb_fail(ctx, KPB_E_INVALID, "%s: null buffer", who);
    const size_t lds = (size_t)4 * C * prm->win_size * prm->win_size * sizeof(float);
    if (lds > 64 * 1024) return kpb_fail(ctx, KPB_E_UNSUPPORTED, "%s: window of %d x %d x %d does not fit the patch buffer", who, prm->win_size, prm->win_size, C);
    KPB_HIP(ctx, hipSetDevice(ctx->device));
    const size_t B = batch, P = (size_t)H * W, plane = (size_t)C * P, pooled = prm->levels > 1 ? (size_t)C * (H / 2) * (W / 2) : 0;
    // workspace: p1, p2, cur [pair][max_n][2]; per pair the pooled image 1 / image 2 (the largest is level 1's, a quarter) and dx, dy of image 2 (full size at level 0)
    float *p1 = nullptr, *p2 = nullptr, *cur = nullptr, *l1 = nullptr, *l2 = nullptr, *dx = nullptr, *dy = nullptr;
    if (int rc = kpb_carve(ctx, ctx->ws_misc, [&](Arena& a) {      // (ws_misc: nothing of an earlier call is expected in it)
            p1 = a.take(2 * B * max_n); p2 = a.take(2 * B * max_n); cur = a.take(2 * B * max_n);
            l1 = a.take(B * pooled); l2 = a.take(B * pooled); dx = a.take(B * plane); dy = a.take(B * plane);
        })) return rc;
    hipStream_t st = ctx->stream;
    const dim3 gpts(cdiv(max_n, 256), batch);
    KPB_LAUNCH(ctx, "lk_init", lk_init, gpts, dim3(256), 0, st, pts1_dev, pts2_dev, pts_stride, unit_dev, n_dev, max_n, H, W, prm->distance, p1, p2, cur);
    const View v1{map1_dev, sb, (int)sc, (int)sh, (int)sw}, v2{map2_dev, sb, (int)sc, (int)sh, (int)sw};
    for (int lv = 0; lv < prm->levels; ++lv) {
        const int idx = prm->levels - lv - 1;
        const int k = idx == 0 ? 1 : 2 * idx;       // build_pyramid (45): level i > 0 is avg_pool2d(img, 2i, 2i) ...
        const int Hl = H / k, Wl = W / k;
        const dim3 gpix((unsigned)(((size_t)C * Hl * Wl + 255) / 256), batch);
        View a = v1, b = v2;
        if (k > 1) {
            KPB_LAUNCH(ctx, "lk_avgpool", lk_avgpool, gpix, dim3(256), 0, st, v1, l1, C, H, W, k);
            KPB_LAUNCH(ctx, "lk_avgpool", lk_avgpool, gpix, dim3(256), 0, st, v2, l2, C, H, W, k);
            const int64_t Pl = (int64_t)Hl * Wl;
            a = View{l1, C * Pl, (int)Pl, Wl, 1}; b = View{l2, C * Pl, (int)Pl, Wl, 1};
        }
        KPB_LAUNCH(ctx, "lk_sobel", lk_sobel, gpix, dim3(256), 0, st, b, dx, dy, C, Hl, Wl);
        LevelArgs la{a, b, dx, dy, p1, cur, n_dev, max_n, C, Hl, Wl, prm->win_size, prm->iterations, (float)(1 << idx)};   // ... while positions scale by 2^i (66, 79)
        KPB_LAUNCH(ctx, "lk_level", lk_level, dim3(cdiv(max_n, 4), batch), dim3(256), lds, st, la);
    }
    KPB_LAUNCH(ctx, "lk_finish", lk_finish, gpts, dim3(256), 0, st, cur, p2, n_dev, max_n, out_pts_dev, out_err_dev);
    KPB_HIP(ctx, hipGetLastError());
    return KPB_OK;
}

// kpb_track_error: one wave per pair (blockIdx.x).  The error of a row is the reference's three fp32 tensor operations (VisualizeTrackingError.py:45-46: a
// multiply, a subtraction, the norm of two components), each rounded on its own -- nothing contracted into an fma.  The mean is a float64 sum in one fixed order:
// lane l adds rows l, l + 64, ... ascending, then the butterfly 32 .. 1 (a + b is commutative, so every lane ends with the same bits).
__global__ __launch_bounds__(64) void lk_track_error(const float* __restrict__ kps01, int stride, const float* __restrict__ tracked, const int32_t* n_dev, int max_n,
                                                     const float* __restrict__ scale, float* __restrict__ out_err, double* __restrict__ out_mean)
{
    const int lane = threadIdx.x, j = blockIdx.x, n = pair_n(n_dev, j, max_n);
    const float sx = scale[2 * j], sy = scale[2 * j + 1];
    double s = 0.0;
    for (int i = lane; i < n; i += 64) {
        const size_t r = (size_t)j * max_n + i;
        const float dx = __fsub_rn(__fmul_rn(kps01[r * stride], sx), tracked[2 * r]);
        const float dy = __fsub_rn(__fmul_rn(kps01[r * stride + 1], sy), tracked[2 * r + 1]);
        const float e = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));       // sqrtf: correctly rounded (__fsqrt_rn is the 1-ulp native root here)
        out_err[r] = e;
        s += (double)e;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out_mean[j] = n > 0 ? s / (double)n : __longlong_as_double(0x7ff8000000000000ll);
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int kpb_track_error(
    kpb_ctx* ctx, const float* kps01_dev, int pts_stride, const float* tracked_dev, int batch, int max_n, const int32_t* n_dev, const float* scale_dev,
    float* out_err_dev, double* out_mean_dev)
{
    if (!ctx) return kpb_fail(nullptr, KPB_E_INVALID, "kpb_track_error: null context");
    if (!scale_dev || !out_mean_dev || pts_stride < 2 || batch <= 0 || max_n < 0) return kpb_fail(ctx, KPB_E_INVALID, "kpb_track_error: bad argument");
    if (max_n > 0 && (!kps01_dev || !tracked_dev || !out_err_dev)) return kpb_fail(ctx, KPB_E_INVALID, "kpb_track_error: null buffer");
    if (batch > 65535) return kpb_fail(ctx, KPB_E_UNSUPPORTED, "kpb_track_error: at most 65535 pairs a call (got %d)", batch);
    KPB_HIP(ctx, hipSetDevice(ctx->device));
    KPB_LAUNCH(ctx, "lk_track_error", lk_track_error, dim3(batch), dim3(64), 0, ctx->stream, kps01_dev, pts_stride, tracked_dev, n_dev, max_n, scale_dev,
               out_err_dev, out_mean_dev);
    KPB_HIP(ctx, hipGetLastError());
    return KPB_OK;
}

extern "C" __attribute__((visibility("default"))) int kpb_lk_track(
    kpb_ctx* ctx, const float* img1_dev, const float* img2_dev, int C, int H, int W, const float* pts1_dev, const float* pts2_dev,
    int pts_stride, const float* unit_dev, int n, const kpb_lk_params* prm, float* out_pts_dev, float* out_err_dev)
{
    if (!ctx) return kpb_fail(nullptr, KPB_E_INVALID, "kpb_lk_track: null context");
    return lk_run(ctx, "kpb_lk_track", img1_dev, img2_dev, 1, C, H, W, (int64_t)C * H * W, (int64_t)H * W, W, 1, pts1_dev, pts2_dev, pts_stride, unit_dev, n,
                  nullptr, prm, out_pts_dev, out_err_dev);
}

// Pair j tracks from map1_dev + j sb into map2_dev + j sb (a sequence passes map2 = map1 + sb).  Row for row the bits of kpb_lk_track on that pair's maps made
// planar: the same kernels, with the pair on the grid's second axis, n[j] read on the device, and only level 0 reading through the strides.
extern "C" __attribute__((visibility("default"))) int kpb_lk_track_batch(
    kpb_ctx* ctx, const float* map1_dev, const float* map2_dev, int batch, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
    const float* pts1_dev, const float* pts2_dev, int pts_stride, const float* unit_dev, int max_n, const int32_t* n_dev, const kpb_lk_params* prm,
    float* out_pts_dev, float* out_err_dev)
{
    if (!ctx) return kpb_fail(nullptr, KPB_E_INVALID, "kpb_lk_track_batch: null context");
    if (ctx->lk_pyrlk) {        // KPB_OPT_LK_PYRLK: the tracker behind optical_flow_cv (csrc/pyrlk.hip); unit_dev, distance and iterations are not read
        if (!prm) return kpb_fail(ctx, KPB_E_INVALID, "kpb_pyrlk_track: null map or params pointer");
        return kpb_pyrlk_track(ctx, map1_dev, map2_dev, batch, C, H, W, sb, sc, sh, sw, pts1_dev, pts2_dev, pts_stride, max_n, n_dev, prm->win_size, prm->levels,
                               out_pts_dev, out_err_dev);
    }
    return lk_run(ctx, "kpb_lk_track_batch", map1_dev, map2_dev, batch, C, H, W, sb, sc, sh, sw, pts1_dev, pts2_dev, pts_stride, unit_dev, max_n, n_dev, prm,
                  out_pts_dev, out_err_dev);
}
