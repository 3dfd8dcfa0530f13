// pyrlk.hip -- the pyramidal Lucas-Kanade tracker behind the reference's optical_flow_cv (utils/matcher.py:145-185), which wraps
//   cv2.calcOpticalFlowPyrLK(img0, img1, pts0, pts1, winSize, maxLevel, OPTFLOW_USE_INITIAL_FLOW, (EPS | COUNT, 10, 0.03))
// and is what the visual_odometer task tracks with (tasks/visual_odometer.py:43-47):
//   kpb_pyrlk_track   `batch` pairs on maps of any strides, the pair on the grid's second axis -- no export of its own: kpb_lk_track_batch runs it under
//                     KPB_OPT_LK_PYRLK (include/kpb.h), and the status goes out as 1.0f / 0.0f where that entry's error column stands
//
// RESTATED, cv2 PARITY UNPINNED (OpenCV is absent here, like for Harris and the RANSAC estimators).  What the kernels compute is "PyrLK-R", the definition of
// DESIGN.md section 7a, restated from OpenCV 4.x lkpyramid.cpp / pyramids.cpp: everything up to the 2 x 2 solve is integer arithmetic on uint8 / int16 data, the
// window sums are EXACT 64-bit integers rounded to fp32 once (cv2 adds them in fp32 in an order its SIMD build decides; the exact sum lies inside that spread and
// has no order), and every fp32 step after that is one IEEE operation (the library is built with -ffp-contract=off; sqrtf and / are the correctly rounded ones).
// So the device agrees bit for bit with the numpy restatement in tests/pyrlk_fixtures.py, alone or in a batch.
//
// One wave per point and launch, one launch per pyramid level (top first), as lk.hip does it.  The point's interpolated window of image 1 -- I, Ix, Iy as int16,
// 6 win^2 C bytes: 17 KB at win 31, C 3 -- stays in LDS through the level's iterations; two window rows a pass (lane >> 5 the row, lane & 31 the column: no division by
// the window size anywhere), every lane reading back only what it wrote.
#include "kpb_common.h"

#include <algorithm>
#include <cfloat>

namespace {

// the caller's maps through their element strides, as lk.hip's View (read once, by the byte conversion: 64-bit offsets cost nothing here)
struct View { const float* p; int64_t sb, sc, sh, sw; };

__device__ __forceinline__ int pair_n(const int32_t* n_dev, int j, int max_n) { return n_dev ? min(max(n_dev[j], 0), max_n) : max_n; }

// reflect-101 (numpy's "reflect"): -1 -> 1, n -> n - 2.  Callers stay within n - 1 of the image (n > win and the range tests below); the clamp is a seat belt, not arithmetic.
__device__ __forceinline__ int refl(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}

// uint8 planes [pair][C][H][W] = trunc(x * 255f) & 255: the reference's (img * 255.).astype(np.uint8), the Harris rule without the channel sum
__global__ __launch_bounds__(256) void pyrlk_bytes(View img, uint8_t* __restrict__ out, int C, int H, int W)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, P = (size_t)H * W;
    if (i >= (size_t)C * P) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), c = (int)(i / P);
    const float v = img.p[(int64_t)blockIdx.y * img.sb + c * img.sc + y * img.sh + x * img.sw] * 255.0f;
    out[(size_t)blockIdx.y * C * P + i] = (uint8_t)((int)v & 255);
}

// cv::pyrDown: out (x, y) = (sum of the 1-4-6-4-1 x 1-4-6-4-1 taps around in (2x, 2y), reflect-101, + 128) >> 8.  `planes` = C; planar [pair][C][..]
__global__ __launch_bounds__(256) void pyrlk_down(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int planes, int H, int W, int Ho, int Wo)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, Po = (size_t)Ho * Wo;
    if (i >= (size_t)planes * Po) return;
    const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho), c = (int)(i / Po);
    const uint8_t* p = in + ((size_t)blockIdx.y * planes + c) * H * W;
    const int k[5] = {1, 4, 6, 4, 1};
    int s = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const uint8_t* r = p + (size_t)refl(2 * y + a - 2, H) * W;
        int t = 0;
#pragma unroll
        for (int b = 0; b < 5; ++b) t += k[b] * r[refl(2 * x + b - 2, W)];
        s += k[a] * t;
    }
    out[(size_t)blockIdx.y * planes * Po + i] = (uint8_t)((s + 128) >> 8);
}

// Scharr pair as int16 (|.| <= 16 * 255 = 4080), reflect-101: dx = S(x + 1) - S(x - 1) with S the vertical 3-10-3 smooth, dy = the horizontal 3-10-3 smooth of row (y + 1) - row (y - 1)
__global__ __launch_bounds__(256) void pyrlk_scharr(const uint8_t* __restrict__ in, int16_t* __restrict__ dx, int16_t* __restrict__ dy, int planes, int H, int W)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, P = (size_t)H * W;
    if (i >= (size_t)planes * P) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), c = (int)(i / P);
    const uint8_t* p = in + ((size_t)blockIdx.y * planes + c) * P;
    const uint8_t *r0 = p + (size_t)refl(y - 1, H) * W, *r1 = p + (size_t)y * W, *r2 = p + (size_t)refl(y + 1, H) * W;
    const int xl = refl(x - 1, W), xr = refl(x + 1, W);
    const int sl = 3 * r0[xl] + 10 * r1[xl] + 3 * r2[xl], sr = 3 * r0[xr] + 10 * r1[xr] + 3 * r2[xr];
    const int dl = r2[xl] - r0[xl], dc = r2[x] - r0[x], dr = r2[xr] - r0[xr];
    const size_t o = (size_t)blockIdx.y * planes * P + i;
    dx[o] = (int16_t)(sr - sl);
    dy[o] = (int16_t)(3 * dl + 10 * dc + 3 * dr);
}

// Pixel positions of the points and of their guesses; a row that is not finite is answered here (as given, status 0) and marked dead (-1) for the level kernels.
// Per-point state, [pair][max_n]: prev (2), cur (2: the carried estimate, full resolution until the top level scales it), status.
__global__ void pyrlk_init(const float* pts1, const float* pts2, int stride, const int32_t* n_dev, int max_n, int H, int W, float* prev, float* cur, int* status,
                           float* out_pts, float* out_status)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= pair_n(n_dev, j, max_n)) return;
    const size_t r = (size_t)j * max_n + i;
    const float gx = pts2[r * stride], gy = pts2[r * stride + 1];
    const float x1 = pts1[r * stride] * (float)(W - 1), y1 = pts1[r * stride + 1] * (float)(H - 1), x2 = gx * (float)(W - 1), y2 = gy * (float)(H - 1);
    if (!(isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2))) {
        out_pts[2 * r] = gx; out_pts[2 * r + 1] = gy; out_status[r] = 0.0f;
        status[r] = -1;
        return;
    }
    prev[2 * r] = x1; prev[2 * r + 1] = y1; cur[2 * r] = x2; cur[2 * r + 1] = y2; status[r] = 1;
}

__device__ __forceinline__ long long wave_sum64(long long v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the 14-bit bilinear weights of a position whose floor is (fx, fy): cvRound = rint, ties to even
struct Weights { int w00, w01, w10, w11; };
__device__ __forceinline__ Weights make_weights(float px, float py, float fx, float fy)
{
    const float a = px - fx, b = py - fy;
    Weights w;
    w.w00 = (int)rintf((1.0f - a) * (1.0f - b) * 16384.0f);
    w.w01 = (int)rintf(a * (1.0f - b) * 16384.0f);
    w.w10 = (int)rintf((1.0f - a) * b * 16384.0f);
    w.w11 = 16384 - w.w00 - w.w01 - w.w10;
    return w;
}

// -win <= floor < n, in the float domain (a NaN or a huge position fails; the integer conversion happens only behind this test)
__device__ __forceinline__ bool in_range(float fx, float fy, int win, int W, int H)
{
    return fx >= (float)-win && fx < (float)W && fy >= (float)-win && fy < (float)H;
}

// DESCALE(sum of the four taps * weights, 9) of a uint8 plane extended by reflect-101
__device__ __forceinline__ int sample_u8(const uint8_t* p, int H, int W, int y, int x, const Weights& w)
{
    const uint8_t *r0 = p + (size_t)refl(y, H) * W, *r1 = p + (size_t)refl(y + 1, H) * W;
    const int x0 = refl(x, W), x1 = refl(x + 1, W);
    return (r0[x0] * w.w00 + r0[x1] * w.w01 + r1[x0] * w.w10 + r1[x1] * w.w11 + 256) >> 9;
}

// DESCALE(.., 14) of an int16 derivative plane that is 0 outside the image
__device__ __forceinline__ int sample_d16(const int16_t* p, int H, int W, int y, int x, const Weights& w)
{
    const bool y0 = y >= 0 && y < H, y1 = y + 1 >= 0 && y + 1 < H, x0 = x >= 0 && x < W, x1 = x + 1 >= 0 && x + 1 < W;
    const int v00 = (y0 && x0) ? p[(size_t)y * W + x] : 0, v01 = (y0 && x1) ? p[(size_t)y * W + x + 1] : 0;
    const int v10 = (y1 && x0) ? p[(size_t)(y + 1) * W + x] : 0, v11 = (y1 && x1) ? p[(size_t)(y + 1) * W + x + 1] : 0;
    return (v00 * w.w00 + v01 * w.w01 + v10 * w.w10 + v11 * w.w11 + 8192) >> 14;
}

struct LevelArgs {
    const uint8_t *img1, *img2;         // this level's planes [pair][C][H][W]
    const int16_t *dx, *dy;             // image 1's derivatives, same layout
    const float* prev;                  // [pair][max_n][2] full-resolution pixel positions in image 1
    float* cur;                         // [pair][max_n][2] the carried estimate in image 2, at the resolution of the level above (full resolution before the top level)
    int* status;                        // [pair][max_n] 1, 0, or -1 = answered by pyrlk_init
    const int32_t* n_dev;
    int max_n, C, H, W, win, level, top, H0, W0;
    float* out_pts; float* out_status;          // written by level 0: normalised points, the status as 1.0f / 0.0f
};

__global__ __launch_bounds__(256) void pyrlk_level(LevelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int16_t lds16[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wpb = blockDim.x >> 6, j = blockIdx.y;
    const int i = blockIdx.x * wpb + wv;
    if (i >= pair_n(a.n_dev, j, a.max_n)) return;
    const size_t row = (size_t)j * a.max_n + i;
    int st = a.status[row];
    if (st < 0) return;
    const int win = a.win, W = a.W, H = a.H, C = a.C, WW = win * win, E = (C * WW + 7) & ~7;
    const size_t P = (size_t)H * W;
    const uint8_t *img1 = a.img1 + (size_t)j * C * P, *img2 = a.img2 + (size_t)j * C * P;
    const int16_t *dxp = a.dx + (size_t)j * C * P, *dyp = a.dy + (size_t)j * C * P;
    int16_t *Iw = lds16 + (size_t)wv * 3 * E, *Ixw = Iw + E, *Iyw = Ixw + E;
    const int ky_l = lane >> 5, kx = lane & 31;
    const float half = (float)(win - 1) * 0.5f, scale = 1.0f / (float)(1 << a.level), FLT_SCALE = 1.0f / (float)(1 << 20);

    const float px = a.prev[2 * row] * scale - half, py = a.prev[2 * row + 1] * scale - half;
    float cx, cy;           // the carried value: stored before anything else happens
    if (a.level == a.top) { cx = a.cur[2 * row] * scale; cy = a.cur[2 * row + 1] * scale; }
    else { cx = a.cur[2 * row] * 2.0f; cy = a.cur[2 * row + 1] * 2.0f; }

    const float pfx = floorf(px), pfy = floorf(py);
    bool go = in_range(pfx, pfy, win, W, H);
    if (!go && a.level == 0) st = 0;
    float A11 = 0.f, A12 = 0.f, A22 = 0.f, D = 0.f;
    if (go) {
        const int ipx = (int)pfx, ipy = (int)pfy;
        const Weights w = make_weights(px, py, pfx, pfy);
        long long sxx = 0, sxy = 0, syy = 0;
        for (int c = 0; c < C; ++c)
            for (int ky0 = 0; ky0 < win; ky0 += 2) {
                const int ky = ky0 + ky_l;
                if (kx < win && ky < win) {
                    const int e = (c * win + ky) * win + kx, y = ipy + ky, x = ipx + kx;
                    const int iv = sample_u8(img1 + c * P, H, W, y, x, w);
                    const int ix = sample_d16(dxp + c * P, H, W, y, x, w), iy = sample_d16(dyp + c * P, H, W, y, x, w);
                    Iw[e] = (int16_t)iv; Ixw[e] = (int16_t)ix; Iyw[e] = (int16_t)iy;
                    sxx += (long long)(ix * ix); sxy += (long long)(ix * iy); syy += (long long)(iy * iy);
                }
            }
        sxx = wave_sum64(sxx); sxy = wave_sum64(sxy); syy = wave_sum64(syy);
        A11 = (float)sxx * FLT_SCALE; A12 = (float)sxy * FLT_SCALE; A22 = (float)syy * FLT_SCALE;
        D = A11 * A22 - A12 * A12;
        const float dif = A11 - A22;
        const float minEig = ((A22 + A11) - sqrtf(dif * dif + (4.0f * A12) * A12)) / (float)(2 * win * win);
        if ((double)minEig < 1e-4 || D < FLT_EPSILON) {
            go = false;
            if (a.level == 0) st = 0;
        }
    }
    if (go) {
        D = 1.0f / D;
        float nx = cx - half, ny = cy - half, pdx = 0.0f, pdy = 0.0f;
        for (int it = 0; it < 10; ++it) {
            const float nfx = floorf(nx), nfy = floorf(ny);
            if (!in_range(nfx, nfy, win, W, H)) {
                if (a.level == 0) st = 0;
                break;
            }
            const int inx = (int)nfx, iny = (int)nfy;
            const Weights w = make_weights(nx, ny, nfx, nfy);
            long long s1 = 0, s2 = 0;
            for (int c = 0; c < C; ++c)
                for (int ky0 = 0; ky0 < win; ky0 += 2) {
                    const int ky = ky0 + ky_l;
                    if (kx < win && ky < win) {
                        const int e = (c * win + ky) * win + kx;
                        const int diff = sample_u8(img2 + c * P, H, W, iny + ky, inx + kx, w) - (int)Iw[e];
                        s1 += (long long)(diff * (int)Ixw[e]); s2 += (long long)(diff * (int)Iyw[e]);
                    }
                }
            s1 = wave_sum64(s1); s2 = wave_sum64(s2);
            const float b1 = (float)s1 * FLT_SCALE, b2 = (float)s2 * FLT_SCALE;
            const float ddx = (A12 * b2 - A22 * b1) * D, ddy = (A12 * b1 - A11 * b2) * D;
            nx += ddx; ny += ddy;
            cx = nx + half; cy = ny + half;
            if ((double)ddx * (double)ddx + (double)ddy * (double)ddy <= 0.03 * 0.03) break;
            if (it > 0 && fabs((double)(ddx + pdx)) < 0.01 && fabs((double)(ddy + pdy)) < 0.01) {
                cx -= ddx * 0.5f; cy -= ddy * 0.5f;
                break;
            }
            pdx = ddx; pdy = ddy;
        }
    }
    if (a.level == 0 && st == 1) {          // the check behind the error output: the window of the answer itself
        if (!in_range(floorf(cx - half), floorf(cy - half), win, W, H)) st = 0;
    }
    if (lane == 0) {
        a.cur[2 * row] = cx; a.cur[2 * row + 1] = cy; a.status[row] = st;
        if (a.level == 0) {
            a.out_pts[2 * row] = cx / (float)(a.W0 - 1); a.out_pts[2 * row + 1] = cy / (float)(a.H0 - 1);
            a.out_status[row] = (float)st;
        }
    }
}

}  // namespace

// The sizes of the pyramid kpb_pyrlk_track builds: level l + 1 is ((W + 1) / 2, (H + 1) / 2), and a level that would not be larger than the window both ways is
// not built.  Returns the top level (<= levels); Ws / Hs hold levels 0 .. top.
static int pyrlk_sizes(int H, int W, int win, int levels, int* Hs, int* Ws)
{
    int L = 0;
    Hs[0] = H; Ws[0] = W;
    while (L < levels) {
        const int nh = (Hs[L] + 1) / 2, nw = (Ws[L] + 1) / 2;
        if (nw <= win || nh <= win) break;
        ++L;
        Hs[L] = nh; Ws[L] = nw;
    }
    return L;
}

int kpb_pyrlk_track(kpb_ctx* ctx, const float* map1_dev, const float* map2_dev, int batch, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                    const float* pts1_dev, const float* pts2_dev, int pts_stride, int max_n, const int32_t* n_dev, int win, int levels, float* out_pts_dev,
                    float* out_status_dev)
{
    const char* who = "kpb_pyrlk_track";
    if (!ctx) return kpb_fail(nullptr, KPB_E_INVALID, "%s: null context", who);
    if (!map1_dev || !map2_dev) return kpb_fail(ctx, KPB_E_INVALID, "%s: null map or params pointer", who);
    if (batch <= 0 || max_n < 0 || pts_stride < 2 || H <= 0 || W <= 0 || sb <= 0 || sc <= 0 || sh <= 0 || sw <= 0)
        return kpb_fail(ctx, KPB_E_INVALID, "%s: bad argument (batch %d, max_n %d, pts_stride %d, a size or a stride below 1)", who, batch, max_n, pts_stride);
    if (max_n > 0 && (!pts1_dev || !pts2_dev || !out_pts_dev || !out_status_dev)) return kpb_fail(ctx, KPB_E_INVALID, "%s: null buffer", who);
    if (win < 3 || win > 31 || !(win & 1) || levels < 0 || levels > 4)
        return kpb_fail(ctx, KPB_E_UNSUPPORTED, "%s: win_size must be odd and in 3 .. 31, levels in 0 .. 4 (got %d, %d)", who, win, levels);
    if (C != 1 && C != 3) return kpb_fail(ctx, KPB_E_UNSUPPORTED, "%s: maps of 1 or 3 channels (got %d)", who, C);
    if (H <= win || W <= win) return kpb_fail(ctx, KPB_E_UNSUPPORTED, "%s: a %d x %d map is not larger than the %d x %d window", who, H, W, win, win);
    if (batch > 65535) return kpb_fail(ctx, KPB_E_UNSUPPORTED, "%s: at most 65535 pairs a call (got %d)", who, batch);
    if ((C - 1) * sc + (H - 1) * sh + (W - 1) * sw >= ((int64_t)1 << 31) || (int64_t)C * H * W >= ((int64_t)1 << 31))
        return kpb_fail(ctx, KPB_E_UNSUPPORTED, "%s: a pair's map spans 2^31 elements or more", who);
    if (max_n == 0) return KPB_OK;
    KPB_HIP(ctx, hipSetDevice(ctx->device));
    int Hs[5], Ws[5];
    const int top = pyrlk_sizes(H, W, win, levels, Hs, Ws);
    const size_t B = batch;
    size_t off[6] = {0};            // level l's planes of all pairs start at off[l] (elements: one per pixel and channel)
    for (int l = 0; l <= top; ++l) off[l + 1] = off[l] + B * C * Hs[l] * Ws[l];
    // workspace: both uint8 pyramids, image 1's derivative pyramids, the per-point state
    uint8_t *u1 = nullptr, *u2 = nullptr;
    int16_t *dx = nullptr, *dy = nullptr;
    float *prev = nullptr, *cur = nullptr;
    int* status = nullptr;
    if (int rc = kpb_carve(ctx, ctx->ws_misc, [&](Arena& a) {      // (ws_misc: nothing of an earlier call is expected in it)
            u1 = a.take<uint8_t>(off[top + 1]); u2 = a.take<uint8_t>(off[top + 1]);
            dx = a.take<int16_t>(off[top + 1]); dy = a.take<int16_t>(off[top + 1]);
            prev = a.take(2 * B * max_n); cur = a.take(2 * B * max_n); status = a.take<int>(B * max_n);
        })) return rc;
    hipStream_t st = ctx->stream;
    const auto gpix = [&](int l) { return dim3((unsigned)(((size_t)C * Hs[l] * Ws[l] + 255) / 256), batch); };
    KPB_LAUNCH(ctx, "pyrlk_bytes", pyrlk_bytes, gpix(0), dim3(256), 0, st, View{map1_dev, sb, sc, sh, sw}, u1, C, H, W);
    KPB_LAUNCH(ctx, "pyrlk_bytes", pyrlk_bytes, gpix(0), dim3(256), 0, st, View{map2_dev, sb, sc, sh, sw}, u2, C, H, W);
    for (int l = 0; l <= top; ++l) {
        if (l > 0) {
            KPB_LAUNCH(ctx, "pyrlk_down", pyrlk_down, gpix(l), dim3(256), 0, st, u1 + off[l - 1], u1 + off[l], C, Hs[l - 1], Ws[l - 1], Hs[l], Ws[l]);
            KPB_LAUNCH(ctx, "pyrlk_down", pyrlk_down, gpix(l), dim3(256), 0, st, u2 + off[l - 1], u2 + off[l], C, Hs[l - 1], Ws[l - 1], Hs[l], Ws[l]);
        }
        KPB_LAUNCH(ctx, "pyrlk_scharr", pyrlk_scharr, gpix(l), dim3(256), 0, st, u1 + off[l], dx + off[l], dy + off[l], C, Hs[l], Ws[l]);
    }
    KPB_LAUNCH(ctx, "pyrlk_init", pyrlk_init, dim3(cdiv(max_n, 256), batch), dim3(256), 0, st, pts1_dev, pts2_dev, pts_stride, n_dev, max_n, H, W, prev, cur,
               status, out_pts_dev, out_status_dev);
    // a wave's window: I, Ix, Iy as int16, the cell count rounded up to 8; as many waves a workgroup (at most 4) as 64 KB of LDS hold
    const size_t wave_lds = (size_t)3 * ((C * win * win + 7) & ~7) * sizeof(int16_t);
    const int wpb = (int)std::min<size_t>(4, (64 * 1024) / wave_lds);
    for (int l = top; l >= 0; --l) {
        LevelArgs la{u1 + off[l], u2 + off[l], dx + off[l], dy + off[l], prev, cur, status, n_dev, max_n, C, Hs[l], Ws[l], win, l, top, H, W, out_pts_dev, out_status_dev};
        KPB_LAUNCH(ctx, "pyrlk_level", pyrlk_level, dim3(cdiv(max_n, wpb), batch), dim3(64 * wpb), wpb * wave_lds, st, la);
    }
    KPB_HIP(ctx, hipGetLastError());
    return KPB_OK;
}
