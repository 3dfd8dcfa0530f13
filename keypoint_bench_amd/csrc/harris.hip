// harris.hip -- N13 Harris (models/Harris.py:13-22: cv2.cornerHarris on the wrapped uint8 channel sum) on gfx950: a detector only -- forward returns
// (score, None), dim = 0, and the score is a SIGNED response (edges are negative): detect on it under KPB_OPT_DETECT_SIGNED.
// What is computed is the correctly rounded value of the formula cv2's float32 chain approximates; everything before the last
// line is an integer, so a pixel's bits cannot depend on the tile, the batch size or the position in the batch:
//  1. gray: g = ((c0 + c1) + c2) * 255 in fp32, every operation rounded to nearest and none contracted; truncated toward zero to int32, low 8 bits kept
//     (numpy's float32 -> uint8 cast on x86: a sum above 1 WRAPS, as it does under the configs' gray: false; a negative one wraps from 256 down).
//     A non-finite or huge g gives whatever byte v_cvt_i32_f32's saturation leaves: any byte, no fault.
//  2. Sobel, un-scaled: dx = [1,2,1]^T (x) [-1,0,1], dy its transpose, over reflect-101 of the IMAGE (-1 -> 1, H -> H - 2); |dx|, |dy| <= 1020.
//  3. A = sum dx^2, B = sum dx dy, C = sum dy^2 over rows [y - b/2, y - b/2 + b - 1] and the same columns, b = block_size, over reflect-101 of the PRODUCT
//     planes: a window position outside the frame takes the gradient AT THE REFLECTED pixel (whose own Sobel reflects the image again), which is not a
//     wider stencil on a reflected image.  int32: A <= b^2 1 040 400.
//  4. det = A C - B B and t2 = (A + C)^2 in int64, both below 2^53 for b <= 6 (at b = 7 t2 passes it: refused at create), so their conversion to double is
//     exact; r = ((double)det - (double)k32 * (double)t2) * s4 with k32 = float(k), s = 1 / (4 b 255), s4 = (s s)(s s), every operation rounded to nearest;
//     score = (float)r.
// One kernel, no intermediate in HBM.  A workgroup of 256 takes HR_TH x HR_TW outputs: gray bytes of the tile + halo (b - 1 for the box, 1 for the Sobel)
// in LDS (all of the tile's loads are issued before the first is used); the Sobel pair of every window position, packed as two int16 in one LDS word; the
// box sum separably -- a thread takes one column and 8 vertically adjacent outputs: the row sums of the three products over its 8 + b - 1 window rows into
// registers, then the column sums from them -- the float64 tail, one fp32 store per pixel, a row of 64 per wave.  13 KB of LDS, two barriers.
// block_size is a template parameter: the row and column sums unroll to b adds on registers, with no loop counter and no address arithmetic, and the tile
// dimensions (the divisors of the staging loops) are constants.
#include "net.h"

#include <cmath>

namespace {

constexpr int HR_TH = 32, HR_TW = 64;       // outputs per workgroup; 8 rows x 64 columns per wave

struct HarrisArgs {
    const float* img;       // [B][3][H][W]
    float* score;           // [B][H][W]
    int H, W;
    double k, s4;           // (double)k32, (s s)(s s)
};

// reflect-101, then clamped: what lies further out than one reflection reaches feeds only outputs outside the frame, which are never written
__device__ __forceinline__ int hr_reflect(int v, int n)
{
    v = v < 0 ? -v : v;
    v = v >= n ? 2 * (n - 1) - v : v;
    return min(max(v, 0), n - 1);
}

template <int BS>
__global__ __launch_bounds__(256) void harris_response(HarrisArgs a)
{
    // window position (r, c) <-> pixel (ty0 - AN + r, tx0 - AN + c); gray position (r, c) <-> pixel (ty0 - AN - 1 + r, tx0 - AN - 1 + c)
    constexpr int AN = BS / 2, PH = HR_TH + BS - 1, PW = HR_TW + BS - 1, GH = PH + 2, GW = PW + 2;
    constexpr int RPT = HR_TH / 4, RW = RPT + BS - 1;       // output rows per thread, and the window rows they span
    constexpr int NG = (GH * GW + 255) / 256;
    __shared__ unsigned char g[GH * GW];
    __shared__ int d[PH * PW];              // dx in the low half, dy in the high half
    const kpb_tile3 t = kpb_xcd_tile(1);    // neighbouring tiles re-read each other's halo: on one XCD's L2
    const int tid = threadIdx.x, ty0 = t.y * HR_TH, tx0 = t.x * HR_TW;
    const size_t plane = (size_t)a.H * a.W;
    const float* img = a.img + (size_t)t.z * 3 * plane;
    float v0[NG], v1[NG], v2[NG];           // every load of the tile in flight before the first is used
#pragma unroll
    for (int n = 0; n < NG; ++n) {
        const int i = min(tid + n * 256, GH * GW - 1), r = i / GW, c = i - r * GW;
        const size_t at = (size_t)hr_reflect(ty0 - AN - 1 + r, a.H) * a.W + hr_reflect(tx0 - AN - 1 + c, a.W);
        v0[n] = img[at]; v1[n] = img[plane + at]; v2[n] = img[2 * plane + at];
    }
#pragma unroll
    for (int n = 0; n < NG; ++n) {
        const int i = tid + n * 256;
        const float v = __fmul_rn(__fadd_rn(__fadd_rn(v0[n], v1[n]), v2[n]), 255.0f);
        if (i < GH * GW) g[i] = (unsigned char)((int)v & 255);
    }
    __syncthreads();
    for (int i = tid; i < PH * PW; i += 256) {
        const int r = i / PW, c = i - r * PW;
        // the window position's pixel reflected into the frame (point 3), in tile coordinates: inside the tile for every position a written output uses
        const int rr = min(max(hr_reflect(ty0 - AN + r, a.H) - (ty0 - AN), 0), PH - 1), cc = min(max(hr_reflect(tx0 - AN + c, a.W) - (tx0 - AN), 0), PW - 1);
        const unsigned char* q = g + (rr + 1) * GW + cc + 1;        // the centre
        const int tl = q[-GW - 1], tc = q[-GW], tr = q[-GW + 1], ml = q[-1], mr = q[1], bl = q[GW - 1], bc = q[GW], br = q[GW + 1];
        const int dx = (tr + 2 * mr + br) - (tl + 2 * ml + bl), dy = (bl + 2 * bc + br) - (tl + 2 * tc + tr);
        d[i] = (dx & 0xffff) | (dy * 65536);
    }
    __syncthreads();
    // rows, then columns: the thread's column c, window rows r0 .. r0 + RW - 1 -- the row sums of the three products over columns c .. c + BS - 1 stay in
    // registers (the BS - 1 rows two threads share are summed by both: cheaper than a round trip through LDS and a third barrier)
    const int c = tid & (HR_TW - 1), r0 = (tid / HR_TW) * RPT, gx = tx0 + c;
    int va[RW], vb[RW], vc[RW];
#pragma unroll
    for (int j = 0; j < RW; ++j) {
        int sa = 0, sb = 0, sc = 0;
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            const int v = d[(r0 + j) * PW + c + i], dx = (short)(v & 0xffff), dy = v >> 16;
            sa += dx * dx; sb += dx * dy; sc += dy * dy;
        }
        va[j] = sa; vb[j] = sb; vc[j] = sc;
    }
    float* score = a.score + (size_t)t.z * plane;
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
        int A = 0, B = 0, C = 0;
#pragma unroll
        for (int j = 0; j < BS; ++j) { A += va[o + j]; B += vb[o + j]; C += vc[o + j]; }
        const long long det = (long long)A * C - (long long)B * B, tr = (long long)A + C, t2 = tr * tr;
        const double r = __dmul_rn(__dsub_rn((double)det, __dmul_rn(a.k, (double)t2)), a.s4);
        const int gy = ty0 + r0 + o;
        if (gy < a.H && gx < a.W) score[(size_t)gy * a.W + gx] = __double2float_rn(r);
    }
}

struct Harris : kpb_net {
    int bs = 0;
    float k32 = 0.0f;

    int forward(const float* img, int batch, int H, int W, float* score_out, float* desc_out) override
    {
        (void)desc_out;         // a detector: there is no descriptor map, the pointer may be null
        if (H < 8 || W < 8) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: Harris image %dx%d is smaller than 8x8", H, W);
        if (H > 16384 || W > 16384 || batch > 65535) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: Harris image %dx%d x %d too large", H, W, batch);
        this->B = batch; this->H = H; this->W = W;
        const double s = 1.0 / (4.0 * bs * 255.0);
        HarrisArgs a{img, score_out, H, W, (double)k32, (s * s) * (s * s)};
        const dim3 grid(cdiv(W, HR_TW), cdiv(H, HR_TH), batch);
        switch (bs) {
        case 2: KPB_LAUNCH(ctx, "harris_response", harris_response<2>, grid, dim3(256), 0, ctx->stream, a); break;
        case 3: KPB_LAUNCH(ctx, "harris_response", harris_response<3>, grid, dim3(256), 0, ctx->stream, a); break;
        case 4: KPB_LAUNCH(ctx, "harris_response", harris_response<4>, grid, dim3(256), 0, ctx->stream, a); break;
        case 5: KPB_LAUNCH(ctx, "harris_response", harris_response<5>, grid, dim3(256), 0, ctx->stream, a); break;
        default: KPB_LAUNCH(ctx, "harris_response", harris_response<6>, grid, dim3(256), 0, ctx->stream, a); break;
        }
        KPB_HIP(ctx, hipGetLastError());
        return KPB_OK;
    }
};

}  // namespace

int harris_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out)
{
    const float* plan = KpbwReader{bl, "kpb_net_create: Harris tensor %s missing or mis-shaped"}.need("harris.plan", {3});      // [block_size, ksize, k32]
    const float b = plan[0], ks = plan[1], k = plan[2];
    if (ks != 3.0f) return kpb_fail(ctx, KPB_E_UNSUPPORTED, "kpb_net_create: Harris ksize %g: this build carries the 3 x 3 Sobel only", (double)ks);
    if (!(b >= 2.0f && b <= 6.0f) || b != std::floor(b))
        return kpb_fail(ctx, KPB_E_UNSUPPORTED, "kpb_net_create: Harris block_size %g outside 2 .. 6 (from 7 on (A + C)^2 is no longer exact in float64)", (double)b);
    if (!std::isfinite(k)) return kpb_fail(ctx, KPB_E_UNSUPPORTED, "kpb_net_create: Harris k is not finite");
    auto net = std::make_unique<Harris>();
    net->ctx = ctx; net->arch = KPB_ARCH_HARRIS; net->dim = 0; net->desc_div = 1;
    net->bs = (int)b; net->k32 = k;
    *out = net.release();
    return KPB_OK;
}
