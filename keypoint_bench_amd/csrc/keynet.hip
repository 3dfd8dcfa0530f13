// keynet.hip -- N10 Key.Net (models/KeyNet.py:99-132) on gfx950: a detector only -- forward returns (score, None), dim = 0.  What the reference computes, point
// by point (each one a place where a restatement goes wrong while still looking plausible):
//  1. gray: x = sum over the 3 channels, fp32, [B,1,H,W], values in [0, 3].
//  2. level sizes: level 0 is H x W, level l + 1 is int(h_l // 1.2) x int(w_l // 1.2) (Python float floor division = floor(h / 1.2) in double for every size
//     from 8 to 8192: tests/test_keynet_cpu.py), computed on the host.  Level 2 is a pyrdown of LEVEL 1's gray, not of level 0 (the reference overwrites x).
//  3. custom_pyrdown: 5 x 5 binomial blur [1,4,6,4,1]^T [1,4,6,4,1] / 256 over torch's `reflect` padding (the edge pixel is not repeated: index -1 maps to 1),
//     then F.interpolate(size, 'bilinear', align_corners = False): scale = in / out, src = max((dst + 0.5) scale - 0.5, 0), i0 = floor(src),
//     i1 = min(i0 + 1, in - 1), weight of i1 = src - floor(src) (kpb_tap_hp of interp.h; kn_lin_taps adds its clamps).
//  4. handcrafted block: spatial_gradient = the 3 x 3 Sobel pair / 8 (x kernel [[-1,0,1],[-2,0,2],[-1,0,1]], y its transpose) as correlation over REPLICATE
//     padding; dx, dy = grad(x), dxx, dxy = grad(dx), dyy = grad(dy)[1].  The second gradients replicate the border of dx and dy THEMSELVES, so the outermost
//     ring is not a 5 x 5 stencil on a replicated image: kn_hc_stage keeps, for every position of the tile, the gradient AT THE CLAMPED pixel.
//     Channels: dx, dy, dx^2, dy^2, dx dy, dxy, dxy^2, dxx, dyy, dxx dyy.
//  5. learnable block: three times Conv2d(5 x 5, padding 2, bias) + BatchNorm2d(eval, eps 1e-5) + ReLU, 10 -> 8 -> 8 -> 8, the BatchNorm folded at pack
//     time (weights.py fold_keynet).  The padding is ZERO padding of the feature maps: outside a level's frame the ten features are 0, not computed from a
//     padded image.
//  6. fusion: the 8-channel outputs of levels 1 and 2 go up to H x W by the bilinear rule of point 3, concatenated [level 0 | level 1 | level 2], then
//     Conv2d(24 -> 1, 5 x 5, padding 2, bias) + ReLU.
//  7. the score is non-negative and unbounded (28 .. 14 400 on the 480 x 640 fixture): every operand scale comes from the data.
// Kernels:
//   keynet_pyrdown     gray sum (level 0 only), blur and resize in one pass, fp32: one float per pixel and level
//   keynet_conv5_h     the three 5 x 5 layers as split-f16 MFMA triples with fp32 accumulation.  <HC>: layer 0 -- the ten features are computed from a gray
//                      tile + halo in LDS and go straight into the operand tile, never to HBM; <!HC>: 8 -> 8 on an 8-channel channels-last map.
//                      N = 8 output channels would waste half of v_mfma_f32_16x16x32_f16, so an accumulator row is a PAIR of horizontally adjacent pixels
//                      (alike_block1_h's mapping): M = (pixel of the pair s, output channel), a column = one of the 16 pairs of a 32-pixel row, K = the
//                      window the pair shares, 6 columns x channels in pieces of 8: piece 4 kb + g (g = lane group) of kernel row ky, the weight of window
//                      column wc for pixel s being w[ky][wc - s] (zero outside the kernel).  8 channels: 2 k-blocks per kernel row (pieces 6, 7 empty);
//                      10 channels: two pieces per pixel (the second holds channels 8, 9), 3 k-blocks.  Per tile the operand is scaled by the power of two
//                      that fits its largest magnitude (cm_scale_of), the weights per layer (weight_scale_h).
//   keynet_conv5_f32   KPB_FP32_MATRIX=1: the same layers as plain fp32 fmaf chains, one pixel x 8 channels per thread -- the cross-check, not the product
//   keynet_head        the bilinear upsampling of levels 1 and 2 is evaluated while the tile is staged (the 24-channel concatenation is never written), then
//                      the 24 -> 1 layer, bias and ReLU as fp32 fmaf chains, level by level through one 8-channel LDS tile
#include "conv_mfma.h"

namespace {

typedef _Float16 kn_h8 __attribute__((ext_vector_type(8)));
typedef float kn_f4 __attribute__((ext_vector_type(4)));

constexpr int KN_TH = 16, KN_TW = 32;       // output tile of the layer kernels and the head
constexpr int KN_IH = KN_TH + 4;            // with the 5 x 5 halo

// source taps of output index o under F.interpolate(mode = 'bilinear', align_corners = False) with scale = in / out (point 3)
__device__ __forceinline__ void kn_lin_taps(int o, int n_in, float scale, int& i0, int& i1, float& l)
{
    const kpb_lin t = kpb_tap_hp(o, n_in, scale);
    i0 = min(t.i0, n_in - 1);           // Key.Net's scales are no powers of two: index and weight stay clamped here -- guards that never act (src < in at every scale)
    i1 = min(i0 + 1, n_in - 1);
    l = fminf(fmaxf(t.l, 0.0f), 1.0f);   // the weight of the UNclamped index: the same value wherever the index clamp does not act
}

// the gray value of pixel `at` of one image: the channel sum of a planar 3-channel image (level 0), or the level's own one-channel map
__device__ __forceinline__ float kn_gray(const float* __restrict__ p, int rgb, size_t plane, size_t at)
{
    return rgb ? (p[at] + p[plane + at]) + p[2 * plane + at] : p[at];
}

__device__ __forceinline__ int kn_clamp(int v, int n) { return min(max(v, 0), n - 1); }

// ------------------------------------------------------------------------------------------------ pyrdown
struct KnPyrArgs {
    const float* src;       // [B][3][h][w] (rgb) or [B][h][w]
    float* dst;             // [B][ho][wo]
    int rgb, h, w, ho, wo;
    float sy, sx;           // h / ho, w / wo in fp32, as torch takes them
};
constexpr int KN_PS = 28;   // source rows / columns staged for 16 outputs: 15 x scale (<= 1.3 for h >= 13) + the second tap + the blur's halo of 2 on both sides <= 26

__global__ __launch_bounds__(256) void keynet_pyrdown(KnPyrArgs a)
{
    __shared__ float s[KN_PS][KN_PS + 1];
    const int tid = threadIdx.x, b = blockIdx.z, oy0 = blockIdx.y * 16, ox0 = blockIdx.x * 16;
    const size_t plane = (size_t)a.h * a.w;
    const float* src = a.src + (size_t)b * (a.rgb ? 3 : 1) * plane;
    int by, bx, t1;
    float tl;
    kn_lin_taps(oy0, a.h, a.sy, by, t1, tl);
    kn_lin_taps(ox0, a.w, a.sx, bx, t1, tl);
    by -= 2; bx -= 2;
    for (int i = tid; i < KN_PS * KN_PS; i += 256) {       // reflect padding applied while staging; what lies further out than the blur reaches is clamped
        const int r = i / KN_PS, c = i - r * KN_PS;
        int y = by + r, x = bx + c;
        y = y < 0 ? -y : y; y = y >= a.h ? 2 * (a.h - 1) - y : y; y = kn_clamp(y, a.h);
        x = x < 0 ? -x : x; x = x >= a.w ? 2 * (a.w - 1) - x : x; x = kn_clamp(x, a.w);
        s[r][c] = kn_gray(src, a.rgb, plane, (size_t)y * a.w + x);
    }
    __syncthreads();
    const int oy = oy0 + (tid >> 4), ox = ox0 + (tid & 15);
    if (oy >= a.ho || ox >= a.wo) return;
    int y0, y1, x0, x1;
    float ly, lx;
    kn_lin_taps(oy, a.h, a.sy, y0, y1, ly);
    kn_lin_taps(ox, a.w, a.sx, x0, x1, lx);
    auto blur = [&](int iy, int ix) {
        const int r = min(max(iy - by, 2), KN_PS - 3), c = min(max(ix - bx, 2), KN_PS - 3);       // always inside; the clamp keeps a wrong bound from reading outside
        const float k[5] = {1.0f, 4.0f, 6.0f, 4.0f, 1.0f};
        float acc = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) acc = fmaf(k[dy + 2] * k[dx + 2] * (1.0f / 256.0f), s[r + dy][c + dx], acc);
        return acc;
    };
    const float p00 = blur(y0, x0), p01 = blur(y0, x1), p10 = blur(y1, x0), p11 = blur(y1, x1);
    a.dst[((size_t)b * a.ho + oy) * a.wo + ox] = kpb_mix(p00, p01, p10, p11, ly, lx);
}

// ------------------------------------------------------------------------------------------------ the handcrafted block, on chip
// A tile of FH x FW feature positions, position (r, c) <-> pixel (ty0 - 2 + r, tx0 - 2 + c): the gradients one ring further out, the gray map two.
template <int FW>
struct KnHcTile {
    static constexpr int FH = KN_IH, GH = FH + 4, GW = FW + 4, DH = FH + 2, DW = FW + 2;
    float g[GH * GW];       // gray at the CLAMPED pixel: position (r, c) <-> pixel (ty0 - 4 + r, tx0 - 4 + c)
    float dx[DH * DW];      // d/dx AT THE CLAMPED pixel (replicate padding of dx itself, point 4): position (r, c) <-> pixel (ty0 - 3 + r, tx0 - 3 + c)
    float dy[DH * DW];
};

__device__ __forceinline__ float kn_sobel_x(const float* q, int pitch)     // q: the centre
{
    return 0.125f * (q[-pitch + 1] - q[-pitch - 1]) + 0.25f * (q[1] - q[-1]) + 0.125f * (q[pitch + 1] - q[pitch - 1]);
}
__device__ __forceinline__ float kn_sobel_y(const float* q, int pitch)
{
    return 0.125f * (q[pitch - 1] - q[-pitch - 1]) + 0.25f * (q[pitch] - q[-pitch]) + 0.125f * (q[pitch + 1] - q[-pitch + 1]);
}

template <int FW>
__device__ __forceinline__ void kn_hc_stage(KnHcTile<FW>& t, const float* __restrict__ src, int rgb, int h, int w, int ty0, int tx0, int tid)
{
    typedef KnHcTile<FW> T;
    const size_t plane = (size_t)h * w;
    for (int i = tid; i < T::GH * T::GW; i += 256) {
        const int r = i / T::GW, c = i - r * T::GW;
        t.g[i] = kn_gray(src, rgb, plane, (size_t)kn_clamp(ty0 - 4 + r, h) * w + kn_clamp(tx0 - 4 + c, w));
    }
    __syncthreads();
    for (int i = tid; i < T::DH * T::DW; i += 256) {
        const int r = i / T::DW, c = i - r * T::DW;
        // the clamped pixel in gray-tile coordinates: the tile meets the frame, so it stays one ring inside the gray tile (rows 1 .. GH - 2)
        const int cr = min(max(kn_clamp(ty0 - 3 + r, h) - (ty0 - 4), 1), T::GH - 2), cc = min(max(kn_clamp(tx0 - 3 + c, w) - (tx0 - 4), 1), T::GW - 2);
        const float* q = t.g + cr * T::GW + cc;
        t.dx[i] = kn_sobel_x(q, T::GW);
        t.dy[i] = kn_sobel_y(q, T::GW);
    }
    __syncthreads();
}

// the ten channels at feature position (r, c); zero outside the level's frame (point 5)
template <int FW>
__device__ __forceinline__ void kn_hc_feat(const KnHcTile<FW>& t, int r, int c, bool inside, float* f)
{
    typedef KnHcTile<FW> T;
    const float* qx = t.dx + (r + 1) * T::DW + c + 1;
    const float* qy = t.dy + (r + 1) * T::DW + c + 1;
    const float dx = qx[0], dy = qy[0];
    const float dxx = kn_sobel_x(qx, T::DW), dxy = kn_sobel_y(qx, T::DW), dyy = kn_sobel_y(qy, T::DW);
    const float v[10] = {dx, dy, dx * dx, dy * dy, dx * dy, dxy, dxy * dxy, dxx, dyy, dxx * dyy};
#pragma unroll
    for (int j = 0; j < 10; ++j) f[j] = inside ? v[j] : 0.0f;
}

// ------------------------------------------------------------------------------------------------ the 5 x 5 layers
struct KnConvArgs {
    const float* src;       // HC: the level's gray map [B][h][w] (level 0: the image [B][3][h][w], rgb = 1); else [B][h][w][8]
    float* out;             // [B][h][w][8]
    const uint4* wpk;       // split-f16: [5 KBR][hi / lo][64 lanes] fragments (kn_pack_h16), scaled by 1 / inv_ws
    const float* wf;        // strict fp32: [25 taps][4 NQ channels][8] (kn_pack_f32)
    const float* bias;      // [8]
    float inv_ws;
    int rgb, h, w;
};

template <bool HC>
__global__ __launch_bounds__(256) void keynet_conv5_h(KnConvArgs a)
{
    // PP pieces of 8 channels per pixel; KBR k-blocks of 4 pieces per kernel row; the plain tile is two columns wider so that the empty pieces 6, 7 read staged data
    constexpr int PP = HC ? 2 : 1, KBR = HC ? 3 : 2, KB = 5 * KBR, IH = KN_IH, IW = HC ? KN_TW + 4 : KN_TW + 6, NPOS = IH * IW, PER = (NPOS + 255) / 256;
    __shared__ __attribute__((aligned(16))) uint4 sp[2 * NPOS * PP];       // [hi | lo][position][piece]
    __shared__ float s_amax[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.z, ty0 = blockIdx.y * KN_TH, tx0 = blockIdx.x * KN_TW;
    kn_h8 whi[KB], wlo[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        whi[kb] = __builtin_bit_cast(kn_h8, a.wpk[(kb * 2 + 0) * 64 + lane]);
        wlo[kb] = __builtin_bit_cast(kn_h8, a.wpk[(kb * 2 + 1) * 64 + lane]);
    }
    const float4 bias = *reinterpret_cast<const float4*>(a.bias + 4 * ((lane >> 4) & 1));
    float v[PER][8 * PP];
    float am = 0.0f;
    if constexpr (HC) {
        __shared__ KnHcTile<IW> t;
        kn_hc_stage(t, a.src + (size_t)b * (a.rgb ? 3 : 1) * a.h * a.w, a.rgb, a.h, a.w, ty0, tx0, tid);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * 256, r = min(i / IW, IH - 1), c = i - (i / IW) * IW;
            const int gy = ty0 - 2 + r, gx = tx0 - 2 + c;
            kn_hc_feat(t, r, c, i < NPOS && gy >= 0 && gy < a.h && gx >= 0 && gx < a.w, v[k]);
#pragma unroll
            for (int j = 10; j < 16; ++j) v[k][j] = 0.0f;
#pragma unroll
            for (int j = 0; j < 10; ++j) am = fmaxf(am, fabsf(v[k][j]));
        }
    } else {
        const float* in = a.src + (size_t)b * a.h * a.w * 8;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * 256, r = i / IW, c = i - r * IW;
            const int gy = ty0 - 2 + r, gx = tx0 - 2 + c;
            const bool inside = i < NPOS && gy >= 0 && gy < a.h && gx >= 0 && gx < a.w;
            float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
            if (inside) {
                const float4* p = reinterpret_cast<const float4*>(in + ((size_t)gy * a.w + gx) * 8);
                q0 = p[0]; q1 = p[1];
            }
            v[k][0] = q0.x; v[k][1] = q0.y; v[k][2] = q0.z; v[k][3] = q0.w; v[k][4] = q1.x; v[k][5] = q1.y; v[k][6] = q1.z; v[k][7] = q1.w;
            am = cm_amax4(cm_amax4(am, q0), q1);
        }
    }
    am = cm_wave_max(am);
    if (lane == 0) s_amax[wv] = am;
    __syncthreads();
    const int e = cm_exp_of(fmaxf(fmaxf(s_amax[0], s_amax[1]), fmaxf(s_amax[2], s_amax[3])));       // the tile's own largest magnitude: the same bits alone or in a batch
    const float sc = cm_scale_of(e), un = a.inv_ws * cm_unscale_of(e);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = tid + k * 256;
        if (i < NPOS) {
#pragma unroll
            for (int p = 0; p < PP; ++p) {
                uint2 h0, l0, h1, l1;
                cm_split4(make_float4(v[k][8 * p] * sc, v[k][8 * p + 1] * sc, v[k][8 * p + 2] * sc, v[k][8 * p + 3] * sc), h0, l0);
                cm_split4(make_float4(v[k][8 * p + 4] * sc, v[k][8 * p + 5] * sc, v[k][8 * p + 6] * sc, v[k][8 * p + 7] * sc), h1, l1);
                sp[i * PP + p] = make_uint4(h0.x, h0.y, h1.x, h1.y);
                sp[NPOS * PP + i * PP + p] = make_uint4(l0.x, l0.y, l1.x, l1.y);
            }
        }
    }
    __syncthreads();
    // D^T = W^T A^T: the weight fragment is the MFMA's A operand, the pieces are B; lane (pair pr, group g) ends with channels 4 (g & 1) .. + 3 of pixel g >> 1 of its pair
    const int pr = lane & 15, g = lane >> 4, sN = g >> 1, c0 = 4 * (g & 1);
    const int gx = tx0 + 2 * pr + sN;
    float* out = a.out + (size_t)b * a.h * a.w * 8;
#pragma unroll 1
    for (int rr = 0; rr < KN_TH / 4; ++rr) {
        const int row = (KN_TH / 4) * wv + rr;
        kn_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 5; ++ky)
#pragma unroll
            for (int kb = 0; kb < KBR; ++kb) {
                const int piece = 4 * kb + g;                                      // window column piece / PP, channels 8 (piece % PP) .. + 7
                const int at = ((row + ky) * IW + 2 * pr + piece / PP) * PP + piece % PP;
                const kn_h8 ihi = __builtin_bit_cast(kn_h8, sp[at]), ilo = __builtin_bit_cast(kn_h8, sp[NPOS * PP + at]);
                const int k = ky * KBR + kb;
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(whi[k], ilo, acc, 0, 0, 0);      // small terms first
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wlo[k], ihi, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(whi[k], ihi, acc, 0, 0, 0);
            }
        const int gy = ty0 + row;
        if (gy < a.h && gx < a.w)
            *reinterpret_cast<float4*>(out + ((size_t)gy * a.w + gx) * 8 + c0) =
                make_float4(relu(fmaf(acc[0], un, bias.x)), relu(fmaf(acc[1], un, bias.y)), relu(fmaf(acc[2], un, bias.z)), relu(fmaf(acc[3], un, bias.w)));
    }
}

// KPB_FP32_MATRIX=1.  Thread (ty, tx) takes pixels (ty, tx) and (ty + 8, tx) of the tile, 8 output channels each; the weights are wave-uniform.
template <bool HC>
__global__ __launch_bounds__(256) void keynet_conv5_f32(KnConvArgs a)
{
    constexpr int NQ = HC ? 3 : 2, IH = KN_IH, IW = KN_TW + 4, NPOS = IH * IW;
    __shared__ __attribute__((aligned(16))) float4 sf[NQ * NPOS];       // [channel quad][position]
    const int tid = threadIdx.x, b = blockIdx.z, ty0 = blockIdx.y * KN_TH, tx0 = blockIdx.x * KN_TW;
    if constexpr (HC) {
        __shared__ KnHcTile<IW> t;
        kn_hc_stage(t, a.src + (size_t)b * (a.rgb ? 3 : 1) * a.h * a.w, a.rgb, a.h, a.w, ty0, tx0, tid);
        for (int i = tid; i < NPOS; i += 256) {
            const int r = i / IW, c = i - r * IW, gy = ty0 - 2 + r, gx = tx0 - 2 + c;
            float f[12];
            kn_hc_feat(t, r, c, gy >= 0 && gy < a.h && gx >= 0 && gx < a.w, f);
            f[10] = f[11] = 0.0f;
#pragma unroll
            for (int q = 0; q < 3; ++q) sf[q * NPOS + i] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
        }
    } else {
        const float* in = a.src + (size_t)b * a.h * a.w * 8;
        for (int i = tid; i < NPOS; i += 256) {
            const int r = i / IW, c = i - r * IW, gy = ty0 - 2 + r, gx = tx0 - 2 + c;
            float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
            if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w) {
                const float4* p = reinterpret_cast<const float4*>(in + ((size_t)gy * a.w + gx) * 8);
                q0 = p[0]; q1 = p[1];
            }
            sf[i] = q0; sf[NPOS + i] = q1;
        }
    }
    __syncthreads();
    const int tx = tid & 31, ty = tid >> 5;
    float acc[2][8];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[0][o] = acc[1][o] = a.bias[o];
#pragma unroll 1
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float4 v0 = sf[q * NPOS + (ty + ky) * IW + tx + kx], v1 = sf[q * NPOS + (ty + 8 + ky) * IW + tx + kx];
                const float* w = a.wf + ((ky * 5 + kx) * NQ * 4 + q * 4) * 8;
                const float x0[4] = {v0.x, v0.y, v0.z, v0.w}, x1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int o = 0; o < 8; ++o) {
                        acc[0][o] = fmaf(x0[c], w[c * 8 + o], acc[0][o]);
                        acc[1][o] = fmaf(x1[c], w[c * 8 + o], acc[1][o]);
                    }
            }
    const int gx = tx0 + tx;
    float* out = a.out + (size_t)b * a.h * a.w * 8;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int gy = ty0 + ty + 8 * p;
        if (gy < a.h && gx < a.w) {
            float4* o = reinterpret_cast<float4*>(out + ((size_t)gy * a.w + gx) * 8);
            o[0] = make_float4(relu(acc[p][0]), relu(acc[p][1]), relu(acc[p][2]), relu(acc[p][3]));
            o[1] = make_float4(relu(acc[p][4]), relu(acc[p][5]), relu(acc[p][6]), relu(acc[p][7]));
        }
    }
}

// ------------------------------------------------------------------------------------------------ fusion
struct KnHeadArgs {
    const float* f0; const float* f1; const float* f2;      // the three levels' outputs [B][h_l][w_l][8]
    float* score;           // [B][H][W]
    const float* w;         // [3 levels][25 taps][8]
    float bias;
    int H, W, h1, w1, h2, w2;
    float sy1, sx1, sy2, sx2;       // h_l / H, w_l / W in fp32
};

__global__ __launch_bounds__(256) void keynet_head(KnHeadArgs a)
{
    constexpr int IH = KN_IH, IW = KN_TW + 4, NPOS = IH * IW;
    __shared__ __attribute__((aligned(16))) float4 sf[2 * NPOS];        // one level's 8 channels: [channel quad][position]
    const int tid = threadIdx.x, b = blockIdx.z, ty0 = blockIdx.y * KN_TH, tx0 = blockIdx.x * KN_TW;
    const int tx = tid & 31, ty = tid >> 5;
    float acc0 = a.bias, acc1 = a.bias;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const int hl = l == 0 ? a.H : l == 1 ? a.h1 : a.h2, wl = l == 0 ? a.W : l == 1 ? a.w1 : a.w2;
        const float sy = l == 1 ? a.sy1 : a.sy2, sx = l == 1 ? a.sx1 : a.sx2;
        const float* src = (l == 0 ? a.f0 : l == 1 ? a.f1 : a.f2) + (size_t)b * hl * wl * 8;
        if (l) __syncthreads();
        for (int i = tid; i < NPOS; i += 256) {
            const int r = i / IW, c = i - r * IW, gy = ty0 - 2 + r, gx = tx0 - 2 + c;
            float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;       // zero padding of the concatenated map
            if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
                if (l == 0) {
                    const float4* p = reinterpret_cast<const float4*>(src + ((size_t)gy * wl + gx) * 8);
                    q0 = p[0]; q1 = p[1];
                } else {
                    int y0, y1, x0, x1;
                    float ly, lx;
                    kn_lin_taps(gy, hl, sy, y0, y1, ly);
                    kn_lin_taps(gx, wl, sx, x0, x1, lx);
                    const float4* p00 = reinterpret_cast<const float4*>(src + ((size_t)y0 * wl + x0) * 8);
                    const float4* p01 = reinterpret_cast<const float4*>(src + ((size_t)y0 * wl + x1) * 8);
                    const float4* p10 = reinterpret_cast<const float4*>(src + ((size_t)y1 * wl + x0) * 8);
                    const float4* p11 = reinterpret_cast<const float4*>(src + ((size_t)y1 * wl + x1) * 8);
                    q0 = kpb_mix4(p00[0], p01[0], p10[0], p11[0], ly, lx);
                    q1 = kpb_mix4(p00[1], p01[1], p10[1], p11[1], ly, lx);
                }
            }
            sf[i] = q0; sf[NPOS + i] = q1;
        }
        __syncthreads();
        // the thread's two pixels are vertically adjacent: tile row 2 ty + r is kernel row r of the upper one and r - 1 of the lower one, read once for both
        // (the kernel is bound by these LDS reads); each pixel still accumulates in the order (level, ky, kx, channel)
#pragma unroll 1
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const int at = (2 * ty + r) * IW + tx + kx;
                const float4 u0 = sf[at], u1 = sf[NPOS + at];
                if (r < 5) {
                    const float* w = a.w + ((l * 25 + r * 5 + kx) * 8);
                    acc0 = fmaf(u0.x, w[0], acc0); acc0 = fmaf(u0.y, w[1], acc0); acc0 = fmaf(u0.z, w[2], acc0); acc0 = fmaf(u0.w, w[3], acc0);
                    acc0 = fmaf(u1.x, w[4], acc0); acc0 = fmaf(u1.y, w[5], acc0); acc0 = fmaf(u1.z, w[6], acc0); acc0 = fmaf(u1.w, w[7], acc0);
                }
                if (r > 0) {
                    const float* w = a.w + ((l * 25 + (r - 1) * 5 + kx) * 8);
                    acc1 = fmaf(u0.x, w[0], acc1); acc1 = fmaf(u0.y, w[1], acc1); acc1 = fmaf(u0.z, w[2], acc1); acc1 = fmaf(u0.w, w[3], acc1);
                    acc1 = fmaf(u1.x, w[4], acc1); acc1 = fmaf(u1.y, w[5], acc1); acc1 = fmaf(u1.z, w[6], acc1); acc1 = fmaf(u1.w, w[7], acc1);
                }
            }
    }
    const int gx = tx0 + tx, gy = ty0 + 2 * ty;
    float* score = a.score + (size_t)b * a.H * a.W;
    if (gx < a.W && gy < a.H) score[(size_t)gy * a.W + gx] = relu(acc0);
    if (gx < a.W && gy + 1 < a.H) score[(size_t)(gy + 1) * a.W + gx] = relu(acc1);
}

// ------------------------------------------------------------------------------------------------ host
// OIHW [8][CIN][5][5] -> keynet_conv5_h fragments [5 KBR][hi / lo][64 lanes][8 halves]: lane (n = (s, cout), g), piece 4 kb + g = (window column wc, channel
// half) = (piece / PP, piece % PP); element j = channel 8 half + j: w[cout][cin][ky][wc - s], zero outside the kernel, past CIN and for window columns >= 6
std::vector<float> kn_pack_h16(const float* w, int CIN, int PP, int KBR, float scale)
{
    return pack_lanes_h16(5 * KBR, [&](int k, int l, int j) {
        const int ky = k / KBR, kb = k % KBR, n = l & 15, g = l >> 4, s2 = n >> 3, co = n & 7, piece = 4 * kb + g;
        const int wc = piece / PP, cin = 8 * (piece % PP) + j, kx = wc - s2;
        return (wc < 6 && cin < CIN && kx >= 0 && kx <= 4) ? w[(((size_t)co * CIN + cin) * 5 + ky) * 5 + kx] * scale : 0.0f;
    });
}

// OIHW [8][CIN][5][5] -> [25 taps][4 NQ channels][8 output channels], zero past CIN
std::vector<float> kn_pack_f32(const float* w, int CIN, int NQ)
{
    std::vector<float> p((size_t)25 * NQ * 4 * 8, 0.0f);
    for (int t = 0; t < 25; ++t)
        for (int c = 0; c < CIN; ++c)
            for (int o = 0; o < 8; ++o) p[((size_t)t * NQ * 4 + c) * 8 + o] = w[((size_t)o * CIN + c) * 25 + t];
    return p;
}

struct KeyNet : kpb_net {
    struct Layer { const uint4* wpk = nullptr; const float* wf = nullptr; const float* b = nullptr; float inv_ws = 1.0f; } lay[3];
    const float* head_w = nullptr;
    float head_b = 0.0f;
    bool h16 = true;

    template <bool HC> void conv(const char* tag, const Layer& L, const float* src, float* out, int rgb, int batch, int h, int w)
    {
        KnConvArgs a{src, out, L.wpk, L.wf, L.b, L.inv_ws, rgb, h, w};
        const dim3 grid(cdiv(w, KN_TW), cdiv(h, KN_TH), batch);
        if (h16) KPB_LAUNCH(ctx, tag, keynet_conv5_h<HC>, grid, dim3(256), 0, ctx->stream, a);
        else KPB_LAUNCH(ctx, tag, keynet_conv5_f32<HC>, grid, dim3(256), 0, ctx->stream, a);
    }

    int forward(const float* img, int batch, int H, int W, float* score_out, float* desc_out) override
    {
        (void)desc_out;         // a detector: there is no descriptor map, the pointer may be null
        if (H < 16 || W < 16) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: KeyNet image %dx%d is smaller than 16x16", H, W);
        if (H > 16384 || W > 16384 || batch > 65535) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: KeyNet image %dx%d x %d too large", H, W, batch);
        int h[3] = {H, 0, 0}, w[3] = {W, 0, 0};
        for (int l = 0; l < 2; ++l) {       // point 2, in double
            h[l + 1] = (int)std::floor((double)h[l] / 1.2);
            w[l + 1] = (int)std::floor((double)w[l] / 1.2);
        }
        const size_t B = batch;
        float* gray[3] = {nullptr, nullptr, nullptr};
        float* fa[3];
        float* fb[3];
        if (int rc = kpb_carve(ctx, act, [&](Arena& a) {
                for (int l = 0; l < 3; ++l) {
                    const size_t P = (size_t)h[l] * w[l];
                    if (l) gray[l] = a.take(B * P);
                    fa[l] = a.take(B * P * 8);
                    fb[l] = a.take(B * P * 8);
                }
            })) return rc;
        this->B = batch; this->H = H; this->W = W;
        hipStream_t st = ctx->stream;
        for (int l = 0; l < 2; ++l) {
            KnPyrArgs p{l ? gray[1] : img, gray[l + 1], l == 0, h[l], w[l], h[l + 1], w[l + 1], (float)h[l] / (float)h[l + 1], (float)w[l] / (float)w[l + 1]};
            KPB_LAUNCH(ctx, "keynet_pyrdown", keynet_pyrdown, dim3(cdiv(w[l + 1], 16), cdiv(h[l + 1], 16), batch), dim3(256), 0, st, p);
        }
        for (int l = 0; l < 3; ++l) {
            conv<true>("keynet_level_hc", lay[0], l ? gray[l] : img, fa[l], l == 0, batch, h[l], w[l]);
            conv<false>("keynet_conv5", lay[1], fa[l], fb[l], 0, batch, h[l], w[l]);
            conv<false>("keynet_conv5", lay[2], fb[l], fa[l], 0, batch, h[l], w[l]);
        }
        KnHeadArgs ha{fa[0], fa[1], fa[2], score_out, head_w, head_b, H, W, h[1], w[1], h[2], w[2],
                      (float)h[1] / (float)H, (float)w[1] / (float)W, (float)h[2] / (float)H, (float)w[2] / (float)W};
        KPB_LAUNCH(ctx, "keynet_head", keynet_head, dim3(cdiv(W, KN_TW), cdiv(H, KN_TH), batch), dim3(256), 0, st, ha);
        KPB_HIP(ctx, hipGetLastError());
        return KPB_OK;
    }
};

}  // namespace

int keynet_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out)
{
    auto net = std::make_unique<KeyNet>();
    net->ctx = ctx; net->arch = KPB_ARCH_KEYNET; net->dim = 0; net->desc_div = 1;
    net->h16 = conv_mfma_use_h16();
    WeightStage ws;
    const KpbwReader rd{bl, "kpb_net_create: KeyNet tensor %s missing or mis-shaped"};
    for (int i = 0; i < 3; ++i) {
        const int cin = i ? 8 : 10;
        const std::string name = "l" + std::to_string(i);
        const float* w = rd.need(name + ".w", {8, (uint32_t)cin, 5, 5});
        const float* b = rd.need(name + ".b", {8});
        KeyNet::Layer& L = net->lay[i];
        if (net->h16) {
            const float sc = weight_scale_h(w, (size_t)8 * cin * 25);
            ws.put(kn_pack_h16(w, cin, i ? 1 : 2, i ? 2 : 3, sc), &L.wpk);
            L.inv_ws = 1.0f / sc;
        } else {
            ws.put(kn_pack_f32(w, cin, i ? 2 : 3), &L.wf);
        }
        ws.put_raw(b, 8, &L.b);
    }
    const float* lw = rd.need("last.w", {1, 24, 5, 5});
    const float* lb = rd.need("last.b", {1});
    std::vector<float> hw((size_t)3 * 25 * 8);
    for (int l = 0; l < 3; ++l)
        for (int t = 0; t < 25; ++t)
            for (int c = 0; c < 8; ++c) hw[((size_t)l * 25 + t) * 8 + c] = lw[((size_t)l * 8 + c) * 25 + t];
    ws.put(hw, &net->head_w);
    net->head_b = lb[0];
    if (int rc = ws.upload(ctx, &net->wdev)) return rc;
    *out = net.release();
    return KPB_OK;
}
