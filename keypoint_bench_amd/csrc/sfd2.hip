// sfd2.hip -- N11 SFD2 (models/sfd2.py:90-185, ResSegNetV2(outdim = 128, require_stability = True)) on gfx950.  What the reference computes:
//  1. trunk: conv1a 3 -> 64, conv1b 64 -> 64 / 2, conv2a 64 -> 128, conv2b 128 -> 128 / 2, conv3a 128 -> 256, conv3b 256 -> 256, all 3 x 3 with bias, eval-mode
//     BatchNorm (eps 1e-5) and ReLU behind each (the BatchNorms are folded at pack time, weights.py fold_sfd2).
//  2. conv4: three ResBlocks at 1/4 resolution, each 1 x 1 -> BN -> ReLU, 3 x 3 in 32 GROUPS of 8 channels -> BN -> ReLU, 1 x 1 -> BN, + identity -> ReLU.
//  3. detector: convPa.0 256 -> 256 / 2 + BN + ReLU, convPa.3 256 -> 256 (NO ReLU), convPb 256 -> 65 at 1/8 resolution; semi = exp(logits) WITHOUT a maximum
//     subtracted, semi / (sum of the 65 + 1e-5), channel 64 dropped, depth-to-space 8 x 8.
//  4. descriptors: convDa.0 + BN + ReLU, convDa.3 (no ReLU), convDb 256 -> 128, F.normalize(dim = 1, eps 1e-12): a 128-channel map at 1/4 RESOLUTION (desc_div 4).
//  5. stability: ConvSta 256 -> 3 on out4, F.interpolate(size = (H, W), 'bilinear', align_corners = False) -- source coordinate (d + 0.5) / 4 - 0.5 clamped at 0,
//     neighbours clamped at the edge --, argmax over the three (the first maximum wins), classes 0 / 1 / 2 -> 0.1 / 0.5 / 1.0; score = semi_norm x stability.
//     H and W must be multiples of 8: the reference's own product fails on mismatched shapes otherwise.
// Kernels:
//   conv1a_rgb64       (conv_layer.h, shared with D2-Net) 3 -> 64 at full resolution on the vector ALU from the planar image
//   conv_mfma_h        the 3 x 3 layers at stride 1 and 2 (SuperPoint's forms); KPB_FP32_MATRIX=1: conv_mfma
//   gemm_h             the 1 x 1 layers; <GE_RES_RELU> adds the ResBlock's identity tile before the ReLU.  KPB_FP32_MATRIX=1: conv_mfma's 1 x 1 form with ConvM::res
//   sfd2_gconv_f32     the grouped 3 x 3 as strict fp32 fmaf chains: a thread takes one pixel and four groups in turn, the 9 x 8 x 8 weights of a group wave-uniform
//   sfd2_gconv_h       the grouped 3 x 3 as split-f16 v_mfma_f32_16x16x32_f16 triples: M = 16 output channels (two groups), N = 16 pixels of a row, K = 4 lane
//                      blocks of 8 = (tap 2 k, group 0), (tap 2 k, group 1), (tap 2 k + 1, group 0), (tap 2 k + 1, group 1): five instructions for the nine taps,
//                      the weights of the other group's rows zero (half of the weight operand).  Operand scale per tile (cm_scale_of), weights per layer.
//   sfd2_score         one wave per 8 x 8 cell: exp, guarded sum, depth-to-space, the x 4 bilinear of the three stability logits, argmax and the product; no
//                      full-resolution stability map is written
//   l2norm_nhwc        (convnet.hip) F.normalize of the 128-channel rows in place, eps_clamp 1e-12
// The dense layers are Layers staged and launched by conv_layer.h's stage_layer / launch_mfma; conv_mfma.h is here for cm_split4 and friends of the grouped kernel.
#include "conv_layer.h"
#include "conv_mfma.h"

namespace {

typedef float sf_f4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ the grouped 3 x 3 layer (256 channels, 32 groups of 8 -> 8)
struct SfGcArgs {
    const float* in;        // [B][H][W][256]
    float* out;             // [B][H][W][256]
    const float* wf;        // strict fp32: [32 groups][9 taps][8 cin][8 cout]
    const uint4* wpk;       // split-f16: [16 slices][5 k][hi / lo][64 lanes] fragments (sf_pack_gconv_h16), scaled by 1 / inv_ws
    const float* bias;      // [256]
    float inv_ws;
    int H, W;
};

// Strict fp32, and the yardstick of the matrix form: a thread = one pixel, the four groups of blockIdx.y in turn; per group bias, then the taps in (ky, kx, cin)
// order, an fma each; a tap outside the image is skipped as the zero it is (fmaf(0, w, acc) = acc for finite w).
__global__ __launch_bounds__(256) void sfd2_gconv_f32(SfGcArgs a)
{
    const int b = blockIdx.z, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= a.H * a.W) return;
    const int oy = pix / a.W, ox = pix - oy * a.W;
    const float* in = a.in + (size_t)b * a.H * a.W * 256;
    float* out = a.out + ((size_t)b * a.H * a.W + pix) * 256;
#pragma unroll 1
    for (int gi = 0; gi < 4; ++gi) {
        const int g = blockIdx.y * 4 + gi;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = a.bias[g * 8 + j];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = oy + ky - 1, ix = ox + kx - 1;
                const bool inside = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                const float4* src = reinterpret_cast<const float4*>(in + ((size_t)(inside ? iy : 0) * a.W + (inside ? ix : 0)) * 256 + g * 8);
                const float4 q0 = src[0], q1 = src[1];
                const float v[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                const float* w = a.wf + ((size_t)(g * 9 + ky * 3 + kx) * 8) * 8;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float vc = inside ? v[c] : 0.0f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaf(vc, w[c * 8 + j], acc[j]);
                }
            }
        float4* o = reinterpret_cast<float4*>(out + g * 8);
        o[0] = make_float4(relu(acc[0]), relu(acc[1]), relu(acc[2]), relu(acc[3]));
        o[1] = make_float4(relu(acc[4]), relu(acc[5]), relu(acc[6]), relu(acc[7]));
    }
}

// Split-f16 matrix form.  Workgroup = 16 x 16 pixels x 32 channels (four groups = two 16-channel slices); the 18 x 18 x 32 input tile goes to LDS split into
// halves at the scale of its own largest magnitude: [hi | lo][position][4 groups + 1 pad] slots of 16 bytes (8 halves = one group of one pixel; the odd pitch keeps
// the 16 pixels of a read apart).  Wave wv owns tile rows 4 wv .. + 3.  For slice s the MFMA's A operand is the weight fragment (row = output channel of the slice),
// B the pixels: lane (n, g) reads group 2 s + (g & 1) of pixel n at tap 2 k + (g >> 1) and ends with channels 4 g .. + 3 of the slice at pixel n.
constexpr int GC_T = 16, GC_I = GC_T + 2, GC_NPOS = GC_I * GC_I, GC_PITCH = 5;
__global__ __launch_bounds__(256) void sfd2_gconv_h(SfGcArgs a)
{
    constexpr int NLD = GC_NPOS * 8, PER = (NLD + 255) / 256, REG = GC_NPOS * GC_PITCH;
    __shared__ __attribute__((aligned(16))) uint4 sp[2 * REG];
    __shared__ float s_amax[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.z >> 3, cq = blockIdx.z & 7, ty0 = blockIdx.y * GC_T, tx0 = blockIdx.x * GC_T;
    const float* in = a.in + (size_t)b * a.H * a.W * 256 + cq * 32;
    float4 ld[PER];
    float am = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = tid + k * 256, pos = i >> 3, q = i & 7, r = pos / GC_I, c = pos - r * GC_I;
        const int gy = ty0 - 1 + r, gx = tx0 - 1 + c;
        const bool ok = i < NLD && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;       // zero padding
        ld[k] = ok ? *reinterpret_cast<const float4*>(in + ((size_t)gy * a.W + gx) * 256 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        am = cm_amax4(am, ld[k]);
    }
    am = cm_wave_max(am);
    if (lane == 0) s_amax[wv] = am;
    __syncthreads();
    const int e = cm_exp_of(fmaxf(fmaxf(s_amax[0], s_amax[1]), fmaxf(s_amax[2], s_amax[3])));       // the tile's own largest magnitude: the same bits alone or in a batch
    const float sc = cm_scale_of(e), un = a.inv_ws * cm_unscale_of(e);
    uint2* sph = reinterpret_cast<uint2*>(sp);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = tid + k * 256, pos = i >> 3, q = i & 7;
        uint2 hi, lo;
        cm_split4(make_float4(ld[k].x * sc, ld[k].y * sc, ld[k].z * sc, ld[k].w * sc), hi, lo);
        if (i < NLD) {
            const int at = (pos * GC_PITCH + (q >> 1)) * 2 + (q & 1);
            sph[at] = hi;
            sph[2 * REG + at] = lo;
        }
    }
    __syncthreads();
    const int n = lane & 15, g = lane >> 4;
    int off[5];         // tap 2 k + (g >> 1) of this lane's k-block; the tenth tap does not exist: its weights are zero and it re-reads the ninth
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int t = min(2 * k + (g >> 1), 8), ky = t / 3, kx = t - 3 * ky;
        off[k] = (ky * GC_I + kx + n) * GC_PITCH + (g & 1);
    }
    const int gx = tx0 + n;
    float* out = a.out + (size_t)b * a.H * a.W * 256;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
        const int sl = cq * 2 + s;
        cm_h8 wh[5], wl[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            wh[k] = __builtin_bit_cast(cm_h8, a.wpk[((sl * 5 + k) * 2 + 0) * 64 + lane]);
            wl[k] = __builtin_bit_cast(cm_h8, a.wpk[((sl * 5 + k) * 2 + 1) * 64 + lane]);
        }
        const float4 bias = *reinterpret_cast<const float4*>(a.bias + sl * 16 + 4 * g);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = 4 * wv + rr, base = row * GC_I * GC_PITCH + 2 * s;
            sf_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const cm_h8 ihi = __builtin_bit_cast(cm_h8, sp[base + off[k]]), ilo = __builtin_bit_cast(cm_h8, sp[REG + base + off[k]]);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[k], ilo, acc, 0, 0, 0);      // small terms first
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[k], ihi, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[k], ihi, acc, 0, 0, 0);
            }
            const int gy = ty0 + row;
            if (gy < a.H && gx < a.W)
                *reinterpret_cast<float4*>(out + ((size_t)gy * a.W + gx) * 256 + sl * 16 + 4 * g) =
                    make_float4(relu(fmaf(acc[0], un, bias.x)), relu(fmaf(acc[1], un, bias.y)), relu(fmaf(acc[2], un, bias.z)), relu(fmaf(acc[3], un, bias.w)));
        }
    }
}

// ------------------------------------------------------------------------------------------------ score head
// One wave per cell, lane c = logit c = pixel (c >> 3, c & 7) of the cell; SF_PXW cells per wave with their loads in flight together (softmax65_d2s).
constexpr int SF_PXW = 4;
__global__ __launch_bounds__(256) void sfd2_score(const float* __restrict__ semi /*[B][Hc][Wc][65]*/, const float* __restrict__ sta /*[B][2 Hc][2 Wc][3]*/,
                                                   float* __restrict__ score /*[B][8 Hc][8 Wc]*/, int Hc, int Wc)
{
    const int lane = threadIdx.x & 63, b = blockIdx.y, ncell = Hc * Wc;
    const int cell0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * SF_PXW;
    if (cell0 >= ncell) return;
    const int H4 = 2 * Hc, W4 = 2 * Wc, W = 8 * Wc;
    float v[SF_PXW], d[SF_PXW];
#pragma unroll
    for (int i = 0; i < SF_PXW; ++i) {
        const float* s = semi + ((size_t)b * ncell + min(cell0 + i, ncell - 1)) * 65;
        v[i] = s[lane]; d[i] = s[64];
    }
    const float* st = sta + (size_t)b * H4 * W4 * 3;
#pragma unroll
    for (int i = 0; i < SF_PXW; ++i) {
        const int cell = cell0 + i;
        if (cell >= ncell) break;       // wave-uniform
        const int cy = cell / Wc, cx = cell - cy * Wc, py = cy * 8 + (lane >> 3), px = cx * 8 + (lane & 7);
        // stability class of pixel (py, px): the three logits upsampled x 4 (point 5), first maximum
        const kpb_lin ty = kpb_tap_hp(py, H4, 0.25f), tx = kpb_tap_hp(px, W4, 0.25f);
        const float* p00 = st + ((size_t)ty.i0 * W4 + tx.i0) * 3;
        const float* p01 = st + ((size_t)ty.i0 * W4 + tx.i1) * 3;
        const float* p10 = st + ((size_t)ty.i1 * W4 + tx.i0) * 3;
        const float* p11 = st + ((size_t)ty.i1 * W4 + tx.i1) * 3;
        float l[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) l[c] = kpb_mix(p00[c], p01[c], p10[c], p11[c], ty.l, tx.l);
        float stab = 0.1f, best = l[0];
        if (l[1] > best) { best = l[1]; stab = 0.5f; }
        if (l[2] > best) stab = 1.0f;
        // exp WITHOUT a maximum subtracted, the sum guarded by 1e-5 (point 3)
        const float ev = expf(v[i]), ed = expf(d[i]);
        const float sum = kpb_wave_sum(ev) + ed;
        score[((size_t)b * 8 * Hc + py) * W + px] = __fdiv_rn(ev, sum + 1e-5f) * stab;
    }
}

// the probe of KPB_OPT_SFD2_PROBE: channels c0 .. c0 + 127 of a 256-channel map into a 128-channel one
__global__ void sfd2_take128(const float* __restrict__ src, float* __restrict__ dst, size_t npix, int c0)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix * 32) return;
    const size_t pix = i >> 5;
    const int q = (int)(i & 31);
    reinterpret_cast<float4*>(dst + pix * 128)[q] = reinterpret_cast<const float4*>(src + pix * 256 + c0)[q];
}

// ------------------------------------------------------------------------------------------------ host
enum { SF_1A, SF_1B, SF_2A, SF_2B, SF_3A, SF_3B, SF_R0, SF_PA0 = SF_R0 + 9, SF_PA3, SF_PB, SF_DA0, SF_DA3, SF_DB, SF_STA, SF_LAYERS };      // sfd2_create's plan order

// OIHW [256][8][3][3] -> sfd2_gconv_f32's [32 groups][9 taps][8 cin][8 cout]
std::vector<float> sf_pack_gconv_f32(const float* w)
{
    std::vector<float> p((size_t)32 * 9 * 8 * 8);
    for (int g = 0; g < 32; ++g)
        for (int t = 0; t < 9; ++t)
            for (int c = 0; c < 8; ++c)
                for (int j = 0; j < 8; ++j) p[(((size_t)g * 9 + t) * 8 + c) * 8 + j] = w[((size_t)(g * 8 + j) * 8 + c) * 9 + t];
    return p;
}

// OIHW [256][8][3][3] -> sfd2_gconv_h fragments [16 slices][5 k][hi / lo][64 lanes][8 halves = cin]: lane (m = output channel of the slice, g): tap 2 k + (g >> 1) of
// group g & 1 of the slice -- the weights of channel m if that is m's group, zero if it is the other one or the tap is the tenth
std::vector<float> sf_pack_gconv_h16(const float* w, float scale)
{
    return pack_lanes_h16(16 * 5, [&](int kb, int l, int cin) {
        const int sl = kb / 5, k = kb % 5, m = l & 15, g = l >> 4, t = 2 * k + (g >> 1);
        return (t < 9 && (m >> 3) == (g & 1)) ? w[((size_t)(sl * 16 + m) * 8 + cin) * 9 + t] * scale : 0.0f;
    });
}

struct Sfd2Net : kpb_net {
    Layer L[SF_LAYERS];             // conv1a (conv1a_rgb64) and the grouped layers of this file are mfma = false: their Layers carry the pointers only
    const uint4* gw[3] = {};        // split-f16: the grouped layers' fragments (sf_pack_gconv_h16), per ResBlock
    bool h16 = true;

    void gconv(int i, const float* in, float* out, int batch, int H, int W)
    {
        SfGcArgs a{in, out, L[i].w, gw[(i - SF_R0) / 3], L[i].b, L[i].unscale, H, W};
        const char* tag = L[i].prof.c_str();
        if (h16) KPB_LAUNCH(ctx, tag, sfd2_gconv_h, dim3(cdiv(W, GC_T), cdiv(H, GC_T), batch * 8), dim3(256), 0, ctx->stream, a);
        else KPB_LAUNCH(ctx, tag, sfd2_gconv_f32, dim3(cdiv(H * W, 256), 8, batch), dim3(256), 0, ctx->stream, a);
    }

    int forward(const float* img, int batch, int H, int W, float* score_out, float* desc_out) override
    {
        if ((H % 8) || (W % 8)) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: SFD2 needs H and W multiples of 8 (got %dx%d)", H, W);
        if (!desc_out) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: SFD2 writes its 128 x H/4 x W/4 descriptor map; desc_out_dev is required");
        if (H > 16384 || W > 16384 || batch > 8191) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: SFD2 image %dx%d x %d too large", H, W, batch);
        const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, Hc = H / 8, Wc = W / 8;
        const size_t P = (size_t)H * W, B = batch;
        float *x1a, *x1b, *x2a, *x2b, *q[4], *cpa0, *cpa3, *semi, *sta;
        if (int rc = kpb_carve(ctx, act, [&](Arena& a) {
                x1a = a.take(B * P * 64); x1b = a.take(B * (P / 4) * 64); x2a = a.take(B * (P / 4) * 128); x2b = a.take(B * (P / 16) * 128);
                for (float*& m : q) m = a.take(B * (P / 16) * 256);
                cpa0 = a.take(B * (P / 64) * 256); cpa3 = a.take(B * (P / 64) * 256); semi = a.take(B * (P / 64) * 65); sta = a.take(B * (P / 16) * 3);
            }))
            return rc;
        this->B = batch; this->H = H; this->W = W;
        hipStream_t st = ctx->stream;
        int rc;
        launch_conv1a_rgb64(ctx, L[SF_1A].prof.c_str(), img, x1a, L[SF_1A].w, L[SF_1A].b, batch, H, W);
        if ((rc = launch_mfma(ctx, L[SF_1B], x1a, x1b, batch, H, W))) return rc;
        if ((rc = launch_mfma(ctx, L[SF_2A], x1b, x2a, batch, H2, W2))) return rc;
        if ((rc = launch_mfma(ctx, L[SF_2B], x2a, x2b, batch, H2, W2))) return rc;
        if ((rc = launch_mfma(ctx, L[SF_3A], x2b, q[0], batch, H4, W4))) return rc;
        if ((rc = launch_mfma(ctx, L[SF_3B], q[0], q[1], batch, H4, W4))) return rc;
        float *x = q[1], *y = q[0];       // conv4: block k reads x and leaves its output in y
        for (int k = 0; k < 3; ++k) {
            const int i = SF_R0 + 3 * k;
            if ((rc = launch_mfma(ctx, L[i], x, q[2], batch, H4, W4))) return rc;
            gconv(i + 1, q[2], q[3], batch, H4, W4);
            if (k == 0 && ctx->sfd2_probe) {      // the test hook: the first grouped layer's output, half of its channels, instead of the descriptor map
                KPB_LAUNCH(ctx, "sfd2_probe", sfd2_take128, dim3((unsigned)((B * H4 * W4 * 32 + 255) / 256)), dim3(256), 0, st, q[3], desc_out, B * H4 * W4,
                           ctx->sfd2_probe == 2 ? 128 : 0);
                KPB_HIP(ctx, hipGetLastError());
                return KPB_OK;
            }
            if ((rc = launch_mfma(ctx, L[i + 2], q[3], y, batch, H4, W4, {.res = x}))) return rc;
            std::swap(x, y);
        }
        const float* out4 = x;          // = q[0]; q[1] .. q[3] are free again
        if ((rc = launch_mfma(ctx, L[SF_PA0], out4, cpa0, batch, H4, W4))) return rc;
        if ((rc = launch_mfma(ctx, L[SF_PA3], cpa0, cpa3, batch, Hc, Wc))) return rc;
        if ((rc = launch_mfma(ctx, L[SF_PB], cpa3, semi, batch, Hc, Wc))) return rc;
        if ((rc = launch_mfma(ctx, L[SF_STA], out4, sta, batch, H4, W4))) return rc;
        if ((rc = launch_mfma(ctx, L[SF_DA0], out4, q[2], batch, H4, W4))) return rc;
        if ((rc = launch_mfma(ctx, L[SF_DA3], q[2], q[3], batch, H4, W4))) return rc;
        if ((rc = launch_mfma(ctx, L[SF_DB], q[3], desc_out, batch, H4, W4))) return rc;
        launch_l2norm_nhwc(ctx, "sfd2_l2norm", desc_out, 128, B * H4 * W4, 1e-12f);       // F.normalize
        KPB_LAUNCH(ctx, "sfd2_score", sfd2_score, dim3(cdiv(Hc * Wc, 4 * SF_PXW), batch), dim3(256), 0, st, semi, sta, score_out, Hc, Wc);
        KPB_HIP(ctx, hipGetLastError());
        return KPB_OK;
    }
};

}  // namespace

int sfd2_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out)
{
    // folded tensor name, cin (per group for the grouped layers), cout, ks, stride, mfma, relu: conv1a and the grouped res*.c2 are kernels of this file; the third
    // layer of a ResBlock gets its ReLU behind the sum
    const Layer plan[] = {
        {"conv1a", 3, 64, 3, 1, false}, {"conv1b", 64, 64, 3, 2, true}, {"conv2a", 64, 128, 3, 1, true}, {"conv2b", 128, 128, 3, 2, true},
        {"conv3a", 128, 256, 3, 1, true}, {"conv3b", 256, 256, 3, 1, true},
        {"res0.c1", 256, 256, 1, 1, true}, {"res0.c2", 8, 256, 3, 1, false}, {"res0.c3", 256, 256, 1, 1, true},
        {"res1.c1", 256, 256, 1, 1, true}, {"res1.c2", 8, 256, 3, 1, false}, {"res1.c3", 256, 256, 1, 1, true},
        {"res2.c1", 256, 256, 1, 1, true}, {"res2.c2", 8, 256, 3, 1, false}, {"res2.c3", 256, 256, 1, 1, true},
        {"convPa0", 256, 256, 3, 2, true}, {"convPa3", 256, 256, 3, 1, true, false}, {"convPb", 256, 65, 1, 1, true, false},
        {"convDa0", 256, 256, 3, 1, true}, {"convDa3", 256, 256, 3, 1, true, false}, {"convDb", 256, 128, 1, 1, true, false},
        {"sta", 256, 3, 1, 1, true, false}};
    static_assert(sizeof(plan) / sizeof(plan[0]) == SF_LAYERS, "one plan entry per SF_* index");
    auto net = std::make_unique<Sfd2Net>();
    net->ctx = ctx; net->arch = KPB_ARCH_SFD2; net->dim = 128; net->desc_div = 4;
    net->h16 = conv_mfma_use_h16();
    WeightStage ws;
    const KpbwReader rd{bl, "kpb_net_create: SFD2 tensor %s missing or mis-shaped"};
    for (int i = 0; i < SF_LAYERS; ++i) {
        Layer& L = net->L[i] = plan[i];
        const float* w = rd.need(L.name + ".w", {(uint32_t)L.cout, (uint32_t)L.cin, (uint32_t)L.ks, (uint32_t)L.ks});
        const float* b = rd.need(L.name + ".b", {(uint32_t)L.cout});
        if (L.mfma || i == SF_1A) {     // (conv1a, mfma = false: [tap][c][64], as conv1a_rgb64 reads it)
            L.cc = L.stride == 2 ? 16 : 32;
            stage_layer(ws, L, "sfd2_", w, b);
            continue;
        }
        L.prof = "sfd2_" + L.name;      // the grouped 3 x 3 of a ResBlock
        if (net->h16) {
            const float sc = weight_scale_h(w, (size_t)L.cout * L.cin * 9);
            ws.put(sf_pack_gconv_h16(w, sc), &net->gw[(i - SF_R0) / 3]);
            L.unscale = 1.0f / sc;
        } else {
            ws.put(sf_pack_gconv_f32(w), &L.w);
        }
        ws.put_raw(b, 256, &L.b);
    }
    if (int rc = ws.upload(ctx, &net->wdev)) return rc;
    *out = net.release();
    return KPB_OK;
}
