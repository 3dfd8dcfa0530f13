// alike_l.hip -- N1 at the reference's DEFAULT plan: ALNet(param = None) = c1..c4 = 32, 64, 128, 128, dim = 128 (models/ALike.py:87-92, upstream's ALIKE-l) on gfx950.
// alike.hip's kernels are specialised to ALIKE-t's 8 / 16 / 32 / 64 channels and stay that way; every channel count here is a multiple of 32, so the trunk is a plan
// on conv_layer.h's Layer / stage_layer / launch_mfma and only the head is this file's own.  What the reference computes (ALike.py:136-164):
//  1. block1: conv 3 -> 32 and conv 32 -> 32, both 3 x 3 + eval-mode BatchNorm (folded at pack time, weights.py fold_alike) + ReLU: x1 at full resolution.
//  2. blocks 2 .. 4 behind max-pools of 2, 4 and 4: relu(conv2(relu(conv1(x))) + downsample(x)), conv1 / conv2 3 x 3 with folded BatchNorm, downsample 1 x 1 with
//     bias: x2 (64 channels, H / 2), x3 (128, H / 8), x4 (128, H / 32).
//  3. a_i = relu(conv_i(x_i)), 1 x 1 without bias, 32 channels each; a2, a3, a4 upsampled x 2, x 8, x 32 bilinearly with align_corners = True
//     (source coordinate = destination x (in - 1) / (out - 1)); the four concatenated: 128 features per pixel.
//  4. convhead2, 1 x 1 without bias, 128 -> 129: rows 0 .. 127 are the descriptor map (NOT normalised), row 128 through a sigmoid is the score.
// Kernels:
//   conv_rgb32         (conv_layer.h, shared with R2D2) block1.conv1 on the vector ALU from the planar image: one pixel x 8 output channels per thread
//   conv_mfma_h        every other 3 x 3 layer; KPB_FP32_MATRIX=1: conv_mfma
//   gemm_h             the 1 x 1 layers: downsample as <GE_RES_RELU> with conv2's output as the identity tile (addition commutes), agg2 .. agg4 plain
//   maxpool_nhwc       (conv_layer.h, shared with ALIKE-t) max_pool2d(x, K, K) of an NHWC map, K = 2 or 4
//   alike_l_head_h     the head, split-f16: a wave takes 32 pixels of a row -- builds their 128 features in registers (agg1 as fp32 fmaf chains, the three coarse maps
//                      gathered bilinearly), splits them at the scale of the tile's own largest magnitude, multiplies by convhead2's fragments (resident in LDS for the
//                      life of the workgroup) as v_mfma_f32_32x32x16_f16 triples and stores 512-byte descriptor rows; <false> is the keypoint-only form: the score
//                      tile alone, the same accumulation and therefore the same score bits, no descriptor store
//   alike_l_head_f32   the same head as plain fmaf chains (KPB_FP32_MATRIX=1)
//   alike_l_desc_at    descriptors at keypoints: the four integer taps of the 128 features blended, then one 128 x 128 mat-vec -- kpb_sample on the dense map up to
//                      re-association, because head and sampling are both linear
#include "conv_layer.h"
#include "conv_mfma.h"

#include <climits>

namespace {

constexpr int LQ = 32;          // channels of x1 and of every aggregated map (dim / 4)
constexpr int LDIM = 128;       // features per pixel = descriptor channels
constexpr int LWT = 132;        // floats of a row of the transposed head matrix [feature][output]: 128 descriptor rows + score row + pad (float4 aligned)

// ------------------------------------------------------------------------------------------------ the features of a pixel
// The four taps of nn.Upsample(scale_factor = H / Hs, 'bilinear', align_corners = True) for destination pixel (y, x): offsets in floats into one image's
// [Hs][Ws][32] map, and the weights of the lower / right taps.  A 1-pixel-high or -wide source is a constant: scale 0, both taps the same sample.
struct LTap { int o00, o01, o10, o11; float ly, lx; };
__device__ __forceinline__ LTap lh_taps(int y, int x, int H, int W, int Hs, int Ws)
{
    const float sy = kpb_ac_scale_gt1(Hs, H), sx = kpb_ac_scale_gt1(Ws, W);
    const kpb_lin ty = kpb_tap_ac(y, Hs, sy), tx = kpb_tap_ac(x, Ws, sx);
    // the first index stays clamped here, a guard that never acts (scale * o < n); the weights are those of the UNclamped index, the same wherever it does not act
    const int y0 = min(ty.i0, Hs - 1), x0 = min(tx.i0, Ws - 1);
    const int y1 = y0 + (y0 < Hs - 1 ? 1 : 0), x1 = x0 + (x0 < Ws - 1 ? 1 : 0);
    return LTap{(y0 * Ws + x0) * LQ, (y0 * Ws + x1) * LQ, (y1 * Ws + x0) * LQ, (y1 * Ws + x1) * LQ, ty.l, tx.l};
}
__device__ __forceinline__ float4 lh_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// channels c .. c + 3 of the upsampled map at the taps t
__device__ __forceinline__ float4 lh_mix4(const float* m, const LTap& t, int c)
{
    return kpb_mix4(lh_ld4(m + t.o00 + c), lh_ld4(m + t.o01 + c), lh_ld4(m + t.o10 + c), lh_ld4(m + t.o11 + c), t.ly, t.lx);
}
__device__ __forceinline__ float lh_mix1(const float* m, const LTap& t, int c) { return kpb_mix(m[t.o00 + c], m[t.o01 + c], m[t.o10 + c], m[t.o11 + c], t.ly, t.lx); }

struct LHeadArgs {
    const float *x1, *a2, *a3, *a4;     // [B][H][W][32], [B][H/2][W/2][32], [B][H/8][W/8][32], [B][H/32][W/32][32]
    const float* agg1;                  // conv1.weight transposed: [32 input channels][32 outputs]
    const uint4* wfr;                   // split-f16: convhead2 as fragments [8 k-steps][5 n-tiles][hi / lo][64 lanes] (lh_pack_head), scaled by 1 / inv_ws
    const float* whT;                   // fp32: convhead2 transposed, [128 features][LWT]
    float* score;                       // [B][H][W]
    float* desc;                        // [B][H][W][128]; null: the score only
    float inv_ws;
    int H, W, ntiles;                   // ntiles: 32-pixel row segments of the batch (split-f16) / 16-pixel ones (fp32)
};

// ------------------------------------------------------------------------------------------------ the head, split-f16
// Workgroup = 8 waves that walk the batch's 32-pixel row segments (W is a multiple of 32), a wave a segment; nothing is shared between the waves but the weights:
// one barrier, behind their load.  The MFMA is v_mfma_f32_32x32x16_f16 with A = the pixels (row = pixel p of the segment) and B = convhead2 (column = output
// channel), so a lane ends with ONE output channel of 16 pixels and a store instruction writes two 128-byte runs; the four n-tiles of a pixel follow each other:
// 512-byte rows from one wave.  Feature c = 16 s + 8 h + j is element j of lane half h in k-step s -- of the A operand, which lane (p, h) builds in registers, and
// of the B fragments (lh_pack_head).  K-steps 0, 1 = relu(agg1 x1), 2 .. 7 = a2, a3, a4 at the pixel (lh_mix4).
// The fifth n-tile carries the score row in ALL its 32 columns: every lane of a half then holds the logits of that half's 16 pixels, and lane (p, h = (p >> 2) & 1)
// picks pixel p's -- its register (p & 3) + 4 (p >> 3) -- so the score leaves as one 128-byte run without passing through LDS.
constexpr int LH_KS = 8, LH_NT = 5;
constexpr int LH_WFRAG = LH_KS * LH_NT * 2 * 64;                    // 16-byte slots of the fragments: 80 KB
constexpr size_t LH_LDS = (size_t)LH_WFRAG * 16 + 2 * 32 * 16 * 4;  // + agg1 as [lane half][input channel][16 outputs of that half]: 4 KB
template <bool DENSE>
__global__ __launch_bounds__(512) void alike_l_head_h(LHeadArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lh_lds[];
    uint4* wf = reinterpret_cast<uint4*>(lh_lds);
    float* aw = reinterpret_cast<float*>(lh_lds + (size_t)LH_WFRAG * 16);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, p = lane & 31, h = lane >> 5;
    for (int i = tid; i < LH_WFRAG; i += 512)
        if (DENSE || ((i >> 7) % LH_NT) == LH_NT - 1) wf[i] = a.wfr[i];
    for (int i = tid; i < 1024; i += 512) {       // output k of half hh: channel 8 hh + k (k-step 0) or 16 + 8 hh + k - 8 (k-step 1)
        const int hh = i >> 9, c = (i >> 4) & 31, k = i & 15;
        aw[i] = a.agg1[c * LQ + (k < 8 ? 8 * hh + k : 8 + 8 * hh + k)];
    }
    __syncthreads();
    const int tw = a.W >> 5;
    for (int t = blockIdx.x * 8 + wv; t < a.ntiles; t += gridDim.x * 8) {
        const int row = t / tw, x0 = (t - row * tw) << 5, b = row / a.H, y = row - b * a.H, x = x0 + p;
        int z = 0;                              // opaque zero: keeps the segment-invariant LDS reads inside the loop
        asm volatile("" : "+v"(z));             // (hoisted, they would pin the registers the features and accumulators need: alike.hip's head does the same)
        const float4* awh = reinterpret_cast<const float4*>(aw + h * 512) + z;
        const uint4* wfz = wf + z;
        float4 f[LH_KS][2];        // f[s][q]: features 16 s + 8 h + 4 q .. + 3
        {   // a1: sixteen fmaf chains over x1's channels in ascending order
            const float4* xr = reinterpret_cast<const float4*>(a.x1 + ((size_t)row * a.W + x) * LQ);
            float4 xv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) xv[q] = xr[q];
            float o[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) o[k] = 0.0f;
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                const float4 v4 = xv[c >> 2];
                const float xc = (c & 3) == 0 ? v4.x : (c & 3) == 1 ? v4.y : (c & 3) == 2 ? v4.z : v4.w;
#pragma unroll
                for (int k4 = 0; k4 < 4; ++k4) {
                    const float4 w4 = awh[c * 4 + k4];
                    o[4 * k4 + 0] = fmaf(xc, w4.x, o[4 * k4 + 0]); o[4 * k4 + 1] = fmaf(xc, w4.y, o[4 * k4 + 1]);
                    o[4 * k4 + 2] = fmaf(xc, w4.z, o[4 * k4 + 2]); o[4 * k4 + 3] = fmaf(xc, w4.w, o[4 * k4 + 3]);
                }
            }
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4)
                f[k4 >> 1][k4 & 1] = make_float4(relu(o[4 * k4]), relu(o[4 * k4 + 1]), relu(o[4 * k4 + 2]), relu(o[4 * k4 + 3]));
        }
        // the phases stay apart (here and below): scheduled into each other, the loads of a later phase are issued under the earlier one and their registers spill
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 1; g < 4; ++g) {
            const int sh = g == 1 ? 2 : (g == 2 ? 8 : 32), Hs = a.H / sh, Ws = a.W / sh;
            const float* m = (g == 1 ? a.a2 : (g == 2 ? a.a3 : a.a4)) + (size_t)b * Hs * Ws * LQ;
            const LTap tp = lh_taps(y, x, a.H, a.W, Hs, Ws);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int q = 0; q < 2; ++q) f[2 * g + ks][q] = lh_mix4(m, tp, 16 * ks + 8 * h + 4 * q);
            __builtin_amdgcn_sched_barrier(0);      // one map's sixteen loads in flight, not all three maps'
        }
        float am = 0.0f;
#pragma unroll
        for (int s = 0; s < LH_KS; ++s) am = cm_amax4(cm_amax4(am, f[s][0]), f[s][1]);
        const int e = cm_exp_of(cm_wave_max(am));       // the segment's own largest magnitude: the same bits alone or in a batch
        const float sc = cm_scale_of(e), un = a.inv_ws * cm_unscale_of(e);
        cm_h8 Ah[LH_KS], Al[LH_KS];
#pragma unroll
        for (int s = 0; s < LH_KS; ++s) {
            uint2 h0, l0, h1, l1;
            cm_split4(make_float4(f[s][0].x * sc, f[s][0].y * sc, f[s][0].z * sc, f[s][0].w * sc), h0, l0);
            cm_split4(make_float4(f[s][1].x * sc, f[s][1].y * sc, f[s][1].z * sc, f[s][1].w * sc), h1, l1);
            Ah[s] = __builtin_bit_cast(cm_h8, make_uint4(h0.x, h0.y, h1.x, h1.y));
            Al[s] = __builtin_bit_cast(cm_h8, make_uint4(l0.x, l0.y, l1.x, l1.y));
            __builtin_amdgcn_sched_barrier(0);      // a k-step's split at a time: its products, halves and residuals are transient
        }
        constexpr int N0 = DENSE ? 0 : LH_NT - 1;
        f32x16 acc[LH_NT - N0];
#pragma unroll
        for (int n = 0; n < LH_NT - N0; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[n][r] = 0.0f;
#pragma unroll
        for (int s = 0; s < LH_KS; ++s) {
#pragma unroll
            for (int n = N0; n < LH_NT; ++n) {
                const cm_h8 Bh = __builtin_bit_cast(cm_h8, wfz[((s * LH_NT + n) * 2 + 0) * 64 + lane]);
                const cm_h8 Bl = __builtin_bit_cast(cm_h8, wfz[((s * LH_NT + n) * 2 + 1) * 64 + lane]);
                acc[n - N0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al[s], Bh, acc[n - N0], 0, 0, 0);      // small terms first
                acc[n - N0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[s], Bl, acc[n - N0], 0, 0, 0);
                acc[n - N0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[s], Bh, acc[n - N0], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);      // one n-tile's fragments at a time
            }
        }
        const size_t pix0 = (size_t)row * a.W + x0;
        if constexpr (DENSE) {
            float* d = a.desc + pix0 * LDIM + p;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int pr = (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
                for (int n = 0; n < 4; ++n) d[(size_t)pr * LDIM + 32 * n] = acc[n][r] * un;
            }
        }
        if (((p >> 2) & 1) == h) {
            const int rs = (p & 3) + 4 * (p >> 3);
            float v = acc[LH_NT - 1 - N0][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) v = rs == r ? acc[LH_NT - 1 - N0][r] : v;
            a.score[pix0 + (p + z)] = __fdiv_rn(1.0f, 1.0f + expf(-(v * un)));       // torch.sigmoid (ALike.py:162)
        }
    }
}

// ------------------------------------------------------------------------------------------------ the head, strict fp32
// Workgroup = 16 pixels of a row.  Thread (pixel t >> 4, chunk t & 15) leaves features 8 (t & 15) .. + 7 of its pixel in LDS; then thread o < 129 runs output row o
// of all 16 pixels, a fmaf chain over the features in ascending order, reading its column of the transposed matrix once.  DENSE = false: thread 128 alone.
template <bool DENSE>
__global__ __launch_bounds__(256) void alike_l_head_f32(LHeadArgs a)
{
    __shared__ __attribute__((aligned(16))) float F[16][LDIM];
    const int tid = threadIdx.x, tw = a.W >> 4, t = blockIdx.x;
    const int row = t / tw, x0 = (t - row * tw) << 4, b = row / a.H, y = row - b * a.H;
    {
        const int pp = tid >> 4, k = tid & 15, g = k >> 2, cc = 8 * (k & 3), x = x0 + pp;
        float4 v0, v1;
        if (g == 0) {
            const float* xr = a.x1 + ((size_t)row * a.W + x) * LQ;
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = 0.0f;
#pragma unroll 4
            for (int c = 0; c < 32; ++c) {
                const float xc = xr[c];
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = fmaf(xc, a.agg1[c * LQ + cc + j], o[j]);
            }
            v0 = make_float4(relu(o[0]), relu(o[1]), relu(o[2]), relu(o[3]));
            v1 = make_float4(relu(o[4]), relu(o[5]), relu(o[6]), relu(o[7]));
        } else {
            const int sh = g == 1 ? 2 : (g == 2 ? 8 : 32), Hs = a.H / sh, Ws = a.W / sh;
            const float* m = (g == 1 ? a.a2 : (g == 2 ? a.a3 : a.a4)) + (size_t)b * Hs * Ws * LQ;
            const LTap tp = lh_taps(y, x, a.H, a.W, Hs, Ws);
            v0 = lh_mix4(m, tp, cc);
            v1 = lh_mix4(m, tp, cc + 4);
        }
        *reinterpret_cast<float4*>(&F[pp][8 * k]) = v0;
        *reinterpret_cast<float4*>(&F[pp][8 * k + 4]) = v1;
    }
    __syncthreads();
    if (DENSE ? tid > LDIM : tid != LDIM) return;
    float acc[16];
#pragma unroll
    for (int px = 0; px < 16; ++px) acc[px] = 0.0f;
#pragma unroll 4
    for (int c = 0; c < LDIM; ++c) {
        const float w = a.whT[c * LWT + tid];
#pragma unroll
        for (int px = 0; px < 16; ++px) acc[px] = fmaf(F[px][c], w, acc[px]);
    }
    const size_t pix0 = (size_t)row * a.W + x0;
    if (tid < LDIM) {
#pragma unroll
        for (int px = 0; px < 16; ++px) a.desc[(pix0 + px) * LDIM + tid] = acc[px];
    } else {
#pragma unroll
        for (int px = 0; px < 16; ++px) a.score[pix0 + px] = __fdiv_rn(1.0f, 1.0f + expf(-acc[px]));
    }
}

// ------------------------------------------------------------------------------------------------ desc_at
struct LDescAtArgs {
    LHeadArgs h;
    const float* pts; const int* n; float* out;
    int pts_cols, max_n;
    int kpw;                // keypoints a wave takes in turn, a multiple of LDA_K
};

// A wave takes LDA_K keypoints at a time: lane l evaluates features l (a1 | a2) and 64 + l (a3 | a4) of each -- at the four integer taps of the keypoint, a1 AFTER its
// ReLU, the coarse maps through their own interpolation -- blends them with grid_sample's weights (align_corners = True, zero padding) and leaves them in LDS; then
// the lane runs output rows l and 64 + l of the LDA_K keypoints together, fmaf chains over the features in ascending order, each weight read once for the LDA_K.
constexpr int LDA_K = 4;
__global__ __launch_bounds__(256) void alike_l_desc_at(LDescAtArgs a)
{
    __shared__ __attribute__((aligned(16))) float fs[4][LDA_K][LDIM];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = a.n ? min(a.n[b], a.max_n) : a.max_n;
    const int i0 = (blockIdx.x * 4 + wv) * a.kpw;
    const int H = a.h.H, W = a.h.W, j = lane & 31, gh = lane >> 5;
    for (int kk = 0; kk < a.kpw; kk += LDA_K) {
        if (i0 + kk >= n) break;                                // wave-uniform
        __builtin_amdgcn_wave_barrier();                        // the previous group's reads of fs are done (a wave's LDS operations execute in order)
#pragma unroll 1
        for (int k = 0; k < LDA_K; ++k) {
            const int i = i0 + kk + k;
            float v0 = 0.0f, v1 = 0.0f;
            if (i < n) {
                const float* pt = a.pts + ((size_t)b * a.max_n + i) * a.pts_cols;
                const kpb_grid gt = kpb_grid_taps((pt[0] - 0.5f) * 2.0f, (pt[1] - 0.5f) * 2.0f, W, H);   // matcher.py:221-222
                const float* cw = gt.w;         // blended below as one fused chain per feature, not kpb_grid_blend: the head that follows re-associates anyway
                const int x0 = (int)gt.x0, y0 = (int)gt.y0;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
                    if (tx < 0 || tx >= W || ty < 0 || ty >= H) continue;   // grid_sample zero padding
                    float u0, u1;
                    if (gh == 0) {
                        const float* px = a.h.x1 + (((size_t)b * H + ty) * W + tx) * LQ;
                        u0 = 0.0f;
#pragma unroll 8
                        for (int c = 0; c < 32; ++c) u0 = fmaf(px[c], a.h.agg1[c * LQ + j], u0);
                        u0 = relu(u0);
                        const int Hs = H / 8, Ws = W / 8;
                        u1 = lh_mix1(a.h.a3 + (size_t)b * Hs * Ws * LQ, lh_taps(ty, tx, H, W, Hs, Ws), j);
                    } else {
                        const int Hs = H / 2, Ws = W / 2, Hq = H / 32, Wq = W / 32;
                        u0 = lh_mix1(a.h.a2 + (size_t)b * Hs * Ws * LQ, lh_taps(ty, tx, H, W, Hs, Ws), j);
                        u1 = lh_mix1(a.h.a4 + (size_t)b * Hq * Wq * LQ, lh_taps(ty, tx, H, W, Hq, Wq), j);
                    }
                    v0 = fmaf(cw[t], u0, v0);
                    v1 = fmaf(cw[t], u1, v1);
                }
            }
            fs[wv][k][lane] = v0;
            fs[wv][k][64 + lane] = v1;
        }
        __builtin_amdgcn_wave_barrier();
        float acc[LDA_K][2];
#pragma unroll
        for (int k = 0; k < LDA_K; ++k) acc[k][0] = acc[k][1] = 0.0f;
#pragma unroll 4
        for (int c = 0; c < LDIM; ++c) {
            const float w0 = a.h.whT[c * LWT + lane], w1 = a.h.whT[c * LWT + 64 + lane];
#pragma unroll
            for (int k = 0; k < LDA_K; ++k) {
                const float fv = fs[wv][k][c];
                acc[k][0] = fmaf(fv, w0, acc[k][0]);
                acc[k][1] = fmaf(fv, w1, acc[k][1]);
            }
        }
#pragma unroll
        for (int k = 0; k < LDA_K; ++k) {
            const int i = i0 + kk + k;
            if (i >= n) break;                                  // wave-uniform: rows at or past n[b] are not written
            float* o = a.out + ((size_t)b * a.max_n + i) * LDIM;
            o[lane] = acc[k][0];
            o[64 + lane] = acc[k][1];
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
enum { AL_B1C1, AL_B1C2, AL_B2C1, AL_B2C2, AL_B2DS, AL_B3C1, AL_B3C2, AL_B3DS, AL_B4C1, AL_B4C2, AL_B4DS, AL_AGG2, AL_AGG3, AL_AGG4, AL_LAYERS };     // alike_l_create's plan order

// convhead2 [129][128] -> alike_l_head_h's B fragments [8 k-steps][5 n-tiles][hi / lo][64 lanes][8 halves]: lane (p, h) of k-step s holds features 16 s + 8 h + j
// of output channel 32 n + p; in the fifth tile EVERY column is the score row
std::vector<float> lh_pack_head(const float* hw, float scale)
{
    return pack_lanes_h16(LH_KS * LH_NT, [&](int kb, int l, int j) {
        const int s = kb / LH_NT, n = kb % LH_NT, p = l & 31, h = l >> 5;
        return hw[(size_t)(n < 4 ? 32 * n + p : LDIM) * LDIM + 16 * s + 8 * h + j] * scale;
    });
}

struct AlikeLNet : kpb_net {
    Layer L[AL_LAYERS];         // block1.conv1 (mfma = false) is conv_rgb32: its Layer carries the pointers only
    const float* agg1 = nullptr;
    const uint4* wfr = nullptr;
    const float* whT = nullptr;
    float inv_ws = 1.0f;
    bool h16 = true;
    const float *x1 = nullptr, *a2 = nullptr, *a3 = nullptr, *a4 = nullptr;       // of the last forward: what desc_at samples

    // relu(conv2(relu(conv1(x))) + downsample(x)) (ALike.py:65-81): the 1 x 1 layer joins conv2's output as its identity tile
    int res_block(int i, const float* x, float* t, float* u, float* out, int batch, int H, int W)
    {
        if (int rc = launch_mfma(ctx, L[i], x, t, batch, H, W)) return rc;
        if (int rc = launch_mfma(ctx, L[i + 1], t, u, batch, H, W)) return rc;
        return launch_mfma(ctx, L[i + 2], x, out, batch, H, W, {.res = u});
    }

    int forward(const float* img, int batch, int H, int W, float* score_out, float* desc_out) override
    {
        if ((H % 32) || (W % 32)) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: ALIKE needs H and W multiples of 32 (got %dx%d)", H, W);
        // 32-bit offsets into one image's maps (lh_taps: a2 is 8 P floats) and 32-bit segment counts
        if (H > 16384 || W > 16384 || batch > 8191 || (size_t)H * W > ((size_t)1 << 27) || (size_t)batch * H * W / 16 > (size_t)INT_MAX)
            return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: ALIKE image %dx%d x %d too large", H, W, batch);
        const int H2 = H / 2, W2 = W / 2, H8 = H / 8, W8 = W / 8, H32 = H / 32, W32 = W / 32;
        const size_t P = (size_t)H * W, B = batch;
        float *c0, *x1m, *p1, *t2, *u2, *x2, *p2, *t3, *u3, *x3, *p3, *t4, *u4, *x4, *a2m, *a3m, *a4m;
        if (int rc = kpb_carve(ctx, act, [&](Arena& a) {
                c0 = a.take(B * P * 32); x1m = a.take(B * P * 32); p1 = a.take(B * (P / 4) * 32);
                t2 = a.take(B * (P / 4) * 64); u2 = a.take(B * (P / 4) * 64); x2 = a.take(B * (P / 4) * 64); p2 = a.take(B * (P / 64) * 64);
                t3 = a.take(B * (P / 64) * 128); u3 = a.take(B * (P / 64) * 128); x3 = a.take(B * (P / 64) * 128); p3 = a.take(B * (P / 1024) * 128);
                t4 = a.take(B * (P / 1024) * 128); u4 = a.take(B * (P / 1024) * 128); x4 = a.take(B * (P / 1024) * 128);
                a2m = a.take(B * (P / 4) * LQ); a3m = a.take(B * (P / 64) * LQ); a4m = a.take(B * (P / 1024) * LQ);
            }))
            return rc;
        if (h16 && !(ctx->lds_attr_done & KPB_ATTR_ALIKE_L_HEAD)) {
            KPB_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(alike_l_head_h<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LH_LDS));
            KPB_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(alike_l_head_h<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LH_LDS));
            ctx->lds_attr_done |= KPB_ATTR_ALIKE_L_HEAD;
        }
        this->B = batch; this->H = H; this->W = W;
        x1 = x1m; a2 = a2m; a3 = a3m; a4 = a4m;
        hipStream_t st = ctx->stream;
        int rc;
        launch_conv_rgb32(ctx, L[AL_B1C1].prof.c_str(), img, c0, L[AL_B1C1].w, L[AL_B1C1].b, batch, H, W);
        if ((rc = launch_mfma(ctx, L[AL_B1C2], c0, x1m, batch, H, W))) return rc;
        launch_maxpool_nhwc(ctx, "alikel_pool_x1", 2, x1m, p1, batch, H2, W2, 32);
        if ((rc = res_block(AL_B2C1, p1, t2, u2, x2, batch, H2, W2))) return rc;
        launch_maxpool_nhwc(ctx, "alikel_pool_x2", 4, x2, p2, batch, H8, W8, 64);
        if ((rc = res_block(AL_B3C1, p2, t3, u3, x3, batch, H8, W8))) return rc;
        launch_maxpool_nhwc(ctx, "alikel_pool_x3", 4, x3, p3, batch, H32, W32, 128);
        if ((rc = res_block(AL_B4C1, p3, t4, u4, x4, batch, H32, W32))) return rc;
        if ((rc = launch_mfma(ctx, L[AL_AGG2], x2, a2m, batch, H2, W2))) return rc;
        if ((rc = launch_mfma(ctx, L[AL_AGG3], x3, a3m, batch, H8, W8))) return rc;
        if ((rc = launch_mfma(ctx, L[AL_AGG4], x4, a4m, batch, H32, W32))) return rc;
        LHeadArgs ha{x1m, a2m, a3m, a4m, agg1, wfr, whT, score_out, desc_out, inv_ws, H, W, 0};
        const char* tag = desc_out ? "alikel_head_dense" : "alikel_head_score";
        if (h16) {
            ha.ntiles = (int)(B * H * (W / 32));
            const dim3 grid(std::min(256, cdiv(ha.ntiles, 8)));       // one 8-wave workgroup per CU holds the fragments; each walks its share of the segments
            if (desc_out) KPB_LAUNCH(ctx, tag, alike_l_head_h<true>, grid, dim3(512), LH_LDS, st, ha);
            else KPB_LAUNCH(ctx, tag, alike_l_head_h<false>, grid, dim3(512), LH_LDS, st, ha);
        } else {
            ha.ntiles = (int)(B * H * (W / 16));
            if (desc_out) KPB_LAUNCH(ctx, tag, alike_l_head_f32<true>, dim3(ha.ntiles), dim3(256), 0, st, ha);
            else KPB_LAUNCH(ctx, tag, alike_l_head_f32<false>, dim3(ha.ntiles), dim3(256), 0, st, ha);
        }
        KPB_HIP(ctx, hipGetLastError());
        return KPB_OK;
    }

    int desc_at(const float* pts, int pts_cols, int max_n, const int32_t* n_dev, float* out) override
    {
        if (B == 0) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_desc_at: no forward has run");
        const int kpw = (long long)B * max_n >= 32768 ? 2 * LDA_K : LDA_K;
        LDescAtArgs a{LHeadArgs{x1, a2, a3, a4, agg1, wfr, whT, nullptr, nullptr, inv_ws, H, W, 0}, pts, n_dev, out, pts_cols, max_n, kpw};
        KPB_LAUNCH(ctx, "alikel_desc_at", alike_l_desc_at, dim3(cdiv(max_n, 4 * kpw), B), dim3(256), 0, ctx->stream, a);
        KPB_HIP(ctx, hipGetLastError());
        return KPB_OK;
    }
};

}  // namespace

int alike_l_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out)
{
    // folded tensor name, cin, cout, ks, stride, mfma, relu: block1.conv1 runs on the vector ALU (conv_rgb32); conv2 of a ResBlock gets its ReLU behind the sum, in the
    // downsample layer's epilogue; the aggregations carry no bias
    const Layer plan[] = {
        {"b1c1", 3, 32, 3, 1, false}, {"b1c2", 32, 32, 3, 1, true},
        {"b2c1", 32, 64, 3, 1, true}, {"b2c2", 64, 64, 3, 1, true, false}, {"b2ds", 32, 64, 1, 1, true},
        {"b3c1", 64, 128, 3, 1, true}, {"b3c2", 128, 128, 3, 1, true, false}, {"b3ds", 64, 128, 1, 1, true},
        {"b4c1", 128, 128, 3, 1, true}, {"b4c2", 128, 128, 3, 1, true, false}, {"b4ds", 128, 128, 1, 1, true},
        {"agg2", 64, LQ, 1, 1, true}, {"agg3", 128, LQ, 1, 1, true}, {"agg4", 128, LQ, 1, 1, true}};
    static_assert(sizeof(plan) / sizeof(plan[0]) == AL_LAYERS, "one plan entry per AL_* index");
    const KpbwReader rd{bl, "kpb_net_create: tensor %s missing or not ALIKE shaped (this build supports c1..c4 = 8,16,32,64, dim = 64 "
                            "and c1..c4 = 32,64,128,128, dim = 128)"};
    auto net = std::make_unique<AlikeLNet>();
    net->ctx = ctx; net->arch = KPB_ARCH_ALIKE; net->dim = LDIM; net->desc_div = 1;
    net->h16 = conv_mfma_use_h16();
    WeightStage ws;
    for (int i = 0; i < AL_LAYERS; ++i) {
        Layer& L = net->L[i] = plan[i];
        const uint32_t co = (uint32_t)L.cout, ci = (uint32_t)L.cin;
        const float* w = L.ks == 3 ? rd.need(L.name + ".w", {co, ci, 3, 3}) : rd.need(L.name + ".w", {co, ci});
        const float* b = i >= AL_AGG2 ? nullptr : rd.need(L.name + ".b", {co});
        L.ntb = (L.ks == 3 && L.cout == 32) ? 1 : 2;        // b1c2 owns one n-tile (r2d2.hip conv1); the 1 x 1 product always reads two (the second of agg2 .. 4 is padding)
        stage_layer(ws, L, "alikel_", w, b);        // (b1c1, mfma = false: [tap][cin][32], as conv_rgb32 reads it)
    }
    const float* a1w = rd.need("agg1.w", {(uint32_t)LQ, (uint32_t)LQ});
    const float* hw = rd.need("head.w", {(uint32_t)LDIM + 1, (uint32_t)LDIM});
    {
        std::vector<float> t((size_t)LQ * LQ), wt((size_t)LDIM * LWT, 0.0f);
        for (int o = 0; o < LQ; ++o)
            for (int c = 0; c < LQ; ++c) t[c * LQ + o] = a1w[o * LQ + c];
        ws.put(t, &net->agg1);
        for (int o = 0; o <= LDIM; ++o)
            for (int c = 0; c < LDIM; ++c) wt[(size_t)c * LWT + o] = hw[(size_t)o * LDIM + c];
        ws.put(wt, &net->whT);
        const float sh = weight_scale_h(hw, (size_t)(LDIM + 1) * LDIM);
        ws.put(lh_pack_head(hw, sh), &net->wfr);
        net->inv_ws = 1.0f / sh;
    }
    if (int rc = ws.upload(ctx, &net->wdev)) return rc;
    *out = net.release();
    return KPB_OK;
}
