// d2net.hip -- N12 D2-Net (models/D2_Net.py:10-105) on gfx950.  What the reference computes:
//  1. trunk: torchvision's vgg16().features[:22] -- conv1_1 3 -> 64, conv1_2 64 -> 64, pool, conv2_1 64 -> 128, conv2_2 128 -> 128, pool, conv3_1 128 -> 256,
//     conv3_2, conv3_3 256 -> 256, pool, conv4_1 256 -> 512, conv4_2, conv4_3 512 -> 512: all 3 x 3, padding 1, bias, no BatchNorm, a ReLU behind every layer but
//     conv4_3, the pools MaxPool2d(2, 2).  feat = the conv4_3 map, 512 x h x w with h = H / 8, w = W / 8.
//  2. soft detection (:57-81): x = relu(feat); m = the image's maximum of x; e = exp(x / m); S = 9 avg_pool3x3(e padded with ONES); local = e / S;
//     dw = the pixel's maximum of x over the 512 channels; s = max_c(local_c (x_c / dw)); score = s / (the image's sum of s).
//     A pixel whose channels are all <= 0 gives 0 / 0 there and, through the sum, NaN everywhere: the divisions are written plainly and do what IEEE does.
//  3. score map = F.interpolate(score, (H, W), 'bilinear', align_corners = True): source coordinate d (h - 1) / (H - 1), scale 0 when h == 1.
//  4. descriptors = F.normalize(feat, dim = 1, eps 1e-12) of the PRE-ReLU map: 512 channels at 1/8 resolution (desc_div 8), stored channels-last.
//     H and W must be multiples of 8 (the reference floor-pools other shapes; not built).
// Kernels:
//   conv1a_rgb64       (conv_layer.h, shared with SFD2) conv1_1 on the vector ALU from the planar image
//   conv_mfma_h        the nine other layers as split-f16 triples (SuperPoint's 16-row form; its pool_out form for conv1_2 / conv2_2 / conv3_3; conv4_3 with
//                      ConvM::relu = 0); KPB_FP32_MATRIX=1: conv_mfma.  conv4_3 writes the caller's descriptor buffer: the head reads the map there before
//                      l2norm_nhwc (convnet.hip) normalises it in place, so no second 512-channel map exists.
//   d2_max             one wave per pixel: dw into a [B][h][w] map, and the image's maximum by one atomic max per workgroup on the bit pattern (non-negative floats
//                      order as unsigned integers; a maximum does not depend on the order it is taken in)
//   d2_softdetect      16 x 16 pixels per workgroup, 16 channels at a time: the 18 x 18 positions' x and e = exp(x / m) go to LDS once (a position outside the map
//                      holds e = 1, the reference's padding), then a thread = a pixel forms the nine-tap sum, e / S x (x / dw) and its running maximum.  Neither
//                      the exp map nor the local map reaches HBM; s [B][h][w] does.
//   d2_sum             one workgroup per image: every thread adds its strided elements in index order, then a fixed tree -- the same bits every run, alone or
//                      in a batch; no float atomics
//   d2_upsample        one thread per output pixel: the four taps each divided by the image's sum (a true division), mixed as torch mixes them
#include "conv_layer.h"
#include "conv_mfma.h"

namespace {

// ------------------------------------------------------------------------------------------------ head
constexpr int D2_C = 512;

// dw[pixel] = max_c relu(feat[pixel][c]); umax[b] = the largest dw of image b as float bits (zeroed before the launch).  A wave takes D2_PXW pixels at a time,
// two float4 per lane and pixel, all loads in flight before the first reduction, D2_MAXIT times; a workgroup folds its four waves in LDS and sends ONE atomic
// (one per wave of four pixels was 38 400 atomics on 32 addresses per 32 images of 480 x 640, and the kernel waited for them: 0.36 ms against 0.05 ms of traffic).
constexpr int D2_PXW = 4, D2_MAXIT = 4, D2_MAXPIX = 4 * D2_PXW * D2_MAXIT;      // pixels per workgroup
__global__ __launch_bounds__(256) void d2_max(const float* __restrict__ feat /*[B][npix][512]*/, float* __restrict__ dw /*[B][npix]*/, unsigned* __restrict__ umax, int npix)
{
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.y;
    float wm = 0.0f;
#pragma unroll 1
    for (int it = 0; it < D2_MAXIT; ++it) {
        const int pix0 = blockIdx.x * D2_MAXPIX + (it * 4 + wv) * D2_PXW;
        if (pix0 >= npix) break;            // wave-uniform
        float4 v[D2_PXW][2];
#pragma unroll
        for (int i = 0; i < D2_PXW; ++i) {
            const float4* p = reinterpret_cast<const float4*>(feat + ((size_t)b * npix + min(pix0 + i, npix - 1)) * D2_C);
            v[i][0] = p[lane]; v[i][1] = p[64 + lane];
        }
#pragma unroll
        for (int i = 0; i < D2_PXW; ++i) {
            float m = fmaxf(fmaxf(fmaxf(v[i][0].x, v[i][0].y), fmaxf(v[i][0].z, v[i][0].w)), fmaxf(fmaxf(v[i][1].x, v[i][1].y), fmaxf(v[i][1].z, v[i][1].w)));
            m = kpb_wave_fmax(relu(m));
            if (pix0 + i < npix) {
                if (lane == 0) dw[(size_t)b * npix + pix0 + i] = m;
                wm = fmaxf(wm, m);
            }
        }
    }
    if (lane == 0) part[wv] = wm;
    __syncthreads();
    if (threadIdx.x == 0)       // >= +0: the bit patterns order as the floats do
        atomicMax(umax + b, __float_as_uint(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]))));
}

// s[pixel] = max_c (e_c / S_c) (x_c / dw) with e = exp(x / m), S = 9 ((sum of the 3 x 3 window of e, outside the map 1) / 9) -- avg_pool2d's sum in (ky, kx)
// order, its division, the reference's 9 x.
constexpr int D2_T = 16, D2_I = D2_T + 2, D2_NPOS = D2_I * D2_I, D2_CC = 16, D2_PITCH = D2_CC + 4;       // pitch 20 floats: the 16 lanes of a ds_read_b128 group
                                                                                                           // (consecutive pixels of a row) hit 16 distinct slots
__global__ __launch_bounds__(256) void d2_softdetect(const float* __restrict__ feat /*[B][h][w][512]*/, const float* __restrict__ dw, const unsigned* __restrict__ umax,
                                                     float* __restrict__ s /*[B][h][w]*/, int h, int w)
{
    constexpr int NLD = D2_NPOS * (D2_CC / 4), PER = (NLD + 255) / 256;
    __shared__ __attribute__((aligned(16))) float se[D2_NPOS * D2_PITCH];       // e of the 18 x 18 positions, 16 channels
    __shared__ __attribute__((aligned(16))) float sx[D2_NPOS * D2_PITCH];       // x = relu(feat) of the same
    const int tid = threadIdx.x, b = blockIdx.z, ty0 = blockIdx.y * D2_T, tx0 = blockIdx.x * D2_T;
    const int ly = tid >> 4, lx = tid & 15, gy = ty0 + ly, gx = tx0 + lx;
    const bool live = gy < h && gx < w;
    const float* in = feat + (size_t)b * h * w * D2_C;
    const float m = __uint_as_float(umax[b]);
    const float dwp = live ? dw[((size_t)b * h + gy) * w + gx] : 1.0f;
    float best = 0.0f;              // every candidate is >= 0 or NaN (the all-negative pixel's 0 / 0), and a NaN stays, as under torch.max
    for (int c0 = 0; c0 < D2_C; c0 += D2_CC) {
        float4 ld[PER];
        bool ok[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * 256, pos = min(i, NLD - 1) >> 2, q = i & 3, r = pos / D2_I, c = pos - r * D2_I;
            const int py = ty0 - 1 + r, px = tx0 - 1 + c;
            ok[k] = i < NLD && py >= 0 && py < h && px >= 0 && px < w;
            ld[k] = ok[k] ? *reinterpret_cast<const float4*>(in + ((size_t)py * w + px) * D2_C + c0 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();            // the previous chunk's taps are done with the tile
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * 256;
            if (i >= NLD) continue;
            const int at = (i >> 2) * D2_PITCH + 4 * (i & 3);
            const float4 x = make_float4(relu(ld[k].x), relu(ld[k].y), relu(ld[k].z), relu(ld[k].w));
            // a position outside the map is the reference's padding: e = 1 (not exp(0 / m), which is NaN when m is 0)
            const float4 e = ok[k] ? make_float4(expf(__fdiv_rn(x.x, m)), expf(__fdiv_rn(x.y, m)), expf(__fdiv_rn(x.z, m)), expf(__fdiv_rn(x.w, m))) : make_float4(1.f, 1.f, 1.f, 1.f);
            *reinterpret_cast<float4*>(se + at) = e;
            *reinterpret_cast<float4*>(sx + at) = x;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < D2_CC / 4; ++q) {
            float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float4 e = *reinterpret_cast<const float4*>(se + ((ly + t / 3) * D2_I + lx + t % 3) * D2_PITCH + 4 * q);
                sum.x += e.x; sum.y += e.y; sum.z += e.z; sum.w += e.w;
            }
            const int at = ((ly + 1) * D2_I + lx + 1) * D2_PITCH + 4 * q;
            const float4 e = *reinterpret_cast<const float4*>(se + at), x = *reinterpret_cast<const float4*>(sx + at);
            const float ev[4] = {e.x, e.y, e.z, e.w}, xv[4] = {x.x, x.y, x.z, x.w}, sv[4] = {sum.x, sum.y, sum.z, sum.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float S = 9.0f * __fdiv_rn(sv[j], 9.0f);
                const float v = __fdiv_rn(ev[j], S) * __fdiv_rn(xv[j], dwp);
                if (v > best || v != v) best = v;
            }
        }
    }
    if (live) s[((size_t)b * h + gy) * w + gx] = best;
}

// sum[b] = the sum of s over image b: thread t adds elements t, t + 256, ... in that order, the 64 lanes of a wave fold by a butterfly, wave 0 adds the four
// wave sums in wave order.  Nothing depends on the batch or on timing.
__global__ __launch_bounds__(256) void d2_sum(const float* __restrict__ s, float* __restrict__ sum, int npix)
{
    __shared__ float part[4];
    const float* p = s + (size_t)blockIdx.x * npix;
    float a = 0.0f;
    for (int i = threadIdx.x; i < npix; i += 256) a += p[i];
    a = kpb_wave_sum(a);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) sum[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// F.interpolate(s / sum, (H, W), 'bilinear', align_corners = True): source coordinate = d x (float)(h - 1) / (H - 1) (0 when H == 1), the second tap
// clamped at the edge, weights (1 - l, l), rows mixed after columns -- torch's own order.
__global__ __launch_bounds__(256) void d2_upsample(const float* __restrict__ s, const float* __restrict__ sum, float* __restrict__ out, int h, int w, int H, int W)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= W || y >= H) return;
    const kpb_lin ty = kpb_tap_ac(y, h, kpb_ac_scale(h, H)), tx = kpb_tap_ac(x, w, kpb_ac_scale(w, W));
    // the source can be one sample: index and weight stay clamped here.  Both are guards that never act (scale * o < n); the weight is that of the UNclamped index
    const int y0 = min(ty.i0, h - 1), x0 = min(tx.i0, w - 1), y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fminf(fmaxf(ty.l, 0.0f), 1.0f), lx = fminf(fmaxf(tx.l, 0.0f), 1.0f);
    const float* p = s + (size_t)b * h * w;
    const float t = sum[b];
    const float a = __fdiv_rn(p[(size_t)y0 * w + x0], t), c = __fdiv_rn(p[(size_t)y0 * w + x1], t);
    const float d = __fdiv_rn(p[(size_t)y1 * w + x0], t), e = __fdiv_rn(p[(size_t)y1 * w + x1], t);
    out[((size_t)b * H + y) * W + x] = kpb_mix(a, c, d, e, ly, lx);
}

// ------------------------------------------------------------------------------------------------ host
enum { D2_11, D2_12, D2_21, D2_22, D2_31, D2_32, D2_33, D2_41, D2_42, D2_43, D2_LAYERS };        // d2net_create's plan order

struct D2Net : kpb_net {
    Layer L[D2_LAYERS];         // conv1_1 is conv1a_rgb64: its Layer carries the pointers only

    int forward(const float* img, int batch, int H, int W, float* score_out, float* desc_out) override
    {
        if ((H % 8) || (W % 8) || H < 8 || W < 8) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: D2Net needs H and W multiples of 8 (got %dx%d)", H, W);
        if (!desc_out) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: D2Net writes its 512 x H/8 x W/8 descriptor map; desc_out_dev is required");
        if (H > 16384 || W > 16384 || batch > 8191) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: D2Net image %dx%d x %d too large", H, W, batch);
        const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, h = H / 8, w = W / 8;
        const size_t P = (size_t)H * W, B = batch;
        float *x11, *x12, *x21, *x22, *x31, *x32, *x33, *x41, *x42, *dw, *s, *sum;
        unsigned* umax;
        if (int rc = kpb_carve(ctx, act, [&](Arena& a) {
                x11 = a.take(B * P * 64); x12 = a.take(B * (P / 4) * 64); x21 = a.take(B * (P / 4) * 128); x22 = a.take(B * (P / 16) * 128);
                x31 = a.take(B * (P / 16) * 256); x32 = a.take(B * (P / 16) * 256); x33 = a.take(B * (P / 64) * 256);
                x41 = a.take(B * (P / 64) * 512); x42 = a.take(B * (P / 64) * 512);
                dw = a.take(B * (P / 64)); s = a.take(B * (P / 64)); sum = a.take(B); umax = a.take<unsigned>(B);
            }))
            return rc;
        this->B = batch; this->H = H; this->W = W;
        hipStream_t st = ctx->stream;
        int rc;
        launch_conv1a_rgb64(ctx, L[D2_11].prof.c_str(), img, x11, L[D2_11].w, L[D2_11].b, batch, H, W);
        if ((rc = launch_mfma(ctx, L[D2_12], x11, x12, batch, H, W))) return rc;
        if ((rc = launch_mfma(ctx, L[D2_21], x12, x21, batch, H2, W2))) return rc;
        if ((rc = launch_mfma(ctx, L[D2_22], x21, x22, batch, H2, W2))) return rc;
        if ((rc = launch_mfma(ctx, L[D2_31], x22, x31, batch, H4, W4))) return rc;
        if ((rc = launch_mfma(ctx, L[D2_32], x31, x32, batch, H4, W4))) return rc;
        if ((rc = launch_mfma(ctx, L[D2_33], x32, x33, batch, H4, W4))) return rc;
        if ((rc = launch_mfma(ctx, L[D2_41], x33, x41, batch, h, w))) return rc;
        if ((rc = launch_mfma(ctx, L[D2_42], x41, x42, batch, h, w))) return rc;
        float* feat = desc_out;         // the pre-ReLU conv4_3 map: read by the head, then normalised in place
        if ((rc = launch_mfma(ctx, L[D2_43], x42, feat, batch, h, w))) return rc;
        KPB_HIP(ctx, hipMemsetAsync(umax, 0, B * sizeof(unsigned), st));
        KPB_LAUNCH(ctx, "d2_max", d2_max, dim3(cdiv(h * w, D2_MAXPIX), batch), dim3(256), 0, st, feat, dw, umax, h * w);
        KPB_LAUNCH(ctx, "d2_softdetect", d2_softdetect, dim3(cdiv(w, D2_T), cdiv(h, D2_T), batch), dim3(256), 0, st, feat, dw, umax, s, h, w);
        KPB_LAUNCH(ctx, "d2_sum", d2_sum, dim3(batch), dim3(256), 0, st, s, sum, h * w);
        KPB_LAUNCH(ctx, "d2_upsample", d2_upsample, dim3(cdiv(W, 64), cdiv(H, 4), batch), dim3(256), 0, st, s, sum, score_out, h, w, H, W);
        launch_l2norm_nhwc(ctx, "d2_l2norm", desc_out, D2_C, B * h * w, 1e-12f);       // F.normalize
        KPB_HIP(ctx, hipGetLastError());
        return KPB_OK;
    }
};

}  // namespace

int d2net_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out)
{
    // folded tensor name, cin, cout, ks, stride, mfma, relu, pool_out (the 2 x 2 max-pool behind conv1_2 / 2_2 / 3_3); all 3 x 3, padding 1, bias
    const Layer plan[] = {
        {"conv1_1", 3, 64, 3, 1, false}, {"conv1_2", 64, 64, 3, 1, true, true, true}, {"conv2_1", 64, 128, 3, 1, true}, {"conv2_2", 128, 128, 3, 1, true, true, true},
        {"conv3_1", 128, 256, 3, 1, true}, {"conv3_2", 256, 256, 3, 1, true}, {"conv3_3", 256, 256, 3, 1, true, true, true},
        {"conv4_1", 256, 512, 3, 1, true}, {"conv4_2", 512, 512, 3, 1, true}, {"conv4_3", 512, 512, 3, 1, true, false}};
    static_assert(sizeof(plan) / sizeof(plan[0]) == D2_LAYERS, "one plan entry per D2_* index");
    auto net = std::make_unique<D2Net>();
    net->ctx = ctx; net->arch = KPB_ARCH_D2NET; net->dim = D2_C; net->desc_div = 8;
    WeightStage ws;
    const KpbwReader rd{bl, "kpb_net_create: D2Net tensor %s missing or mis-shaped"};
    for (int i = 0; i < D2_LAYERS; ++i) {
        Layer& L = net->L[i] = plan[i];
        const float* w = rd.need(L.name + ".w", {(uint32_t)L.cout, (uint32_t)L.cin, 3u, 3u});
        const float* b = rd.need(L.name + ".b", {(uint32_t)L.cout});
        stage_layer(ws, L, "d2_", w, b);        // (conv1_1, mfma = false: [tap][c][64], as conv1a_rgb64 reads it)
    }
    if (int rc = ws.upload(ctx, &net->wdev)) return rc;
    *out = net.release();
    return KPB_OK;
}
