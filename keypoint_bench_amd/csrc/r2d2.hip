// r2d2.hip -- N6 R2D2 (models/r2d2.py:101-141, Quad_L2Net_ConfCFS) on gfx950.  Nine convolutions at FULL resolution: the reference replaces every
// stride by a dilation (1, 1, 1, 2, 2, 4 for the 3 x 3 layers, 4, 8, 16 for the closing 2 x 2 ones), BatchNorm(affine = False) folded at pack time
// (weights.py fold_r2d2), then the confidence head on x^2 and the L2-normalised descriptor -- 483 168 MAC per pixel.
//   conv0          conv_rgb32 (conv_layer.h, shared with ALIKE-l): 3 -> 32 on the vector ALU from the planar image (0.2 % of the work)
//   conv1, conv2   conv_mfma_h, the forms SuperPoint uses
//   conv3 .. 5     conv_mfma_h with CmForm::dil = 2, 2, 4: the halo tile grows by (ks - 1) dil
//   conv6 .. 8     gemm_h<.., TAPK = 2>: four taps x 128 channels gathered at (+-d / 2, +-d / 2) -- no halo in LDS
//   r2d2_head      one pass over the 128-channel map: score and the normalised descriptor row
// KPB_FP32_MATRIX=1: conv1 .. 8 on conv_mfma (fp32 MFMA) with the same dilation field.
// matrix.mode = 1 in the blob (Quad_L2Net_ConfCFS(matrix="f16")): conv1 .. 8 in the single-f16 mode (Layer::h1, profile names r2d2_conv1_h1 ..): one MFMA a_hi b_hi
// per product -- TF32-class operands, what the reference's convolutions are on its own GPU.  conv0 and the head stay fp32.
#include "conv_layer.h"
#include "conv_mfma.h"      // relu

namespace {

// r2d2.py:136-141 on x = conv8's row of 128, IN PLACE on the descriptor map: reliability = softmax(clf(x^2))[1], repeatability = softplus(sal(x^2)) / (1 + softplus),
// score = their product, desc = x / max(||x||_2, 1e-12).  One wave per pixel, RHW pixels per wave with their loads in flight together; lane l holds channels
// 2 l and 2 l + 1, so a row is read and written as one 512-byte access.  The four sums are butterflies in a fixed order.  hw: [3][128] = clf row 0, clf row 1, sal; hb: [3].
__global__ __launch_bounds__(256) void r2d2_head(float* __restrict__ desc, float* __restrict__ score, const float* __restrict__ hw, const float* __restrict__ hb, size_t npix)
{
    constexpr int RHW = 4;
    const int lane = threadIdx.x & 63;
    const size_t pix0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RHW;
    if (pix0 >= npix) return;
    const float2 w0 = reinterpret_cast<const float2*>(hw)[lane], w1 = reinterpret_cast<const float2*>(hw + 128)[lane], ws = reinterpret_cast<const float2*>(hw + 256)[lane];
    const float b0 = hb[0], b1 = hb[1], bs = hb[2];
    float2 x[RHW];
#pragma unroll
    for (int i = 0; i < RHW; ++i) x[i] = reinterpret_cast<const float2*>(desc + min(pix0 + i, npix - 1) * 128)[lane];
#pragma unroll
    for (int i = 0; i < RHW; ++i) {
        const size_t pix = pix0 + i;
        const float q0 = x[i].x * x[i].x, q1 = x[i].y * x[i].y;
        const float ss = kpb_wave_sum(q0 + q1);
        const float u0 = kpb_wave_sum(fmaf(q0, w0.x, q1 * w0.y)) + b0;
        const float u1 = kpb_wave_sum(fmaf(q0, w1.x, q1 * w1.y)) + b1;
        const float us = kpb_wave_sum(fmaf(q0, ws.x, q1 * ws.y)) + bs;
        const float n = fmaxf(sqrtf(ss), 1e-12f);
        if (pix < npix) {
            reinterpret_cast<float2*>(desc + pix * 128)[lane] = make_float2(__fdiv_rn(x[i].x, n), __fdiv_rn(x[i].y, n));
            if (lane == 0) {
                const float m = fmaxf(u0, u1), e0 = expf(u0 - m), e1 = expf(u1 - m);
                const float rel = __fdiv_rn(e1, e0 + e1);
                const float sp = us > 20.0f ? us : log1pf(expf(us));      // torch's softplus (beta 1, threshold 20)
                score[pix] = __fdiv_rn(sp, 1.0f + sp) * rel;
            }
        }
    }
}

enum { R2_C0, R2_C1, R2_C2, R2_C3, R2_C4, R2_C5, R2_C6, R2_C7, R2_C8, R2_LAYERS };       // r2d2_create's plan order

struct R2d2Net : kpb_net {
    Layer L[R2_LAYERS];         // conv0 (mfma = false) is conv_rgb32: its Layer carries the pointers only
    const float* head_w = nullptr;
    const float* head_b = nullptr;
    int forward(const float* img, int batch, int H, int W, float* score_out, float* desc_out) override
    {
        if (!desc_out) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: R2D2 writes its 128 x H x W descriptor map; desc_out_dev is required");
        if (H > 32767 || W > 32767 || (size_t)H * W > ((size_t)1 << 30)) return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_forward: R2D2 image %dx%d too large", H, W);
        const size_t P = (size_t)H * W, B = batch;
        // every layer runs at full resolution: two ping-pong maps of the widest layer (128 channels: 157 MB per 480 x 640 image each) carry the narrower early
        // maps too; conv8 writes into the caller's descriptor map, which the head then normalises in place
        float* pp[2];
        if (int rc = kpb_carve(ctx, act, [&](Arena& a) { for (float*& q : pp) q = a.take(B * P * 128); })) return rc;
        this->B = batch; this->H = H; this->W = W;
        hipStream_t st = ctx->stream;
        launch_conv_rgb32(ctx, "r2d2_conv0", img, pp[0], L[R2_C0].w, L[R2_C0].b, batch, H, W);
        for (int i = R2_C1; i <= R2_C8; ++i)
            if (int rc = launch_mfma(ctx, L[i], pp[(i - 1) & 1], i == R2_C8 ? desc_out : pp[i & 1], batch, H, W)) return rc;
        KPB_LAUNCH(ctx, "r2d2_head", r2d2_head, dim3((unsigned)((B * P + 15) / 16)), dim3(256), 0, st, desc_out, score_out, head_w, head_b, B * P);
        KPB_HIP(ctx, hipGetLastError());
        return KPB_OK;
    }
};

}  // namespace

int r2d2_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out)
{
    // name, cin, cout, ks, stride, mfma, relu, pool_out, dil -- r2d2.py:105-117 with dilated = True: the strides of Quad_L2Net became the dilation of every layer behind them
    const Layer plan[] = {
        {"conv0", 3, 32, 3, 1, false}, {"conv1", 32, 32, 3, 1, true}, {"conv2", 32, 64, 3, 1, true}, {"conv3", 64, 64, 3, 1, true, true, false, 2},
        {"conv4", 64, 128, 3, 1, true, true, false, 2}, {"conv5", 128, 128, 3, 1, true, true, false, 4}, {"conv6", 128, 128, 2, 1, true, false, false, 4},
        {"conv7", 128, 128, 2, 1, true, false, false, 8}, {"conv8", 128, 128, 2, 1, true, false, false, 16}};
    static_assert(sizeof(plan) / sizeof(plan[0]) == R2_LAYERS, "one plan entry per R2_* index");
    auto net = std::make_unique<R2d2Net>();
    net->ctx = ctx; net->arch = KPB_ARCH_R2D2; net->dim = 128; net->desc_div = 1;
    WeightStage ws;
    const KpbwReader rd{bl, "kpb_net_create: R2D2 tensor %s missing or mis-shaped"};
    // the matrix mode travels in the blob (as harris.plan does): the optional tensor matrix.mode {1}; absent or 0 = split-f16, 1 = single f16 on conv1 .. conv8
    bool h1 = false;
    if (bl.t.count("matrix.mode")) {
        const float m = rd.need("matrix.mode", {1})[0];
        if (m != 0.0f && m != 1.0f) return kpb_fail(ctx, KPB_E_UNSUPPORTED, "kpb_net_create: R2D2 matrix.mode %g: 0 (split-f16) or 1 (single f16)", (double)m);
        if (m == 1.0f && !conv_mfma_use_h16())
            return kpb_fail(ctx, KPB_E_UNSUPPORTED, "kpb_net_create: R2D2 matrix.mode 1: the single-f16 mode needs the matrix-pipe build of the convolutions (KPB_FP32_MATRIX is set)");
        h1 = m == 1.0f;
    }
    for (int i = 0; i < R2_LAYERS; ++i) {
        Layer& L = net->L[i] = plan[i];
        L.h1 = h1 && L.mfma;
        const float* w = rd.need(L.name + ".w", {(uint32_t)L.cout, (uint32_t)L.cin, (uint32_t)L.ks, (uint32_t)L.ks});
        const float* b = rd.need(L.name + ".b", {(uint32_t)L.cout});
        // strict fp32: the 2 x 2, dilation-16 tile fits the LDS window in 16-channel slabs; the tap-gathered split-f16 product reads 32-channel slabs
        L.cc = (L.ks == 2 && !conv_mfma_use_h16()) ? 16 : 32;
        L.ntb = L.cout == 32 ? 1 : 2;       // conv1 owns one n-tile: the packs are n-tile-major, so its fragments sit where a two-tile pack had them and no second tile is fetched
        // (conv0, mfma = false: [tap][cin][32], as conv_rgb32 reads it.)  Profile names: the split net's layers are conv1 .. conv8 as they always were; the
        // single-f16 layers are r2d2_conv1_h1 .. r2d2_conv8_h1, so a report or a trace that holds both nets tells them apart
        stage_layer(ws, L, L.h1 ? "r2d2_" : "", w, b);
    }
    const float* cw = rd.need("clf.w", {2, 128});
    const float* cb = rd.need("clf.b", {2});
    const float* sw = rd.need("sal.w", {1, 128});
    const float* sb = rd.need("sal.b", {1});
    std::vector<float> hw(cw, cw + 256), hb = {cb[0], cb[1], sb[0]};
    hw.insert(hw.end(), sw, sw + 128);
    ws.put(hw, &net->head_w);
    ws.put(hb, &net->head_b);
    if (int rc = ws.upload(ctx, &net->wdev)) return rc;
    *out = net.release();
    return KPB_OK;
}
