// conv_layer.hip -- stage_layer and launch_mfma (conv_layer.h): the one place where the generic forms of conv_mfma_h, conv_mfma and gemm_h that the six
// networks launch are instantiated.  A network that needs a new form adds it to the lists here.  Also the small kernels more than one network's unit
// launches, each defined here once: conv_rgb32, conv1a_rgb64, maxpool_nhwc.
#include "conv_layer.h"
#include "conv_mfma.h"

namespace {

// 3 -> 32 from the planar image + ReLU: one pixel x 8 output channels per thread, the 27 x 8 weights wave-uniform; reads [B][3][H][W], writes [B][H][W][32]
__global__ __launch_bounds__(256) void conv_rgb32(const float* __restrict__ img, float* __restrict__ out, const float* __restrict__ w /*[27][32]*/,
                                                  const float* __restrict__ bias, int H, int W)
{
    const int b = blockIdx.z, cg = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const int oy = pix / W, ox = pix - oy * W;
    const float* im = img + (size_t)b * 3 * H * W;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bias[cg * 8 + j];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int iy = oy + ky - 1, ix = ox + kx - 1;
            const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = in ? im[((size_t)c * H + iy) * W + ix] : 0.0f;
                const float* wt = w + ((ky * 3 + kx) * 3 + c) * 32 + cg * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = fmaf(v, wt[j], acc[j]);
            }
        }
    float4* o = reinterpret_cast<float4*>(out + ((size_t)b * H * W + pix) * 32 + cg * 8);
    o[0] = make_float4(relu(acc[0]), relu(acc[1]), relu(acc[2]), relu(acc[3]));
    o[1] = make_float4(relu(acc[4]), relu(acc[5]), relu(acc[6]), relu(acc[7]));
}

// 3 -> 64 from the planar image + ReLU (27 taps; conv1a_c64's column walk): 16 lanes share a pixel, each keeps the 27 taps of its 4 output channels in registers
// and walks down a column; a wave store is 4 whole 256-byte pixels.  Every output is bias, then the taps in (kx, channel) order of rows y - 1, y, y + 1
// interleaved, an fma each; a tap outside the image is zero.
__global__ __launch_bounds__(256) void conv1a_rgb64(const float* __restrict__ img, float* __restrict__ out, const float* __restrict__ w /*[3 ky][3 kx][3 c][64]*/,
                                                     const float* __restrict__ bias, int H, int W, int rows_per_block)
{
    const int b = blockIdx.z, lane16 = threadIdx.x & 15, c4 = lane16 * 4;
    const int x = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (x >= W) return;
    float wr[27][4], bv[4];
#pragma unroll
    for (int t = 0; t < 27; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) wr[t][j] = w[t * 64 + c4 + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = bias[c4 + j];
    const size_t P = (size_t)H * W;
    const float* im = img + (size_t)b * 3 * P;
    auto ld = [&](int yy, int k) {      // k = 3 kx + channel
        const int xx = x - 1 + k / 3;
        return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? im[(size_t)(k % 3) * P + (size_t)yy * W + xx] : 0.0f;
    };
    const int y0 = blockIdx.y * rows_per_block, y1 = min(y0 + rows_per_block, H);
    float r0[9], r1[9], r2[9], r3[9];       // the row below is requested one iteration before it is used
#pragma unroll
    for (int k = 0; k < 9; ++k) { r0[k] = ld(y0 - 1, k); r1[k] = ld(y0, k); r2[k] = ld(y0 + 1, k); }
    for (int y = y0; y < y1; ++y) {
#pragma unroll
        for (int k = 0; k < 9; ++k) r3[k] = ld(y + 2, k);
        float acc[4] = {bv[0], bv[1], bv[2], bv[3]};
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[j] = fmaf(r0[k], wr[k][j], acc[j]);
                acc[j] = fmaf(r1[k], wr[9 + k][j], acc[j]);
                acc[j] = fmaf(r2[k], wr[18 + k][j], acc[j]);
            }
        *reinterpret_cast<float4*>(out + (((size_t)b * H + y) * W + x) * 64 + c4) = make_float4(relu(acc[0]), relu(acc[1]), relu(acc[2]), relu(acc[3]));
#pragma unroll
        for (int k = 0; k < 9; ++k) { r0[k] = r1[k]; r1[k] = r2[k]; r2[k] = r3[k]; }
    }
}

// max_pool2d(x, K, K) of an NHWC map [B][K Ho][K Wo][C] (ALike.py:139, 141, 143): one thread per pooled pixel and channel quad.  ALIKE-t at batch size: block 4's
// conv1 reads the pooled x3 (19.7 MB per 512 images) instead of max-pooling x3 itself while it stages: sixteen loads per staged value, by four workgroups per tile
template <int K>
__global__ __launch_bounds__(256) void maxpool_nhwc(const float* __restrict__ in, float* __restrict__ out, int Ho, int Wo, int C)
{
    const int C4 = C / 4;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= (size_t)Ho * Wo * C4) return;
    const int c = (int)(i % C4) * 4;
    const size_t pix = i / C4;
    const int y = (int)(pix / Wo), x = (int)(pix - (size_t)y * Wo);
    const float* s = in + ((b * K * Ho + K * y) * (size_t)(K * Wo) + K * x) * C + c;
    float4 m = *reinterpret_cast<const float4*>(s);
#pragma unroll
    for (int py = 0; py < K; ++py)
#pragma unroll
        for (int px = 0; px < K; ++px) {
            if (py == 0 && px == 0) continue;
            const float4 v = *reinterpret_cast<const float4*>(s + ((size_t)py * K * Wo + px) * C);
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    *reinterpret_cast<float4*>(out + ((b * Ho + y) * (size_t)Wo + x) * C + c) = m;
}

// OIHW -> [tap][cin][COUT8]: conv_valu's weights (convnet.hip), and conv_rgb32's / conv1a_rgb64's with CIN = 3
std::vector<float> pack_valu(const float* w, int COUT, int CIN, int KS)
{
    const int T = KS * KS, C8 = ((COUT + 7) / 8) * 8;
    std::vector<float> out((size_t)T * CIN * C8, 0.0f);
    for (int o = 0; o < COUT; ++o)
        for (int c = 0; c < CIN; ++c)
            for (int t = 0; t < T; ++t) out[((size_t)t * CIN + c) * C8 + o] = w[((size_t)o * CIN + c) * T + t];
    return out;
}

}  // namespace

void launch_conv_rgb32(kpb_ctx* ctx, const char* tag, const float* img, float* out, const float* w, const float* bias, int batch, int H, int W)
{
    KPB_LAUNCH(ctx, tag, conv_rgb32, dim3((unsigned)(((size_t)H * W + 255) / 256), 4, batch), dim3(256), 0, ctx->stream, img, out, w, bias, H, W);
}

void launch_conv1a_rgb64(kpb_ctx* ctx, const char* tag, const float* img, float* out, const float* w, const float* bias, int batch, int H, int W)
{
    KPB_LAUNCH(ctx, tag, conv1a_rgb64, dim3(cdiv(W, 16), cdiv(H, 32), batch), dim3(256), 0, ctx->stream, img, out, w, bias, H, W, 32);
}

void launch_maxpool_nhwc(kpb_ctx* ctx, const char* tag, int K, const float* in, float* out, int batch, int Ho, int Wo, int C)
{
    const dim3 grid((unsigned)(((size_t)Ho * Wo * (C / 4) + 255) / 256), batch);
    if (K == 2) KPB_LAUNCH(ctx, tag, maxpool_nhwc<2>, grid, dim3(256), 0, ctx->stream, in, out, Ho, Wo, C);
    else KPB_LAUNCH(ctx, tag, maxpool_nhwc<4>, grid, dim3(256), 0, ctx->stream, in, out, Ho, Wo, C);
}

int launch_mfma(kpb_ctx* ctx, const Layer& L, const float* in, float* out, int B, int Hi, int Wi, const MfmaOpt& o)
{
    const int S = L.stride, CC = L.cc, HALO = (L.ks - 1) * L.dil, PAD = HALO / 2;       // CmForm::dil: the output keeps the input's extent at stride 1 for odd and even ks
    const char* name = L.prof.c_str();
    ConvM a{.in = in, .out = out, .wp = L.w, .bias = L.b, .xf = o.xf, .res = o.res,
            .Hi = Hi, .Wi = Wi, .H = (Hi + 2 * PAD - HALO - 1) / S + 1, .W = (Wi + 2 * PAD - HALO - 1) / S + 1, .CIN = L.cin, .COUT = L.cout, .NCH = L.cin / CC,
            .relu = o.res ? 0 : L.relu, .nblk = (L.cout + 32 * L.ntb - 1) / (32 * L.ntb), .istride = L.cin, .ostride = L.cout, .rstride = o.res ? L.cout : 0,
            .aux0 = reinterpret_cast<const float*>(o.unfold_mr), .unfold_w = o.unfold_w};
    if (o.unfold_w && !(conv_mfma_use_h16() && L.ks == 1 && S == 1 && CC == 32 && !L.pool_out && !o.xf && L.cin == 64))
        return kpb_fail(ctx, KPB_E_INVALID, "launch_mfma: the unfolded input exists for 64-channel 1x1 layers of the split-f16 form only");
    if (o.res && (L.ks != 1 || L.cout % 64)) return kpb_fail(ctx, KPB_E_INVALID, "SFD2 %s: the identity branch joins 1x1 layers of whole 64-channel tiles", L.name.c_str());
    if (o.last_only && L.ntb != 5) return kpb_fail(ctx, KPB_E_INVALID, "launch_mfma: %s has no channel beside its tiles to compute alone", L.name.c_str());
    const std::string last_name = L.prof + "_score";
    if (o.last_only) name = last_name.c_str();
    hipStream_t st = ctx->stream;
    const bool x = o.xf != nullptr;
    if (L.h1 && !conv_mfma_use_h16()) return kpb_fail(ctx, KPB_E_INVALID, "launch_mfma: %s: the single-f16 mode has no strict-fp32 form (KPB_FP32_MATRIX is set)", L.name.c_str());
    if (conv_mfma_use_h16()) {
        a.unscale = L.unscale;
        if (L.ks == 1 && S == 1 && CC == 32 && !L.pool_out && !x && !o.pre) {     // 1x1: gemm_h
            if (L.h1) return kpb_fail(ctx, KPB_E_INVALID, "launch_mfma: no single-f16 instance of the 1x1 product for %s", L.name.c_str());
            const dim3 grid(cdiv(a.H * a.W, 128), 1, B * a.nblk), block(256);
            if (o.l2_eps > 0.0f) {
                if (L.cout != 64 || L.ntb != 2) return kpb_fail(ctx, KPB_E_INVALID, "launch_mfma: the fused L2 norm needs a 64-channel layer");
                a.xb = o.l2_eps;
                KPB_LAUNCH(ctx, name, (gemm_h<2, 1, GE_L2NORM>), grid, block, 0, st, a);
            }
            else if (o.unfold_w) KPB_LAUNCH(ctx, name, (gemm_h<2, 1, GE_PLAIN, true>), grid, block, 0, st, a);
            else if (o.res) KPB_LAUNCH(ctx, name, (gemm_h<2, 1, GE_RES_RELU>), grid, block, 0, st, a);
            else KPB_LAUNCH(ctx, name, (gemm_h<2, 1>), grid, block, 0, st, a);
            return KPB_OK;
        }
        if (L.ks == 2) {        // tap-gathered product (R2D2's dilated 2 x 2 layers): K = 4 taps x cin, 128 pixels x 64 output channels per workgroup
            a.NCH = 4 * (L.cin / 32); a.tap_dil = L.dil;
            if (L.h1) KPB_LAUNCH(ctx, name, (gemm_h<2, 1, GE_PLAIN, false, 2, true>), dim3(cdiv(a.H * a.W, 128), 1, B * a.nblk), dim3(256), 0, st, a);
            else KPB_LAUNCH(ctx, name, (gemm_h<2, 1, GE_PLAIN, false, 2>), dim3(cdiv(a.H * a.W, 128), 1, B * a.nblk), dim3(256), 0, st, a);
            return KPB_OK;
        }
        // split-f16 form: stride-1 layers on 16-row workgroup tiles; with two n-tiles per workgroup the waves form 2 row groups x 2 n-tiles
        // (four M tiles and one n-tile per wave)
        CmForm f{.ks = L.ks, .s = S, .cc = CC, .pool_out = L.pool_out, .xf = x, .ntb = 1, .mt = 4, .wn = 2, .dil = L.dil, .h1 = L.h1};
        // one-tile layers (cout <= 32) are bound by per-workgroup latency: 8-row tiles (one M tile per wave, 28 KB of LDS, five
        // workgroups per CU) measured 8-16 % faster; layers with two output tiles lose the fragment reuse that way (+8 % time)
        if (L.ntb == 1) f.mt = f.wn = 1;
        if (S == 2) f.mt = 2;           // stride 2: 8-row tiles
        if (L.dil == 4) f.mt = 2;       // dilation 4: 8-row tiles -- the 24-pixel-wide tile would not fit 16 rows into the LDS window
        if (const PreSplit* pre = o.pre) {      // the input arrives already split (ConvM::pre_amax), generated while the tile is staged from the one-channel image the layer in front reads
            if (!pre->gen_w) return kpb_fail(ctx, KPB_E_INVALID, "conv_mfma_h: no generated-input instance for %s", L.name.c_str());
            a.pre_amax = pre->amax; a.pre_l1 = pre->l1; a.pre_bmax = pre->bmax; a.gen_w = pre->gen_w; a.gen_b = pre->gen_b; a.istride = 1;
            f.pre = f.gen = true;
        }
        if (const UpSrc* up = o.up) {       // [up(bottom) | horizontal] evaluated while staging (ConvM::up_src); `in` holds the channels behind the upsampled ones
            if (up->c % CC || up->c >= L.cin || (Hi % 2) || (Wi % 2)) return kpb_fail(ctx, KPB_E_INVALID, "launch_mfma: bad upsampled-input split for %s", L.name.c_str());
            a.up_src = up->src; a.up_c = up->c; a.istride = L.cin - up->c;
            f.up = true;
        }
        if (L.ntb == 5) {
            // 129 = 4 x 32 + 1 (DISK up_3): four MFMA tiles (two workgroups of two: 64 accumulator registers, three waves per SIMD)
            // and the score channel on the VALU of the first workgroup
            a.nblk = 2; a.xw = L.xw; a.xb = L.xb; a.xun = L.xun; a.xco = L.cout - 1;
            f.xc = true;
            if (o.last_only) {      // the same staging and the same VALU channel, no tiles: one workgroup per tile of the image, one float per pixel
                a.nblk = 1; a.ostride = 1; a.xco = 0;
                f.xo = true;
            }
        }
        return launch_conv_mfma_h<
            CmForm{.ks = 3, .s = 1, .cc = 32, .ntb = 1}, CmForm{.ks = 3, .s = 1, .cc = 32, .ntb = 1, .mt = 4, .wn = 2},
            CmForm{.ks = 3, .s = 1, .cc = 32, .pool_out = true, .ntb = 1, .mt = 4, .wn = 2}, CmForm{.ks = 3, .s = 1, .cc = 32, .pool_out = true, .ntb = 1, .mt = 4, .pre = true, .wn = 2, .gen = true},
            CmForm{.ks = 3, .s = 2, .cc = 16, .ntb = 1, .mt = 2, .wn = 2}, CmForm{.ks = 5, .s = 1, .cc = 16, .xf = true, .ntb = 1, .mt = 4, .wn = 2},
            CmForm{.ks = 5, .s = 1, .cc = 32, .xf = true, .ntb = 1, .mt = 4, .wn = 2}, CmForm{.ks = 5, .s = 1, .cc = 32, .xf = true, .ntb = 1, .mt = 4, .wn = 2, .up = true},
            CmForm{.ks = 5, .s = 1, .cc = 16, .xf = true, .ntb = 1, .mt = 4, .xc = true, .wn = 2, .up = true},
            CmForm{.ks = 5, .s = 1, .cc = 16, .xf = true, .ntb = 1, .mt = 4, .xc = true, .wn = 2, .up = true, .xo = true},
            CmForm{.ks = 3, .s = 1, .cc = 32, .ntb = 1, .mt = 4, .wn = 2, .dil = 2}, CmForm{.ks = 3, .s = 1, .cc = 32, .ntb = 1, .mt = 2, .wn = 2, .dil = 4},
            // the single-f16 mode (CmForm::h1): R2D2's conv1, conv2, conv3 / conv4, conv5
            CmForm{.ks = 3, .s = 1, .cc = 32, .ntb = 1, .h1 = true}, CmForm{.ks = 3, .s = 1, .cc = 32, .ntb = 1, .mt = 4, .wn = 2, .h1 = true},
            CmForm{.ks = 3, .s = 1, .cc = 32, .ntb = 1, .mt = 4, .wn = 2, .dil = 2, .h1 = true}, CmForm{.ks = 3, .s = 1, .cc = 32, .ntb = 1, .mt = 2, .wn = 2, .dil = 4, .h1 = true}>(ctx, name, f, a, B);
    }
    int ntb = L.ntb;
    if (o.last_only) {
        // strict fp32: channel 4 x 32 of the fifth tile.  An accumulator's chain of v_mfma_f32_32x32x2_f32 does not depend on the tiles beside it, so the tile launched
        // by itself (its fragments and its bias row, one stored column) gives the logit the five-tile form gives
        a.wp = L.w + (size_t)4 * L.ks * L.ks * a.NCH * 2 * 32 * (CC / 2);
        a.bias = L.b + 128;
        a.COUT = 1; a.nblk = 1; a.ostride = 1;
        ntb = 1;
    }
    return launch_conv_mfma<
        CmForm{.ks = 1, .s = 1, .cc = 32}, CmForm{.ks = 3, .s = 1, .cc = 32}, CmForm{.ks = 3, .s = 1, .cc = 32, .ntb = 1},
        CmForm{.ks = 3, .s = 1, .cc = 32, .pool_out = true}, CmForm{.ks = 3, .s = 2, .cc = 16},
        CmForm{.ks = 5, .s = 1, .cc = 32, .xf = true}, CmForm{.ks = 5, .s = 1, .cc = 16, .xf = true}, CmForm{.ks = 5, .s = 1, .cc = 16, .xf = true, .ntb = 5},
        CmForm{.ks = 5, .s = 1, .cc = 16, .xf = true, .ntb = 1},
        CmForm{.ks = 3, .s = 1, .cc = 32, .dil = 2}, CmForm{.ks = 3, .s = 1, .cc = 32, .dil = 4},
        CmForm{.ks = 2, .s = 1, .cc = 16, .dil = 4}, CmForm{.ks = 2, .s = 1, .cc = 16, .dil = 8}, CmForm{.ks = 2, .s = 1, .cc = 16, .dil = 16}>(
        ctx, name, CmForm{.ks = L.ks, .s = S, .cc = CC, .pool_out = L.pool_out, .xf = x, .ntb = ntb, .dil = L.dil}, a, B);
}

void stage_layer(WeightStage& ws, Layer& L, const char* prefix, const float* w, const float* b)
{
    L.prof = prefix + L.name + (L.h1 ? "_h1" : "");
    if (L.mfma) {
        if (conv_mfma_use_h16() && L.ntb == 5) {       // cout = 4 x 32 + 1: the last channel goes to the VALU side of conv_mfma_h<XC>
            const int T = L.ks * L.ks, co = L.cout - 1;
            const float sc = weight_scale_h(w, (size_t)co * L.cin * T);
            ws.put(pack_mfma_h(w, co, L.cin, L.ks, L.cc, 2, sc), &L.w);
            L.unscale = 1.0f / sc;
            const float xs = weight_scale_h(w + (size_t)co * L.cin * T, (size_t)L.cin * T);
            ws.put(pack_xc_pairs(w + (size_t)co * L.cin * T, L.cin, T, xs), &L.xw);
            L.xun = 1.0f / xs;
            L.xb = b ? b[co] : 0.0f;
        } else if (conv_mfma_use_h16()) {       // tap-major fragments: the same pack serves the halo form, the 1 x 1 product and the tap-gathered one
            const float sc = weight_scale_h(w, (size_t)L.cout * L.cin * L.ks * L.ks);
            ws.put(pack_mfma_h(w, L.cout, L.cin, L.ks, L.cc, L.ntb, sc), &L.w);
            L.unscale = 1.0f / sc;
        } else {
            ws.put(pack_mfma(w, L.cout, L.cin, L.ks, L.cc, L.ntb), &L.w);
        }
        ws.put(pad_bias(b, L.cout, 32 * L.ntb), &L.b);
    } else {
        ws.put(pack_valu(w, L.cout, L.cin, L.ks), &L.w);
        ws.put(pad_bias(b, L.cout, 8), &L.b);
    }
}
