// conv1a_rgb.h -- the first layer of the nets whose trunk starts 3 -> 64, 3 x 3, bias, ReLU on the planar RGB image (SFD2's conv1a, D2-Net's conv1_1): on the
// vector ALU at full resolution (27 taps; conv1a_c64's column walk), with the packing of its weights.  Its 64-channel map is written and read back once
// (2 x 79 MB per 480 x 640 image): generating it inside the next layer's staging, as SuperPoint does, is not built.
#pragma once
#include "conv_mfma.h"

namespace {

// 16 lanes share a pixel, each keeps the 27 taps of its 4 output channels in registers and walks down a column; a wave store is 4 whole 256-byte pixels.
// Every output is bias, then the taps in (kx, channel) order of rows y - 1, y, y + 1 interleaved, an fma each; a tap outside the image is zero.
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

// OIHW [64][3][3][3] -> conv1a_rgb64's [ky][kx][c][64]
inline std::vector<float> pack_conv1a_rgb64(const float* w)
{
    std::vector<float> p(27 * 64);
    for (int o = 0; o < 64; ++o)
        for (int c = 0; c < 3; ++c)
            for (int t = 0; t < 9; ++t) p[(t * 3 + c) * 64 + o] = w[(o * 3 + c) * 9 + t];
    return p;
}

inline void launch_conv1a_rgb64(kpb_ctx* ctx, const char* tag, const float* img, float* out, const float* w, const float* bias, int batch, int H, int W)
{
    KPB_LAUNCH(ctx, tag, conv1a_rgb64, dim3(cdiv(W, 16), cdiv(H, 32), batch), dim3(256), 0, ctx->stream, img, out, w, bias, H, W, 32);
}

}  // namespace
