// conv_layer.h -- the dense-layer path of the six networks whose convolutions run on conv_mfma.h's three kernel families (SuperPoint, XFeat, DISK in
// convnet.hip; r2d2.hip, sfd2.hip, d2net.hip): a layer is described once (Layer), staged once (stage_layer: the one copy of the pack rule) and launched one
// way (launch_mfma: the one copy of "ConvM from the layer, form from the layer's fields").  Declarations only -- conv_layer.hip defines them and is the one
// translation unit that instantiates the generic forms of conv_mfma_h, conv_mfma and gemm_h.
#pragma once
#include "net.h"

struct Layer {      // one convolution of a network plan
    std::string name;
    int cin, cout, ks, stride;
    bool mfma;
    bool relu = true;           // ReLU on the output
    bool pool_out = false;      // the output max-pooled 2 x 2 (SuperPoint's MaxPool2d after conv1b / 2b / 3b)
    int dil = 1;                // dilation (CmForm::dil; R2D2), padding (ks - 1) dil / 2
    int cc = 32;    // channels per LDS chunk of conv_mfma (32, or 16 for stride 2 / CIN not a multiple of 32)
    int ntb = 2;    // 32-wide output tiles per workgroup
    // what a launch needs of the staged weights, bound once at create by stage_layer: host scalars, device pointers and the profile name
    float unscale = 1.0f;               // split-f16 form: 1 / the power-of-two scale the pack was made with (conv_mfma_h)
    float xb = 0.0f, xun = 1.0f;        // ntb == 5 (DISK up_3): the score channel's bias and 1 / the scale of its pack
    const float *w = nullptr, *b = nullptr, *xw = nullptr;
    const float* slope = nullptr;       // DISK: the PReLU slopes of the layer's input
    std::string prof;                   // profile name of its launch
    // the single-f16 matrix mode (CmForm::h1), set by the net's create BEFORE stage_layer: one MFMA a_hi * b_hi per product on the same pack and LDS layout;
    // profile name + "_h1".  launch_mfma refuses it (KPB_E_INVALID) on a layer whose form has no such instance, and on the strict-fp32 path
    bool h1 = false;
};

struct UpSrc { const float* src; int c; };      // ConvM::up_src, up_c
struct PreSplit { const unsigned* amax = nullptr; float l1 = 0.0f, bmax = 0.0f; const float* gen_w = nullptr; const float* gen_b = nullptr; };     // ConvM::pre_*, gen_*

// What one launch_mfma call adds to its layer, by designated initialisers: launch_mfma(..., {.xf = xf, .up = &up})
struct MfmaOpt {
    const float* xf = nullptr;          // ConvM::xf: DISK's InstanceNorm + PReLU of the input, applied while it is staged
    const PreSplit* pre = nullptr;      // SuperPoint conv1b: its input generated from the grey image while the tile is staged
    const UpSrc* up = nullptr;          // DISK up2 / up3: the upsampled input channels evaluated while the tile is staged
    int unfold_w = 0;                   // XFeat keypoint_head.0: the 8 x 8 cells of a [B][8 H][unfold_w] image read in place (ConvM::unfold_w),
    const float2* unfold_mr = nullptr;  // normalised by the per-image (mean, 1 / std) as they are read
    float l2_eps = 0.0f;                // > 0: F.normalize(eps = l2_eps) of every output row in the epilogue (XFeat block_fusion.2, split-f16 form)
    const float* res = nullptr;         // the identity map of a ResBlock [B][H][W][cout], added before the ReLU (SFD2; 1 x 1 layers only)
    bool last_only = false;             // ntb == 5 layers (DISK up_3): `out` is [B][H][W] and receives the LAST output channel alone (the score logit), with the
                                        // bits the full layer gives it -- conv_mfma_h<xo> (profile name + "_score"), or the fifth tile by itself on the strict-fp32 path
};

// L is the net's own Layer (net->L[i]): the stage binds its pointers at the upload.  Profile name = prefix + layer name: "sp_conv1b", "xf_block2.0", "disk_up3"
void stage_layer(WeightStage& ws, Layer& L, const char* prefix, const float* w, const float* b);

// One layer with L.mfma on the matrix cores: (Hi, Wi) -> (Hi, Wi) / stride, halved once more with pool_out
int launch_mfma(kpb_ctx* ctx, const Layer& L, const float* in, float* out, int B, int Hi, int Wi, const MfmaOpt& o = {});

// The first layer of the trunks that start on the planar RGB image [B][3][H][W]: 3 x 3, padding 1, bias, ReLU on the vector ALU, out [B][H][W][cout].  Weights and
// bias as stage_layer leaves them for an mfma = false layer: [tap][c][cout].  conv_rgb32 (R2D2 conv0, ALIKE-l block1.conv1): one pixel x 8 output channels per
// thread.  conv1a_rgb64 (SFD2 conv1a, D2-Net conv1_1): 16 lanes share a pixel and walk down a column; its 64-channel map is written and read back once (2 x 79 MB per
// 480 x 640 image): generating it inside the next layer's staging, as SuperPoint does, is not built.
void launch_conv_rgb32(kpb_ctx* ctx, const char* tag, const float* img, float* out, const float* w, const float* bias, int batch, int H, int W);
void launch_conv1a_rgb64(kpb_ctx* ctx, const char* tag, const float* img, float* out, const float* w, const float* bias, int batch, int H, int W);

// max_pool2d(x, K, K) of an NHWC map [B][K Ho][K Wo][C] -> [B][Ho][Wo][C], K = 2 or 4, C a multiple of 4 (the ALIKE family's pools)
void launch_maxpool_nhwc(kpb_ctx* ctx, const char* tag, int K, const float* in, float* out, int batch, int Ho, int Wo, int C);

// convnet.hip's l2norm_nhwc for the nets of other translation units: every C-channel row of an NHWC map divided by its L2 norm in place, the norm clamped from
// below at eps_clamp when that is > 0 (F.normalize)
void launch_l2norm_nhwc(kpb_ctx* ctx, const char* tag, float* desc, int C, size_t npix, float eps_clamp);
