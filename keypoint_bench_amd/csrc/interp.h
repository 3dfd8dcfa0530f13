// interp.h -- torch's three interpolation rules, each stated once for every kernel (and the host) that needs it.  Parity with the reference rests on the
// operation ORDER of these few lines, so a kernel calls them and never retypes them (tests/test_interp_cpu.py pins them against torch itself).
// Device-inline functions only (no kernel lives here); a host compiler sees plain inline functions.  Build with -ffp-contract=off, as build.py does.  At the
// callers stay, on purpose: the clamps of lh_taps, d2_upsample and kn_lin_taps (applied to the result of these functions), the fused fmaf blends of up8ch_lerp4,
// alike_desc_at and alike_l_desc_at (documented there), how a grid coordinate is made and how validity becomes an address.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KPB_HD __host__ __device__ __forceinline__
#else
#define KPB_HD static inline
#endif
// One axis of a bilinear read: source samples i0 <= i1 and the weight l of i1 (1 - l of i0); the second tap stays on the last sample of a source of n.
struct kpb_lin { int i0, i1; float l; };
KPB_HD kpb_lin kpb_lin_at(float f, int n)
{
    const int i0 = (int)f;
    return kpb_lin{i0, i0 + (i0 < n - 1 ? 1 : 0), f - (float)i0};
}
// F.interpolate / nn.Upsample(bilinear, align_corners = True): output o reads source coordinate scale * o, scale = kpb_ac_scale(n_src, n_dst) -- one float
// division, the same on host and device (_gt1: n_dst > 1 is the caller's precondition, no select in a kernel)
KPB_HD float kpb_ac_scale_gt1(int n_src, int n_dst) { return (float)(n_src - 1) / (float)(n_dst - 1); }
KPB_HD float kpb_ac_scale(int n_src, int n_dst) { return n_dst > 1 ? kpb_ac_scale_gt1(n_src, n_dst) : 0.0f; }
KPB_HD kpb_lin kpb_tap_ac(int o, int n, float scale) { return kpb_lin_at(scale * (float)o, n); }
// F.interpolate(bilinear, align_corners = False): output o reads source coordinate max((o + 0.5) scale - 0.5, 0), scale = n_src / n_dst
KPB_HD kpb_lin kpb_tap_hp(int o, int n, float scale) { return kpb_lin_at(fmaxf(((float)o + 0.5f) * scale - 0.5f, 0.0f), n); }
// torch's blend of taps (y0, x0), (y0, x1), (y1, x0), (y1, x1): columns first, then rows, nothing fused
KPB_HD float kpb_mix(float p00, float p01, float p10, float p11, float ly, float lx)
{
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    return hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11);
}
// the same blend of the taps at(iy, ix) reads, the weights formed BEFORE the reads, as the scalar kernels were written (same values; the schedule follows the source)
template <class At>
KPB_HD float kpb_mix_at(const kpb_lin& ty, const kpb_lin& tx, At at)
{
    const float hy = 1.0f - ty.l, hx = 1.0f - tx.l;
    return hy * (hx * at(ty.i0, tx.i0) + tx.l * at(ty.i0, tx.i1)) + ty.l * (hx * at(ty.i1, tx.i0) + tx.l * at(ty.i1, tx.i1));
}
#if defined(__HIPCC__)
KPB_HD float4 kpb_mix4(const float4 p00, const float4 p01, const float4 p10, const float4 p11, float ly, float lx)
{
    return make_float4(kpb_mix(p00.x, p01.x, p10.x, p11.x, ly, lx), kpb_mix(p00.y, p01.y, p10.y, p11.y, ly, lx),
                       kpb_mix(p00.z, p01.z, p10.z, p11.z, ly, lx), kpb_mix(p00.w, p01.w, p10.w, p11.w, ly, lx));
}
#endif
// F.grid_sample(bilinear, zeros, align_corners = True) at grid coordinate (gx, gy) in [-1, 1] of a W x H map: ATen's un-normalisation (g + 1) * ((size - 1) / 2),
// the floored corner (x0, y0) -- as floats: a caller converts to the integer width it addresses with -- and the weights of taps (y0, x0), (y0, x0 + 1),
// (y0 + 1, x0), (y0 + 1, x0 + 1).  A tap outside the map contributes zero: the caller masks it (a select, never 0 x something) before kpb_grid_blend.
struct kpb_grid { float x0, y0; float w[4]; };
KPB_HD kpb_grid kpb_grid_taps(float gx, float gy, int W, int H)
{
    const float x = (gx + 1.0f) * ((float)(W - 1) / 2.0f), y = (gy + 1.0f) * ((float)(H - 1) / 2.0f);
    const float xw = floorf(x), yn = floorf(y);
    const float w = x - xw, e = 1.0f - w, nn = y - yn, s = 1.0f - nn;
    return kpb_grid{xw, yn, {s * e, s * w, nn * e, nn * w}};
}
// ((nw w0 + ne w1) + sw w2) + se w3 on four already-masked taps, every product and sum rounded on its own
KPB_HD float kpb_grid_blend(float nw, float ne, float sw, float se, const float* w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(nw, w[0]), __fmul_rn(ne, w[1])), __fmul_rn(sw, w[2])), __fmul_rn(se, w[3]));
#else
    return ((nw * w[0] + ne * w[1]) + sw * w[2]) + se * w[3];
#endif
}
