"""scripts/hack_build.py r2d2_gather3 profiles/r2d2_gather3x3_partner.py -- the A/B partner of profiles/r2d2_rate.json: R2D2's dilated 3 x 3 layers
(conv3 .. 5) on the tap-gathered gemm_h form (K = 9 x cin) instead of the halo tile of conv_mfma_h<dil>."""
import os


def patch(csrc):
    sub(os.path.join(csrc, "r2d2.hip"), "        if (L.ks == 2) {        // tap-gathered product: K = 4 taps x cin,", "        if (L.ks == 2 || L.dil > 1) {        // tap-gathered product: K = ks^2 taps x cin,")
    sub(os.path.join(csrc, "r2d2.hip"), "            a.NCH = 4 * (L.cin / 32); a.tap_dil = L.dil;\n            KPB_LAUNCH(ctx, L.name, (gemm_h<2, 1, GE_PLAIN, false, 2>),",
        "            a.NCH = L.ks * L.ks * (L.cin / 32); a.tap_dil = L.dil;\n            if (L.ks == 3) KPB_LAUNCH(ctx, L.name, (gemm_h<2, 1, GE_PLAIN, false, 3>), dim3(cdiv(H * W, 128), 1, batch * a.nblk), dim3(256), 0, ctx->stream, a);\n            else KPB_LAUNCH(ctx, L.name, (gemm_h<2, 1, GE_PLAIN, false, 2>),")
