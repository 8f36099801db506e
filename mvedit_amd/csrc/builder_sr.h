// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): SRVGGNetCompact plan.
#pragma once
#include "executor_builder.h"

namespace {

// SRVGGNetCompact.forward (lib/models/decoders/image_space_ss.py:63-70): conv + PReLU stack at the input resolution, last conv to
// out_ch * r * r channels, PixelShuffle(r), plus the nearest-upsampled input.  H x W is the input size.
int Builder::build_sr(int B_, int H, int W, int io_dtype) {
    begin(B_, H, W, 1, io_dtype);
    const int e = 2, d = dt, F = c.ch[0], r = c.sr_scale, last = 2 * (c.layers_per_block + 1);
    const int opad = (c.out_ch * r * r + 7) & ~7;
    MVE_CHECK((size_t)B_ * H * W * (size_t)(F > opad * 2 ? F : opad * 2) < ((size_t)1 << 31), MVE_ERR_ARG,
              "srvgg: batch %d at %dx%d overflows 32-bit activation indexing; enhance in smaller batches", B_, H, W);
    const int M = B_ * H * W;
    rows_img = H * W;
    const Ref src = arg(Ref::SAMPLE), dst = arg(Ref::OUT);
    Ref cur = ws((size_t)M * 8 * e);
    to_nhwc(src, B_, c.in_ch, H, W, 8, cur);
    int cin = 8;
    for (int k = 0; k <= c.layers_per_block; ++k) {
        const std::string b = "body." + std::to_string(2 * k);
        Ref y = ws((size_t)M * F * e);
        conv(cur, cin, B_, H, W, 1, 0, wt(b + ".w"), F, y, wt(b + ".b"), Ref(), 0, Ref(), 0, "conv");
        rel(cur);
        Ref a = wt("body." + std::to_string(2 * k + 1) + ".a");
        const size_t nel = (size_t)M * F;
        op(OC_OTHER, 0, "prelu", [=](const Run& rr) { return mve_prelu(d, rr.p(y), (const float*)rr.p(a), F, rr.p(y), nel, rr.stream); });
        cur = y; cin = F;
    }
    Ref o = ws((size_t)M * opad * 4);
    conv(cur, F, B_, H, W, 1, 0, wt("body." + std::to_string(last) + ".w"), opad, o, wt("body." + std::to_string(last) + ".b"), Ref(), 0, Ref(),
         MVE_GEMM_OUT_F32, "conv (to r*r sub-pixels)");
    rel(cur);
    const int oc = c.out_ch;
    live(o, "pixel shuffle");
    op(OC_OTHER, 0, "pixel shuffle + nearest-upsampled input", [=](const Run& rr) {
        return mve_pixel_shuffle_add(io_dtype, (const float*)rr.p(o), opad, rr.p(src), B_, oc, H, W, r, rr.p(dst), rr.stream);
    });
    return finish("srvgg");
}

}  // namespace
