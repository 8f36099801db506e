// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): Segment Anything image encoder plan.
#pragma once
#include "executor_builder.h"

namespace {

// segment_anything's ImageEncoderViT.forward = transformers' SamVisionEncoder.forward (models/sam/modeling_sam.py), the network behind
// `SamPredictor.set_image` (lib/apis/adapter3d.py:363-372, :723-734; lib/pipelines/utils.py:114-131).  With G = image_size / patch_size,
// C = hidden_size, hd = C / heads:
//   1. patch_embed: Conv2d(3, C, kernel = stride = patch, WITH bias) as a GEMM over mve_clip_patchify rows -> [B, G, G, C]; + pos_embed [1, G, G, C]
//      in fp32 with one rounding (mve_sam_pos_add).  This is hidden state 0.
//   2. per block: s = x; x = LayerNorm(x) (eps = layer_norm_eps).  A windowed block (w = window_size) zero-pads the NORMALISED map at the bottom
//      and right to Gp = w * ceil(G / w) and cuts it into (Gp / w)^2 windows of w^2 tokens (mve_sam_window_partition).  The padded tokens are real
//      tokens: they pass through qkv (their q, k, v equal the bias), they are attended to as keys inside their window, and their output rows are
//      dropped on un-partition.  Attention per (window or image, head):
//          softmax_k( scale q.k + q.Rh[qh - kh + (n-1)] + q.Rw[qw - kw + (n-1)] ) v,   n = w (windowed) or G (global), scale = hd^-1/2,
//      the UNSCALED q against the tables rel_pos_h / rel_pos_w [2n-1, hd] (mve_attention_relpos).  Then proj, x = s + x, and
//      x = x + lin2(GELU_erf(lin1(LayerNorm(x)))).  Global blocks are those of global_attn_indexes (Config::sm_global).
//   3. neck: conv 1 x 1 C -> O without bias, LayerNorm2d, conv 3 x 3 O -> O (pad 1, no bias), LayerNorm2d -- LayerNorm2d normalises over the
//      channels of a pixel, i.e. mve_layernorm over NHWC rows, eps 1e-6 -- then NHWC -> NCHW [B, O, G, G].
// `proj` acts per row, so it runs AFTER un-partition on the B G^2 kept rows with the residual in its epilogue -- the same numbers as projecting
// the padded rows and adding afterwards, without the GEMM over rows that are dropped and without an add pass.  Un-partition is data movement only.
// GEMMs never split K (rows_img = 0) and mve_attention_relpos works per (sequence, head, query tile): an item's result does not depend on B.
// Pixels arrive as Run::sample ([B,3,S,S] NCHW, engine dtype), the neck output leaves through Run::out, hidden state k through Run::cn_out[k].
int Builder::build_sam(int B_) {
    const int S = c.sm_image, Pz = c.sm_patch, G = S / Pz, G2 = G * G, Kp = (3 * Pz * Pz + 7) / 8 * 8, w = c.sm_window, nW = (G + w - 1) / w;
    begin(B_, S, S, 1, c.dtype);
    const int e = 2, d = dt, Bn = B_, C = c.ch[0], I = c.clip_inter, O = c.sm_out, heads = c.heads[0], hd = C / heads;
    const float eps = c.eps, scale = 1.0f / sqrtf((float)hd);
    const size_t widest = (size_t)(I > 3 * C ? I : 3 * C) > (size_t)Kp ? (size_t)(I > 3 * C ? I : 3 * C) : (size_t)Kp;
    MVE_CHECK((size_t)Bn * nW * nW * w * w * widest < ((size_t)1 << 31) && (size_t)Bn * 3 * S * S < ((size_t)1 << 31), MVE_ERR_ARG,
              "sam_encoder: batch %d overflows 32-bit activation indexing", Bn);
    const int M = Bn * G2, Mw = Bn * nW * nW * w * w;
    const size_t bytes = (size_t)M * C * e;
    const Ref px = arg(Ref::SAMPLE);
    Ref x = ws(bytes);
    {
        Ref rows = ws((size_t)M * Kp * e);
        op(OC_OTHER, 0, "patchify", [=](const Run& r) { return mve_clip_patchify(d, r.p(px), Bn, S, S, Pz, r.p(rows), Kp, r.stream); });
        Ref patch = ws(bytes);
        dense(rows, wt("patch_embed.projection.w"), wt("patch_embed.projection.b"), patch, M, C, Kp, Ref(), "patch_embed");
        rel(rows);
        const Ref pos = wt("pos_embed");
        live(patch, "position embedding"); live(x, "position embedding");
        op(OC_OTHER, 0, "position embedding", [=](const Run& r) { return mve_sam_pos_add(d, r.p(patch), r.p(pos), r.p(x), Bn, G2, C, r.stream); });
        rel(patch);
    }
    copy_out(x, bytes, 0, "hidden state -> output");
    for (int k = 0; k < c.layers_per_block; ++k) {
        const std::string p = "layers." + std::to_string(k);
        const bool global = (c.sm_global >> k) & 1ull;
        const int n = global ? G : w, rowsA = global ? M : Mw, NS = global ? Bn : Bn * nW * nW;
        Ref src = ws(bytes);
        layernorm(x, C, src, M, C, p + ".layer_norm1", eps);
        if (!global) {
            Ref win = ws((size_t)Mw * C * e);
            live(src, "window partition"); live(win, "window partition");
            op(OC_OTHER, 0, "window partition", [=](const Run& r) { return mve_sam_window_partition(d, r.p(src), Bn, G, C, w, r.p(win), r.stream); });
            rel(src); src = win;
        }
        Ref qkv = ws((size_t)rowsA * 3 * C * e);
        dense(src, wt(p + ".attn.qkv.w"), wt(p + ".attn.qkv.b"), qkv, rowsA, 3 * C, C, Ref(), "attn.qkv");
        rel(src);
        Ref a = ws((size_t)rowsA * C * e);
        {
            const Ref q = qkv, kk = at(qkv, (size_t)C * e), v = at(qkv, (size_t)2 * C * e), rh = wt(p + ".attn.rel_pos_h"), rw = wt(p + ".attn.rel_pos_w");
            const char* what = global ? "rel-pos attention (global)" : "rel-pos attention (windows)";
            live(qkv, what); live(a, what);
            op(OC_ATTN, 4.0 * NS * heads * (double)(n * n) * (n * n) * hd, what, [=](const Run& r) {
                return mve_attention_relpos(d, r.p(q), 3 * C, r.p(kk), 3 * C, r.p(v), 3 * C, r.p(rh), r.p(rw), r.p(a), C, NS, n, n, heads, hd, scale, r.stream);
            });
        }
        rel(qkv);
        if (!global) {
            Ref un = ws(bytes);
            live(a, "window un-partition"); live(un, "window un-partition");
            op(OC_OTHER, 0, "window un-partition", [=](const Run& r) { return mve_sam_window_unpartition(d, r.p(a), Bn, G, C, w, r.p(un), r.stream); });
            rel(a); a = un;
        }
        Ref x2 = ws(bytes);
        dense(a, wt(p + ".attn.proj.w"), wt(p + ".attn.proj.b"), x2, M, C, C, x, "attn.proj+residual");
        rel(a); rel(x);
        Ref n2 = ws(bytes);
        layernorm(x2, C, n2, M, C, p + ".layer_norm2", eps);
        Ref f = ws((size_t)M * I * e);
        dense(n2, wt(p + ".mlp.lin1.w"), wt(p + ".mlp.lin1.b"), f, M, I, C, Ref(), "mlp.lin1");
        rel(n2);
        act(f, (size_t)M * I, MVE_ACT_GELU, "gelu");
        Ref x3 = ws(bytes);
        dense(f, wt(p + ".mlp.lin2.w"), wt(p + ".mlp.lin2.b"), x3, M, C, I, x2, "mlp.lin2+residual");
        rel(f); rel(x2);
        x = x3;
        copy_out(x, bytes, k + 1, "hidden state -> output");
    }
    Ref y = conv1x1(x, M, C, "neck.conv1.w", Ref(), O, "neck.conv1");
    rel(x);
    Ref yn = ws((size_t)M * O * e);
    layernorm(y, O, yn, M, O, "neck.layer_norm1", 1e-6f);      // SamLayerNorm / LayerNorm2d: eps 1e-6 whatever the blocks use
    rel(y);
    y = conv3x3(yn, O, Bn, G, G, 1, "neck.conv2.w", Ref(), O, Ref(), 0, "neck.conv2");
    rel(yn);
    yn = ws((size_t)M * O * e);
    layernorm(y, O, yn, M, O, "neck.layer_norm2", 1e-6f);
    rel(y);
    to_nchw(yn, d, O, Bn, O, G, G);
    rel(yn);
    return finish("sam_encoder");
}

}  // namespace
