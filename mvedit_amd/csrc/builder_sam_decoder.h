// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): Segment Anything prompt encoder + mask decoder plan.
#pragma once
#include "executor_builder.h"

namespace {

// transformers' SamPromptEncoder + SamMaskDecoder (SamTwoWayAttentionBlock, SamTwoWayTransformer; models/sam/modeling_sam.py) = segment_anything's
// PromptEncoder + MaskDecoder + TwoWayTransformer: what `SamPredictor.predict` runs per prompt (lib/apis/adapter3d.py:721-735,
// lib/pipelines/utils.py:108-146).  fp32 throughout.  N = B * P items (B images, P prompts per image), T tokens per item, G the
// embedding grid, C = hidden_size, Mt = num_mask_tokens:
//   tokens [N, T, C]   = [iou token | Mt mask tokens | points (+ padding point) | box corners]              (mve_sam_prompt_tokens)
//   keys   [N, G^2, C] = embedding of image n / P as pixel rows + no_mask_embed                             (mve_sam_src)
//   queries = tokens; pe = tokens (the point embedding); key_pe = the dense positional encoding [G^2, C] (mve_sam_dense_pe, once at load)
//   attention(q_in, k_in, v_in) = out_proj( softmax_heads( q_proj(q_in) k_proj(k_in)^T hd^-1/2 ) v_proj(v_in) ); self-attention projects to C
//   (head_dim C / heads = 32), the cross-attentions to C / 2 (head_dim 16)
//   layer k:
//     self-attention: k = 0: queries = attention(queries, queries, queries)              (no pe, and the result REPLACES the tokens)
//                     else : queries = queries + attention(queries + pe, queries + pe, queries)
//                     queries = layer_norm1(queries)
//     token -> image: queries = layer_norm2(queries + attention(queries + pe, keys + key_pe, keys))
//     MLP           : queries = layer_norm3(queries + lin2(ReLU(lin1(queries))))
//     image -> token: keys = layer_norm4(keys + attention(keys + key_pe, queries + pe, queries))
//   after the layers: queries = layer_norm_final_attn(queries + final_attention(queries + pe, keys + key_pe, keys))      (eps sd_eps_final)
//   up [N, 16 G^2, C/8] = GELU(convT2(GELU(LayerNorm2d(convT1(keys)))))                                     (mve_sam_upscale twice, LayerNorm2d eps 1e-6)
//   hyper_in [N, Mt, C/8] = MLP_m(queries[:, 1 + m]); iou [N, Mt] = iou_head(queries[:, 0])                 (mve_sam_token_mlps)
//   low_res [N, Mt, 4G, 4G] = hyper_in @ up^T                                                              (mve_sam_mask_product)
// Every residual add rides in the epilogue of the out_proj / lin2 GEMM; the LayerNorm behind it runs in place.  The plan returns ALL Mt masks:
// multimask_output selects [1:] or [:1] of them on the caller's side.  Nothing is read back to the host.
// The embedding arrives as Run::sample, the prompts as Run::sd_boxes / sd_points / sd_labels, low_res leaves through Run::out, iou through
// Run::cn_out[0], tap k through Run::cn_out[1 + k] (include/mvedit_amd.h lists them).
int Builder::build_sam_decoder(int N_, int P, int n_points, int has_box) {
    begin(N_, P, n_points, 1, c.dtype);
    pl.has_res = has_box;
    const int N = N_, C = c.ch[0], heads = c.heads[0], L = c.layers_per_block, I = c.clip_inter, Mt = c.sd_masks, G = c.sd_grid, G2 = G * G, Ci = C / 2, C4 = C / 4, C8 = C / 8;
    const int d = c.dtype, pad = n_points > 0 && !has_box ? 1 : 0, T = 1 + Mt + n_points + pad + 2 * has_box;
    const float eps = c.eps, eps_final = c.sd_eps_final, S = (float)c.sd_image;
    MVE_CHECK(has_box || n_points > 0, MVE_ERR_ARG, "sam_decoder: no prompt (neither a box nor points)");
    MVE_CHECK(T <= 16, MVE_ERR_ARG, "sam_decoder: %d tokens exceed the 16 the kernels take", T);
    MVE_CHECK(N >= 1 && N <= 128 && P >= 1 && N % P == 0, MVE_ERR_ARG, "sam_decoder: bad N %d (1..128 items) / P %d", N, P);
    const int Mq = N * T, Mk = N * G2;
    const size_t qb = (size_t)Mq * C * 4, kb = (size_t)Mk * C * 4;
    const int n_taps = 2 * L + 5;

    // fp32 ops over this plan's buffers --------------------------------------------------------------------------------------------------------
    auto gemm32 = [&](Ref A, Ref out, int M, int Nn, int K, const std::string& slot, Ref res, int relu, const char* what) {
        const Ref W = wt(slot + ".w"), bias = wt(slot + ".b");
        live(A, what); live(out, what); live(res, what);
        op(OC_LINEAR, 2.0 * M * Nn * K, what, [=](const Run& r) {
            return mve_gemm_f32((const float*)r.p(A), K, (const float*)r.p(W), K, (const float*)r.p(bias), (const float*)r.p(res), Nn, (float*)r.p(out), Nn, M, Nn, K, relu,
                                r.stream);
        });
    };
    auto ln32 = [&](Ref x, int rows, const std::string& slot, float e) {
        const Ref g = wt(slot + ".g"), b = wt(slot + ".b");
        live(x, "layernorm");
        op(OC_NORM, 0, "layernorm", [=](const Run& r) {
            return mve_layernorm_f32((const float*)r.p(x), (float*)r.p(x), rows, C, (const float*)r.p(g), (const float*)r.p(b), e, r.stream);
        });
    };
    auto add32 = [&](Ref x, Ref pe, Ref y, int rows, int period, const char* what) {
        live(x, what); live(pe, what); live(y, what);
        op(OC_OTHER, 0, what, [=](const Run& r) { return mve_add_rows_f32((const float*)r.p(x), (const float*)r.p(pe), (float*)r.p(y), rows, C, period, r.stream); });
    };
    // out = res + out_proj(attention(q_proj(q_in), k_proj(k_in), v_proj(v_in))) over Lq queries / Lk keys per item, projected to `inner` columns
    auto attention = [&](const std::string& p, Ref q_in, Ref k_in, Ref v_in, int Lq, int Lk, int inner, Ref res, Ref out, const char* what) {
        const int hd = inner / heads;
        Ref q = ws((size_t)N * Lq * inner * 4), k = ws((size_t)N * Lk * inner * 4), v = ws((size_t)N * Lk * inner * 4);
        gemm32(q_in, q, N * Lq, inner, C, p + ".q_proj", Ref(), 0, "attn.q_proj");
        gemm32(k_in, k, N * Lk, inner, C, p + ".k_proj", Ref(), 0, "attn.k_proj");
        gemm32(v_in, v, N * Lk, inner, C, p + ".v_proj", Ref(), 0, "attn.v_proj");
        Ref a = ws((size_t)N * Lq * inner * 4);
        const float scale = 1.0f / sqrtf((float)hd);
        live(a, what);
        op(OC_ATTN, 4.0 * N * heads * (double)Lq * Lk * hd, what, [=](const Run& r) {
            return mve_attention_f32((const float*)r.p(q), inner, (const float*)r.p(k), inner, (const float*)r.p(v), inner, (float*)r.p(a), inner, N, Lq, Lk, heads, hd, scale,
                                     r.stream);
        });
        rel(q); rel(k); rel(v);
        gemm32(a, out, N * Lq, C, inner, p + ".out_proj", res, 0, res.kind == Ref::NUL ? "attn.out_proj" : "attn.out_proj+residual");
        rel(a);
    };
    auto tap = [&](Ref x, size_t bytes, int k) { copy_out(x, bytes, 1 + k, "tap -> output"); };

    // prompt tokens and image rows -------------------------------------------------------------------------------------------------------------
    const Ref tokens = ws(qb);
    {
        const Ref gs = wt("gaussian"), pemb = wt("point_embed"), nap = wt("not_a_point"), it = wt("iou_token"), mt = wt("mask_tokens");
        op(OC_OTHER, 0, "prompt tokens", [=](const Run& r) {
            return mve_sam_prompt_tokens(has_box ? r.sd_boxes : nullptr, n_points ? r.sd_points : nullptr, n_points ? r.sd_labels : nullptr, N, n_points, (const float*)r.p(gs),
                                         (const float*)r.p(pemb), (const float*)r.p(nap), (const float*)r.p(it), (const float*)r.p(mt), Mt, C, S, (float*)r.p(tokens), T, r.stream);
        });
    }
    tap(tokens, qb, 0);
    Ref keys = ws(kb);
    {
        const Ref emb = arg(Ref::SAMPLE), nm = wt("no_mask");
        op(OC_OTHER, 0, "embedding -> rows + no_mask_embed", [=](const Run& r) { return mve_sam_src(d, r.p(emb), (const float*)r.p(nm), (float*)r.p(keys), N, P, C, G, r.stream); });
    }
    const Ref dense_pe = wt("dense_pe");
    Ref queries = tokens;          // layer 0 reads the tokens themselves; every later `queries` is a buffer of its own
    Ref qpe = ws(qb), kpe = ws(kb);
    for (int k = 0; k < L; ++k) {
        const std::string b = "mask_decoder.transformer.layers." + std::to_string(k);
        Ref q1 = ws(qb);
        if (k == 0) {
            attention(b + ".self_attn", queries, queries, queries, T, T, C, Ref(), q1, "self-attention");
        } else {
            add32(queries, tokens, qpe, Mq, Mq, "queries + pe");
            attention(b + ".self_attn", qpe, qpe, queries, T, T, C, queries, q1, "self-attention");
            rel(queries);
        }
        queries = q1;
        ln32(queries, Mq, b + ".layer_norm1", eps);
        add32(queries, tokens, qpe, Mq, Mq, "queries + pe");
        add32(keys, dense_pe, kpe, Mk, G2, "keys + dense pe");
        Ref q2 = ws(qb);
        attention(b + ".cross_attn_token_to_image", qpe, kpe, keys, T, G2, Ci, queries, q2, "attention tokens -> image");
        rel(queries); queries = q2;
        ln32(queries, Mq, b + ".layer_norm2", eps);
        Ref h = ws((size_t)Mq * I * 4), q3 = ws(qb);
        gemm32(queries, h, Mq, I, C, b + ".mlp.lin1", Ref(), 1, "mlp.lin1+relu");
        gemm32(h, q3, Mq, C, I, b + ".mlp.lin2", queries, 0, "mlp.lin2+residual");
        rel(h); rel(queries); queries = q3;
        ln32(queries, Mq, b + ".layer_norm3", eps);
        add32(queries, tokens, qpe, Mq, Mq, "queries + pe");
        Ref k2 = ws(kb);
        attention(b + ".cross_attn_image_to_token", kpe, qpe, queries, G2, T, Ci, keys, k2, "attention image -> tokens");
        rel(keys); keys = k2;
        ln32(keys, Mk, b + ".layer_norm4", eps);
        tap(queries, qb, 1 + 2 * k);
        tap(keys, kb, 2 + 2 * k);
    }
    {
        add32(queries, tokens, qpe, Mq, Mq, "queries + pe");
        add32(keys, dense_pe, kpe, Mk, G2, "keys + dense pe");
        Ref qf = ws(qb);
        attention("mask_decoder.transformer.final_attn_token_to_image", qpe, kpe, keys, T, G2, Ci, queries, qf, "final attention tokens -> image");
        if (L > 0) rel(queries);
        queries = qf;
        ln32(queries, Mq, "mask_decoder.transformer.layer_norm_final_attn", eps_final);
        tap(queries, qb, 1 + 2 * L);
    }
    rel(qpe); rel(kpe);
    // upscaling, hypernetworks, masks ----------------------------------------------------------------------------------------------------------
    Ref up = keys;
    for (int k = 0; k < 2; ++k) {
        const std::string u2 = "mask_decoder.upscale_conv" + std::to_string(k + 1);
        const int Gi = G << k, cin = k ? C4 : C, cout = k ? C8 : C4, mode = k ? 2 : 1;
        Ref tmp = ws((size_t)N * Gi * Gi * 4 * cout * 4), y = ws((size_t)N * 4 * Gi * Gi * cout * 4);
        const Ref W4 = wt(u2 + ".w"), bias = wt(u2 + ".b"), g = wt("mask_decoder.upscale_layer_norm.g"), bb = wt("mask_decoder.upscale_layer_norm.b");
        const char* what = k ? "upscale_conv2+gelu" : "upscale_conv1+layernorm2d+gelu";
        live(up, what);
        op(OC_CONV, 2.0 * N * Gi * Gi * (double)cin * 4 * cout, what, [=](const Run& r) {
            return mve_sam_upscale((const float*)r.p(up), (const float*)r.p(W4), (const float*)r.p(bias), (const float*)r.p(g), (const float*)r.p(bb), 1e-6f, (float*)r.p(tmp),
                                   (float*)r.p(y), N, Gi, cin, cout, mode, r.stream);
        });
        rel(tmp); rel(up); up = y;
    }
    const int P2 = 16 * G2;
    tap(up, (size_t)N * P2 * C8 * 4, 2 + 2 * L);
    Ref hyper = ws((size_t)N * Mt * C8 * 4);
    {
        const Ref w0 = wt("mlps.w0"), b0 = wt("mlps.b0"), w1 = wt("mlps.w1"), b1 = wt("mlps.b1"), w2 = wt("mlps.w2"), b2 = wt("mlps.b2");
        live(queries, "token MLPs");
        op(OC_LINEAR, 2.0 * N * (Mt + 1) * (2.0 * C * C + (double)C8 * C), "hypernetwork MLPs + iou head", [=](const Run& r) {
            float* iou = r.cn_out ? (float*)r.cn_out[0] : nullptr;
            return mve_sam_token_mlps((const float*)r.p(queries), N, T, C, C, C8, Mt, (const float*)r.p(w0), (const float*)r.p(b0), (const float*)r.p(w1), (const float*)r.p(b1),
                                      (const float*)r.p(w2), (const float*)r.p(b2), (float*)r.p(hyper), iou, r.stream);
        });
    }
    tap(hyper, (size_t)N * Mt * C8 * 4, 3 + 2 * L);
    {
        const Ref out = arg(Ref::OUT);
        live(up, "mask product");
        op(OC_LINEAR, 2.0 * N * Mt * (double)P2 * C8, "masks = hyper_in . upscaled", [=](const Run& r) {
            return mve_sam_mask_product((const float*)r.p(hyper), (const float*)r.p(up), (float*)r.p(out), N, Mt, C8, P2, r.stream);
        });
    }
    tap(dense_pe, (size_t)G2 * C * 4, n_taps - 1);
    rel(hyper); rel(up); rel(queries);
    if (L > 0) rel(tokens);
    return finish("sam_decoder");
}

}  // namespace
