// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): CLIP vision tower plan and the
// IP-Adapter Resampler plan.
#pragma once
#include "executor_builder.h"
#include "builder_clip.h"

namespace {

// CLIPVisionModel.forward / CLIPVisionModelWithProjection.forward (transformers models/clip/modeling_clip.py: CLIPVisionEmbeddings, pre_layrnorm,
// CLIPEncoderLayer x layers, post_layernorm over the class row, visual_projection).  Pixels arrive as Run::sample ([B,3,S,S] NCHW, engine
// dtype); the outputs use the text tower's slots (CLIP_OUT_*): last_hidden_state is the encoder output WITHOUT post_layernorm, pooler_output
// is post_layernorm(last_hidden_state[:, 0]), hidden state 0 is the pre_layrnorm output.  GEMMs never split K (rows_img = 0): one accumulation
// chain per element at every batch, and mve_attention works per (item, head, query tile), so an item's result does not depend on its neighbours.
int Builder::build_clip_vision(int B_) {
    const int S = c.cv_image, Pz = c.cv_patch, G = S / Pz, G2 = G * G, T = G2 + 1, Kp = (3 * Pz * Pz + 7) / 8 * 8;
    begin(B_, T, 1, 1, c.dtype);
    const int e = 2, d = dt, Bn = B_, C = c.ch[0], I = c.clip_inter, P = c.clip_proj;
    const float eps = c.eps;
    const size_t widest = (size_t)(I > 3 * C ? I : 3 * C) > (size_t)Kp ? (size_t)(I > 3 * C ? I : 3 * C) : (size_t)Kp;
    MVE_CHECK((size_t)Bn * T * widest < ((size_t)1 << 31) && (size_t)Bn * 3 * S * S < ((size_t)1 << 31), MVE_ERR_ARG,
              "clip_vision: batch %d overflows 32-bit activation indexing", Bn);
    const int M = Bn * T, Mp = Bn * G2;
    const size_t bytes = (size_t)M * C * e;
    const Ref px = arg(Ref::SAMPLE);
    const std::string em = "vision_model.embeddings.";
    Ref x = ws(bytes);
    {
        Ref rows = ws((size_t)Mp * Kp * e);
        op(OC_OTHER, 0, "patchify", [=](const Run& r) { return mve_clip_patchify(d, r.p(px), Bn, S, S, Pz, r.p(rows), Kp, r.stream); });
        Ref patch = ws((size_t)Mp * C * e);
        dense(rows, wt(em + "patch_embedding.w"), Ref(), patch, Mp, C, Kp, Ref(), "patch_embedding");
        rel(rows);
        Ref x0 = ws(bytes);
        const Ref cls = wt(em + "class_embedding"), pos = wt(em + "position_embedding.w");
        live(patch, "class + position embedding"); live(x0, "class + position embedding");
        op(OC_OTHER, 0, "class + position embedding", [=](const Run& r) { return mve_clip_vision_embed(d, r.p(patch), r.p(cls), r.p(pos), r.p(x0), Bn, G2, C, r.stream); });
        rel(patch);
        layernorm(x0, C, x, M, C, "vision_model.pre_layrnorm", eps);
        rel(x0);
    }
    copy_out(x, bytes, CLIP_OUT_HIDDEN0, "hidden state -> output");      // output_hidden_states
    for (int k = 0; k < c.layers_per_block; ++k) {
        x = encoder_layer(CLIP_ENCODER, "vision_model.encoder.layers." + std::to_string(k), x, M, C, I, c.clip_act, false);
        copy_out(x, bytes, CLIP_OUT_HIDDEN0 + k + 1, "hidden state -> output");
    }
    const Ref last = cn_out(CLIP_OUT_LAST), pooled = cn_out(CLIP_OUT_POOLED);
    live(x, "last_hidden_state -> output");
    op(OC_OTHER, 0, "last_hidden_state -> output", [=](const Run& r) {
        return hipMemcpyAsync(r.p(last), r.p(x), bytes, hipMemcpyDeviceToDevice, r.stream) == hipSuccess ? (int)MVE_OK : (int)MVE_ERR_HIP;
    });
    layernorm(x, T * C, pooled, Bn, C, "vision_model.post_layernorm", eps);      // the class rows: row b at x + b * T * C
    rel(x);
    if (P) dense(pooled, wt("visual_projection.w"), Ref(), cn_out(CLIP_OUT_EMBEDS), Bn, P, C, Ref(), "visual_projection");
    return finish("clip_vision");
}

// Resampler.forward (lib/models/architecture/ip_adapter/resampler.py:109-120) with PerceiverAttention (:45-74) and FeedForward (:9-16).
// x [B, n1, embedding_dim] arrives as Run::sample, the tokens [B, num_queries, output_dim] leave through Run::out.  to_kv acts per row, so
// to_kv(cat(x, latents)) is two GEMMs whose outputs are the two KV segments of mve_attention -- the concatenation is never formed.
// One intended rounding difference: the reference multiplies q and k by dim_head^-1/4 each (two roundings) and rounds the softmax to 16 bit;
// here the logits are scaled by 1/8 in fp32 and the probabilities keep mve_attention's fp32 softmax.
int Builder::build_resampler(int B_, int n1) {
    begin(B_, n1, 1, 1, c.dtype);
    const int e = 2, d = dt, Bn = B_, D = c.ch[0], heads = c.heads[0], inner = heads * 64, F = c.rs_inner, E = c.rs_embed, O = c.rs_out, Q = c.rs_queries;
    const float eps = 1e-5f;      // nn.LayerNorm default
    const size_t widest = (size_t)(2 * inner > F ? 2 * inner : F) > (size_t)E ? (size_t)(2 * inner > F ? 2 * inner : F) : (size_t)E;
    MVE_CHECK((size_t)Bn * (n1 > Q ? n1 : Q) * widest < ((size_t)1 << 31), MVE_ERR_ARG, "ip_resampler: batch %d overflows 32-bit activation indexing", Bn);
    const int Mx = Bn * n1, Ml = Bn * Q;
    Ref x = ws((size_t)Mx * D * e);
    dense(arg(Ref::SAMPLE), wt("proj_in.w"), wt("proj_in.b"), x, Mx, D, E, Ref(), "proj_in");
    Ref lat = ws((size_t)Ml * D * e);
    {
        const Ref src = wt("latents");
        const size_t bytes = (size_t)Q * D * e;
        live(lat, "latents.repeat");
        op(OC_OTHER, 0, "latents.repeat", [=](const Run& r) {
            for (int b = 0; b < Bn; ++b)
                if (hipMemcpyAsync((unsigned char*)r.p(lat) + (size_t)b * bytes, r.p(src), bytes, hipMemcpyDeviceToDevice, r.stream) != hipSuccess) return (int)MVE_ERR_HIP;
            return (int)MVE_OK;
        });
    }
    for (int k = 0; k < c.layers_per_block; ++k) {
        const std::string a = "layers." + std::to_string(k) + ".0", f = "layers." + std::to_string(k) + ".1";
        Ref nx = ws((size_t)Mx * D * e), nl = ws((size_t)Ml * D * e);
        layernorm(x, D, nx, Mx, D, a + ".norm1", eps);
        layernorm(lat, D, nl, Ml, D, a + ".norm2", eps);
        Ref q = ws((size_t)Ml * inner * e), kvx = ws((size_t)Mx * 2 * inner * e), kvl = ws((size_t)Ml * 2 * inner * e);
        dense(nl, wt(a + ".to_q.w"), Ref(), q, Ml, inner, D, Ref(), "to_q");
        dense(nx, wt(a + ".to_kv.w"), Ref(), kvx, Mx, 2 * inner, D, Ref(), "to_kv (image rows)");
        dense(nl, wt(a + ".to_kv.w"), Ref(), kvl, Ml, 2 * inner, D, Ref(), "to_kv (latent rows)");
        rel(nx); rel(nl);
        Ref o = ws((size_t)Ml * inner * e);
        {
            const Ref vx = at(kvx, (size_t)inner * e), vl = at(kvl, (size_t)inner * e);
            live(q, "perceiver attention"); live(kvx, "perceiver attention"); live(kvl, "perceiver attention"); live(o, "perceiver attention");
            op(OC_ATTN, 4.0 * Bn * heads * (double)Q * (n1 + Q) * 64, "perceiver attention", [=](const Run& r) {
                return mve_attention(d, r.p(q), inner, r.p(kvx), 2 * inner, r.p(vx), 2 * inner, r.p(kvl), 2 * inner, r.p(vl), 2 * inner, r.p(o), inner, Bn, Q, n1, Q,
                                     heads, 64, 0.125f, r.stream);
            });
        }
        rel(q); rel(kvx); rel(kvl);
        Ref lat2 = ws((size_t)Ml * D * e);
        dense(o, wt(a + ".to_out.w"), Ref(), lat2, Ml, D, inner, lat, "to_out+residual");
        rel(o); rel(lat); lat = lat2;
        Ref n = ws((size_t)Ml * D * e);
        layernorm(lat, D, n, Ml, D, f + ".0", eps);
        Ref h = ws((size_t)Ml * F * e);
        dense(n, wt(f + ".1.w"), Ref(), h, Ml, F, D, Ref(), "ff.1");
        rel(n);
        act(h, (size_t)Ml * F, MVE_ACT_GELU, "gelu");
        Ref lat3 = ws((size_t)Ml * D * e);
        dense(h, wt(f + ".3.w"), Ref(), lat3, Ml, D, F, lat, "ff.3+residual");
        rel(h); rel(lat); lat = lat3;
    }
    rel(x);
    Ref po = ws((size_t)Ml * O * e);
    dense(lat, wt("proj_out.w"), wt("proj_out.b"), po, Ml, O, D, Ref(), "proj_out");
    rel(lat);
    layernorm(po, O, arg(Ref::OUT), Ml, O, "norm_out", eps);
    rel(po);
    return finish("ip_resampler");
}

}  // namespace
