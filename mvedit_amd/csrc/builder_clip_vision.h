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
    B = B_; dt = c.dtype;
    pl = Plan();
    const int S = c.cv_image, Pz = c.cv_patch, G = S / Pz, G2 = G * G, T = G2 + 1, Kp = (3 * Pz * Pz + 7) / 8 * 8;
    pl.B = B_; pl.H = T; pl.W = 1; pl.n_img = 1; pl.io_dtype = c.dtype;
    const int e = 2, d = dt, Bn = B_, C = c.ch[0], heads = c.heads[0], hd = C / heads, I = c.clip_inter, P = c.clip_proj, act = c.clip_act;
    const float eps = c.eps, scale = 1.0f / sqrtf((float)hd);
    const size_t widest = (size_t)(I > 3 * C ? I : 3 * C) > (size_t)Kp ? (size_t)(I > 3 * C ? I : 3 * C) : (size_t)Kp;
    MVE_CHECK((size_t)Bn * T * widest < ((size_t)1 << 31) && (size_t)Bn * 3 * S * S < ((size_t)1 << 31), MVE_ERR_ARG,
              "clip_vision: batch %d overflows 32-bit activation indexing", Bn);
    const int M = Bn * T, Mp = Bn * G2;
    ld_temb = 0; ld_kv = 0;
    rows_img = 0;
    Ref px; px.kind = Ref::SAMPLE;
    auto out_ref = [](int idx) { Ref r; r.kind = Ref::CNOUT; r.idx = idx; return r; };
    auto layernorm = [&](Ref x, int ldx, Ref y, int rows, const std::string& n) {
        const Ref g = wt(n + ".g"), b = wt(n + ".b");
        live(x, "layernorm"); live(y, "layernorm");
        op(OC_NORM, 0, "layernorm", [=](const Run& r) { return mve_layernorm(d, r.p(x), ldx, r.p(y), C, rows, C, (const float*)r.p(g), (const float*)r.p(b), eps, r.stream); });
    };
    auto hidden_state = [&](Ref x, int k) {       // output_hidden_states: copied out only when the caller gave a tensor for it
        const size_t bytes = (size_t)M * C * e;
        live(x, "hidden state -> output");
        op(OC_OTHER, 0, "hidden state -> output", [=](const Run& r) {
            void* dst = r.cn_out[CLIP_OUT_HIDDEN0 + k];
            if (!dst) return (int)MVE_OK;
            return hipMemcpyAsync(dst, r.p(x), bytes, hipMemcpyDeviceToDevice, r.stream) == hipSuccess ? (int)MVE_OK : (int)MVE_ERR_HIP;
        });
    };
    const std::string em = "vision_model.embeddings.";
    Ref x = ws((size_t)M * C * e);
    {
        Ref rows = ws((size_t)Mp * Kp * e);
        op(OC_OTHER, 0, "patchify", [=](const Run& r) { return mve_clip_patchify(d, r.p(px), Bn, S, S, Pz, r.p(rows), Kp, r.stream); });
        Ref patch = ws((size_t)Mp * C * e);
        gemm(rows, Kp, wt(em + "patch_embedding.w"), Kp, patch, C, Mp, C, Kp, Ref(), Ref(), 0, 0, Ref(), 0, 0, "patch_embedding");
        rel(rows);
        Ref x0 = ws((size_t)M * C * e);
        const Ref cls = wt(em + "class_embedding"), pos = wt(em + "position_embedding.w");
        live(patch, "class + position embedding"); live(x0, "class + position embedding");
        op(OC_OTHER, 0, "class + position embedding", [=](const Run& r) { return mve_clip_vision_embed(d, r.p(patch), r.p(cls), r.p(pos), r.p(x0), Bn, G2, C, r.stream); });
        rel(patch);
        layernorm(x0, C, x, M, "vision_model.pre_layrnorm");
        rel(x0);
    }
    hidden_state(x, 0);
    for (int k = 0; k < c.layers_per_block; ++k) {
        const std::string b = "vision_model.encoder.layers." + std::to_string(k);
        Ref n1 = ws((size_t)M * C * e);
        layernorm(x, C, n1, M, b + ".layer_norm1");
        Ref qkv = ws((size_t)M * 3 * C * e);
        gemm(n1, C, wt(b + ".self_attn.qkv.w"), C, qkv, 3 * C, M, 3 * C, C, wt(b + ".self_attn.qkv.b"), Ref(), 0, 0, Ref(), 0, 0, "self_attn.qkv");
        rel(n1);
        Ref a = ws((size_t)M * C * e);
        {
            const Ref q = qkv, kk = at(qkv, (size_t)C * e), v = at(qkv, (size_t)2 * C * e);
            live(qkv, "attention"); live(a, "attention");
            op(OC_ATTN, 4.0 * Bn * heads * (double)T * T * hd, "attention", [=](const Run& r) {
                return mve_attention(d, r.p(q), 3 * C, r.p(kk), 3 * C, r.p(v), 3 * C, nullptr, 0, nullptr, 0, r.p(a), C, Bn, T, T, 0, heads, hd, scale, r.stream);
            });
        }
        rel(qkv);
        Ref x2 = ws((size_t)M * C * e);
        gemm(a, C, wt(b + ".self_attn.out_proj.w"), C, x2, C, M, C, C, wt(b + ".self_attn.out_proj.b"), Ref(), 0, 0, x, C, 0, "self_attn.out_proj+residual");
        rel(a); rel(x); x = x2;
        Ref n2 = ws((size_t)M * C * e);
        layernorm(x, C, n2, M, b + ".layer_norm2");
        Ref f = ws((size_t)M * I * e);
        gemm(n2, C, wt(b + ".mlp.fc1.w"), C, f, I, M, I, C, wt(b + ".mlp.fc1.b"), Ref(), 0, 0, Ref(), 0, 0, "mlp.fc1");
        rel(n2);
        {
            const size_t nel = (size_t)M * I;
            live(f, "activation");
            op(OC_OTHER, 0, act == MVE_ACT_GELU ? "gelu" : "quick_gelu", [=](const Run& r) { return mve_act(d, act, r.p(f), r.p(f), nel, r.stream); });
        }
        Ref x3 = ws((size_t)M * C * e);
        gemm(f, I, wt(b + ".mlp.fc2.w"), I, x3, C, M, C, I, wt(b + ".mlp.fc2.b"), Ref(), 0, 0, x, C, 0, "mlp.fc2+residual");
        rel(f); rel(x); x = x3;
        hidden_state(x, k + 1);
    }
    const Ref last = out_ref(CLIP_OUT_LAST), pooled = out_ref(CLIP_OUT_POOLED);
    {
        const size_t bytes = (size_t)M * C * e;
        live(x, "last_hidden_state -> output");
        op(OC_OTHER, 0, "last_hidden_state -> output", [=](const Run& r) {
            return hipMemcpyAsync(r.p(last), r.p(x), bytes, hipMemcpyDeviceToDevice, r.stream) == hipSuccess ? (int)MVE_OK : (int)MVE_ERR_HIP;
        });
    }
    layernorm(x, T * C, pooled, Bn, "vision_model.post_layernorm");      // the class rows: row b at x + b * T * C
    rel(x);
    if (P) gemm(pooled, C, wt("visual_projection.w"), C, out_ref(CLIP_OUT_EMBEDS), P, Bn, P, C, Ref(), Ref(), 0, 0, Ref(), 0, 0, "visual_projection");
    pl.enc_end = pl.ops.size();
    pl.ws_bytes = ar.peak + 256;
    if (!u.err.empty()) { mve_set_error("clip_vision plan: %s", u.err.c_str()); u.err.clear(); return MVE_ERR_STATE; }
    return MVE_OK;
}

// Resampler.forward (lib/models/architecture/ip_adapter/resampler.py:109-120) with PerceiverAttention (:45-74) and FeedForward (:9-16).
// x [B, n1, embedding_dim] arrives as Run::sample, the tokens [B, num_queries, output_dim] leave through Run::out.  to_kv acts per row, so
// to_kv(cat(x, latents)) is two GEMMs whose outputs are the two KV segments of mve_attention -- the concatenation is never formed.
// One intended rounding difference: the reference multiplies q and k by dim_head^-1/4 each (two roundings) and rounds the softmax to 16 bit;
// here the logits are scaled by 1/8 in fp32 and the probabilities keep mve_attention's fp32 softmax.
int Builder::build_resampler(int B_, int n1) {
    B = B_; dt = c.dtype;
    pl = Plan();
    pl.B = B_; pl.H = n1; pl.W = 1; pl.n_img = 1; pl.io_dtype = c.dtype;
    const int e = 2, d = dt, Bn = B_, D = c.ch[0], heads = c.heads[0], inner = heads * 64, F = c.rs_inner, E = c.rs_embed, O = c.rs_out, Q = c.rs_queries;
    const float eps = 1e-5f;      // nn.LayerNorm default
    const size_t widest = (size_t)(2 * inner > F ? 2 * inner : F) > (size_t)E ? (size_t)(2 * inner > F ? 2 * inner : F) : (size_t)E;
    MVE_CHECK((size_t)Bn * (n1 > Q ? n1 : Q) * widest < ((size_t)1 << 31), MVE_ERR_ARG, "ip_resampler: batch %d overflows 32-bit activation indexing", Bn);
    const int Mx = Bn * n1, Ml = Bn * Q;
    ld_temb = 0; ld_kv = 0;
    rows_img = 0;
    Ref xin; xin.kind = Ref::SAMPLE;
    Ref out; out.kind = Ref::OUT;
    auto layernorm = [&](Ref x, Ref y, int rows, int C, const std::string& n) {
        const Ref g = wt(n + ".g"), b = wt(n + ".b");
        live(x, "layernorm"); live(y, "layernorm");
        op(OC_NORM, 0, "layernorm", [=](const Run& r) { return mve_layernorm(d, r.p(x), C, r.p(y), C, rows, C, (const float*)r.p(g), (const float*)r.p(b), eps, r.stream); });
    };
    Ref x = ws((size_t)Mx * D * e);
    gemm(xin, E, wt("proj_in.w"), E, x, D, Mx, D, E, wt("proj_in.b"), Ref(), 0, 0, Ref(), 0, 0, "proj_in");
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
        layernorm(x, nx, Mx, D, a + ".norm1");
        layernorm(lat, nl, Ml, D, a + ".norm2");
        Ref q = ws((size_t)Ml * inner * e), kvx = ws((size_t)Mx * 2 * inner * e), kvl = ws((size_t)Ml * 2 * inner * e);
        gemm(nl, D, wt(a + ".to_q.w"), D, q, inner, Ml, inner, D, Ref(), Ref(), 0, 0, Ref(), 0, 0, "to_q");
        gemm(nx, D, wt(a + ".to_kv.w"), D, kvx, 2 * inner, Mx, 2 * inner, D, Ref(), Ref(), 0, 0, Ref(), 0, 0, "to_kv (image rows)");
        gemm(nl, D, wt(a + ".to_kv.w"), D, kvl, 2 * inner, Ml, 2 * inner, D, Ref(), Ref(), 0, 0, Ref(), 0, 0, "to_kv (latent rows)");
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
        gemm(o, inner, wt(a + ".to_out.w"), inner, lat2, D, Ml, D, inner, Ref(), Ref(), 0, 0, lat, D, 0, "to_out+residual");
        rel(o); rel(lat); lat = lat2;
        Ref n = ws((size_t)Ml * D * e);
        layernorm(lat, n, Ml, D, f + ".0");
        Ref h = ws((size_t)Ml * F * e);
        gemm(n, D, wt(f + ".1.w"), D, h, F, Ml, F, D, Ref(), Ref(), 0, 0, Ref(), 0, 0, "ff.1");
        rel(n);
        {
            const size_t nel = (size_t)Ml * F;
            live(h, "gelu");
            op(OC_OTHER, 0, "gelu", [=](const Run& r) { return mve_act(d, MVE_ACT_GELU, r.p(h), r.p(h), nel, r.stream); });
        }
        Ref lat3 = ws((size_t)Ml * D * e);
        gemm(h, F, wt(f + ".3.w"), F, lat3, D, Ml, D, F, Ref(), Ref(), 0, 0, lat, D, 0, "ff.3+residual");
        rel(h); rel(lat); lat = lat3;
    }
    rel(x);
    Ref po = ws((size_t)Ml * O * e);
    gemm(lat, D, wt("proj_out.w"), D, po, O, Ml, O, D, wt("proj_out.b"), Ref(), 0, 0, Ref(), 0, 0, "proj_out");
    rel(lat);
    layernorm(po, out, Ml, O, "norm_out");
    rel(po);
    pl.enc_end = pl.ops.size();
    pl.ws_bytes = ar.peak + 256;
    if (!u.err.empty()) { mve_set_error("ip_resampler plan: %s", u.err.c_str()); u.err.clear(); return MVE_ERR_STATE; }
    return MVE_OK;
}

}  // namespace
