// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): CLIP text tower plan.
#pragma once
#include "executor_builder.h"

namespace {

// Output slots of a text-tower forward (Run::cn_out): fixed three, then the layers + 1 hidden states (null pointers: not requested)
enum { CLIP_OUT_LAST = 0, CLIP_OUT_POOLED = 1, CLIP_OUT_EMBEDS = 2, CLIP_OUT_HIDDEN0 = 3 };

// CLIPTextModel.forward / CLIPTextModelWithProjection.forward (transformers models/clip/modeling_clip.py:513-586, :856-895): embeddings,
// CLIPEncoderLayer x layers (:362-383: pre-norm attention and MLP, each with its residual), final_layer_norm, the end-of-text gather, and
// text_projection.  ids arrive as Run::sample (int32 [B, L]).  GEMMs never split K (rows_img = 0): one accumulation chain per element at
// every batch, so an item's result does not depend on its neighbours.
int Builder::build_clip(int B_, int L) {
    B = B_; dt = c.dtype;
    pl = Plan();
    pl.B = B_; pl.H = L; pl.W = 1; pl.n_img = 1; pl.io_dtype = c.dtype;
    const int e = 2, d = dt, Bn = B_, C = c.ch[0], heads = c.heads[0], I = c.clip_inter, P = c.clip_proj, act = c.clip_act;
    const int vocab = c.clip_vocab, max_pos = c.clip_max_pos;
    const float eps = c.eps, scale = 0.125f;      // head_dim 64
    MVE_CHECK(L >= 1 && L <= max_pos, MVE_ERR_ARG, "clip_text: L %d must be in [1, max_position_embeddings = %d]", L, max_pos);
    MVE_CHECK(L <= 128, MVE_ERR_ARG, "clip_text: L %d exceeds the 128 positions of mve_attention_causal", L);
    MVE_CHECK((size_t)Bn * L * (size_t)(I > 3 * C ? I : 3 * C) < ((size_t)1 << 31), MVE_ERR_ARG, "clip_text: batch %d overflows 32-bit activation indexing", Bn);
    const int M = Bn * L;
    ld_temb = 0; ld_kv = 0;
    rows_img = 0;
    Ref ids; ids.kind = Ref::SAMPLE;
    auto out_ref = [](int idx) { Ref r; r.kind = Ref::CNOUT; r.idx = idx; return r; };
    auto layernorm = [&](Ref x, Ref y, int rows, const std::string& n) {
        const Ref g = wt(n + ".g"), b = wt(n + ".b");
        live(x, "layernorm"); live(y, "layernorm");
        op(OC_NORM, 0, "layernorm", [=](const Run& r) { return mve_layernorm(d, r.p(x), C, r.p(y), C, rows, C, (const float*)r.p(g), (const float*)r.p(b), eps, r.stream); });
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
    const std::string em = "text_model.embeddings.";
    Ref x = ws((size_t)M * C * e);
    {
        const Ref tok = wt(em + "token_embedding.w"), pos = wt(em + "position_embedding.w");
        op(OC_OTHER, 0, "token + position embedding", [=](const Run& r) {
            return mve_clip_embed(d, (const int32_t*)r.p(ids), r.p(tok), r.p(pos), r.p(x), Bn, L, C, vocab, max_pos, r.stream);
        });
    }
    hidden_state(x, 0);
    for (int k = 0; k < c.layers_per_block; ++k) {
        const std::string b = "text_model.encoder.layers." + std::to_string(k);
        Ref n1 = ws((size_t)M * C * e);
        layernorm(x, n1, M, b + ".layer_norm1");
        Ref qkv = ws((size_t)M * 3 * C * e);
        gemm(n1, C, wt(b + ".self_attn.qkv.w"), C, qkv, 3 * C, M, 3 * C, C, wt(b + ".self_attn.qkv.b"), Ref(), 0, 0, Ref(), 0, 0, "self_attn.qkv");
        rel(n1);
        Ref a = ws((size_t)M * C * e);
        {
            const Ref q = qkv, kk = at(qkv, (size_t)C * e), v = at(qkv, (size_t)2 * C * e);
            live(qkv, "causal attention"); live(a, "causal attention");
            op(OC_ATTN, 4.0 * Bn * heads * (double)L * L * 64, "causal attention", [=](const Run& r) {
                return mve_attention_causal(d, r.p(q), 3 * C, r.p(kk), 3 * C, r.p(v), 3 * C, r.p(a), C, Bn, L, heads, 64, scale, r.stream);
            });
        }
        rel(qkv);
        Ref x2 = ws((size_t)M * C * e);
        gemm(a, C, wt(b + ".self_attn.out_proj.w"), C, x2, C, M, C, C, wt(b + ".self_attn.out_proj.b"), Ref(), 0, 0, x, C, 0, "self_attn.out_proj+residual");
        rel(a); rel(x); x = x2;
        Ref n2 = ws((size_t)M * C * e);
        layernorm(x, n2, M, b + ".layer_norm2");
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
    layernorm(x, last, M, "text_model.final_layer_norm");
    rel(x);
    op(OC_OTHER, 0, "end-of-text pooling", [=](const Run& r) { return mve_clip_pool(d, r.p(last), (const int32_t*)r.p(ids), r.p(pooled), Bn, L, C, r.clip_eos, r.stream); });
    if (P) gemm(pooled, C, wt("text_projection.w"), C, out_ref(CLIP_OUT_EMBEDS), P, Bn, P, C, Ref(), Ref(), 0, 0, Ref(), 0, 0, "text_projection");
    pl.enc_end = pl.ops.size();
    pl.ws_bytes = ar.peak + 256;
    if (!u.err.empty()) { mve_set_error("clip_text plan: %s", u.err.c_str()); u.err.clear(); return MVE_ERR_STATE; }
    return MVE_OK;
}

}  // namespace
