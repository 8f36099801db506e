// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): CLIP text tower plan.
#pragma once
#include "executor_builder.h"

namespace {

// Output slots of a text-tower forward (Run::cn_out): fixed three, then the layers + 1 hidden states (null pointers: not requested)
enum { CLIP_OUT_LAST = 0, CLIP_OUT_POOLED = 1, CLIP_OUT_EMBEDS = 2, CLIP_OUT_HIDDEN0 = 3 };

// parameter names and labels of Builder::encoder_layer in the transformers CLIPEncoderLayer scheme (text and vision tower)
constexpr Builder::EncoderNames CLIP_ENCODER = {".layer_norm1", ".self_attn.qkv", ".self_attn.out_proj", ".layer_norm2", ".mlp.fc1", ".mlp.fc2", "self_attn.qkv",
                                                "self_attn.out_proj+residual"};

// CLIPTextModel.forward / CLIPTextModelWithProjection.forward (transformers models/clip/modeling_clip.py:513-586, :856-895): embeddings,
// CLIPEncoderLayer x layers (:362-383: pre-norm attention and MLP, each with its residual), final_layer_norm, the end-of-text gather, and
// text_projection.  ids arrive as Run::sample (int32 [B, L]).  GEMMs never split K (rows_img = 0): one accumulation chain per element at
// every batch, so an item's result does not depend on its neighbours.
int Builder::build_clip(int B_, int L) {
    begin(B_, L, 1, 1, c.dtype);
    const int e = 2, d = dt, Bn = B_, C = c.ch[0], I = c.clip_inter, P = c.clip_proj;
    const int vocab = c.clip_vocab, max_pos = c.clip_max_pos;
    MVE_CHECK(L >= 1 && L <= max_pos, MVE_ERR_ARG, "clip_text: L %d must be in [1, max_position_embeddings = %d]", L, max_pos);
    MVE_CHECK(L <= 128, MVE_ERR_ARG, "clip_text: L %d exceeds the 128 positions of mve_attention_causal", L);
    MVE_CHECK((size_t)Bn * L * (size_t)(I > 3 * C ? I : 3 * C) < ((size_t)1 << 31), MVE_ERR_ARG, "clip_text: batch %d overflows 32-bit activation indexing", Bn);
    const int M = Bn * L;
    const size_t bytes = (size_t)M * C * e;
    const Ref ids = arg(Ref::SAMPLE);
    const std::string em = "text_model.embeddings.";
    Ref x = ws(bytes);
    {
        const Ref tok = wt(em + "token_embedding.w"), pos = wt(em + "position_embedding.w");
        op(OC_OTHER, 0, "token + position embedding", [=](const Run& r) {
            return mve_clip_embed(d, (const int32_t*)r.p(ids), r.p(tok), r.p(pos), r.p(x), Bn, L, C, vocab, max_pos, r.stream);
        });
    }
    copy_out(x, bytes, CLIP_OUT_HIDDEN0, "hidden state -> output");      // output_hidden_states
    for (int k = 0; k < c.layers_per_block; ++k) {
        x = encoder_layer(CLIP_ENCODER, "text_model.encoder.layers." + std::to_string(k), x, M, C, I, c.clip_act, true);
        copy_out(x, bytes, CLIP_OUT_HIDDEN0 + k + 1, "hidden state -> output");
    }
    const Ref last = cn_out(CLIP_OUT_LAST), pooled = cn_out(CLIP_OUT_POOLED);
    layernorm(x, C, last, M, C, "text_model.final_layer_norm", c.eps);
    rel(x);
    op(OC_OTHER, 0, "end-of-text pooling", [=](const Run& r) { return mve_clip_pool(d, r.p(last), (const int32_t*)r.p(ids), r.p(pooled), Bn, L, C, r.clip_eos, r.stream); });
    if (P) dense(pooled, wt("text_projection.w"), Ref(), cn_out(CLIP_OUT_EMBEDS), Bn, P, C, Ref(), "text_projection");
    return finish("clip_text");
}

}  // namespace
