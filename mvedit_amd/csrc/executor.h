// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): primitive declarations, weight packing kernel, configuration, parameter table, plan / op / arena types, block enumeration.
#pragma once
#include "common.h"

#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

extern "C" {
int mve_gemm(int, const void*, int, const void*, int, void*, int, int, int, int, const float*, const float*, int, int,
             const void*, int, int, float, void*, size_t, int, void*);
int mve_gemm_pair(int, const void*, int, const void*, int, void*, int, int, int, int, const float*, const float*, int, int,
                  const void*, int, int, float, void*, size_t, int, const void*, void*, void*);
int mve_gemm_pair_ln(int, const void*, int, const void*, int, void*, int, int, int, int, const float*, const void*, int, void*, size_t, int,
                     const void*, void*, void*, int, const float*, const float*, float, void*);
int mve_conv3x3_pair(int, const void*, int, const void*, int, int, int, int, int, int, const void*, int, void*, int,
                     const float*, const float*, int, const void*, int, int, float, void*, size_t, const void*, void*, void*);
int mve_conv3x3_shortcut_pair(int, const void*, int, const void*, int, const void*, int, int, int, int, const void*, int, void*, int,
                              const float*, const float*, int, float, void*, size_t, void*, void*);
int mve_groupnorm_silu_pair(int, const void*, int, const void*, int, int, int, int, float, const float*, const float*, int, void*,
                            void*, const void*, const void*, void*);
int mve_layernorm_pair(int, const void*, int, void*, int, int, int, const float*, const float*, float, const void*, void*);
int mve_axpy_pair(int, const void*, const void*, const void*, float, void*, void*, size_t, void*);
int mve_conv3x3(int, const void*, int, const void*, int, int, int, int, int, int, const void*, int, void*, int,
                const float*, const float*, int, const void*, int, int, float, void*, size_t, void*);
size_t mve_gemm_workspace_bytes(int, int, int, int);
int mve_upsample_conv_phases_supported(int, int, int, int, int);
size_t mve_upsample_conv_phases_workspace_bytes(int, int, int, int, int);
int mve_pack_upsample_phase_weights(int, int, const void*, int, int, void*, void*);
int mve_upsample_conv_phases(int, const void*, int, int, int, int, const void*, int, void*, const float*, int, void*, size_t, void*, void*);
int mve_attention_prescaled(int, const void*, int, const void*, int, const void*, int, const void*, int, const void*, int, void*, int, int, int, int, int, int, int, void*);
int mve_attention(int, const void*, int, const void*, int, const void*, int, const void*, int, const void*, int, void*, int,
                  int, int, int, int, int, int, float, void*);
size_t mve_groupnorm_workspace_bytes(int, int, int, int);
int mve_groupnorm_silu(int, const void*, int, const void*, int, int, int, int, float, const float*, const float*, int, void*,
                       void*, void*);
int mve_layernorm(int, const void*, int, void*, int, int, int, const float*, const float*, float, void*);
int mve_nchw_to_nhwc(int, int, const void*, int, int, int, int, int, void*, void*);
int mve_nhwc_to_nchw(int, int, const void*, int, int, int, int, int, void*, void*);
int mve_timestep_embedding(int, const float*, int, int, void*, void*);
int mve_text_time_embedding(int, const void*, int, int, const float*, int, int, int, void*, void*);
int mve_silu(int, const void*, void*, size_t, void*);
int mve_axpy(int, const void*, const void*, float, void*, size_t, void*);
int mve_softmax_rows(int, const float*, size_t, int, int, void*, size_t, void*);
int mve_prelu(int, const void*, const float*, int, void*, size_t, void*);
int mve_pixel_shuffle_add(int, const float*, int, const void*, int, int, int, int, int, void*, void*);
int mve_lpips_scale(int, int, const void*, const void*, int, int, int, const float*, const float*, int, void*, void*);
int mve_lpips_input_grad(int, int, const void*, int, int, int, const float*, int, void*, void*);
int mve_maxpool2x2(int, const void*, int, int, int, int, void*, void*);
int mve_maxpool2x2_backward(int, const void*, const void*, int, int, int, int, void*, void*);
int mve_relu_backward(int, void*, const void*, size_t, void*);
size_t mve_lpips_layer_scratch_bytes(int, int);
int mve_lpips_layer(int, const void*, const float*, int, int, int, int, float*, void*, void*);
int mve_lpips_layer_backward(int, const void*, const float*, const float*, int, int, int, void*, void*);
int mve_attention_causal(int, const void*, int, const void*, int, const void*, int, void*, int, int, int, int, int, float, void*);
int mve_clip_embed(int, const int32_t*, const void*, const void*, void*, int, int, int, int, int, void*);
int mve_act(int, int, const void*, void*, size_t, void*);
int mve_clip_pool(int, const void*, const int32_t*, void*, int, int, int, int, void*);
int mve_clip_patchify(int, const void*, int, int, int, int, void*, int, void*);
int mve_clip_vision_embed(int, const void*, const void*, const void*, void*, int, int, int, void*);
int mve_dpt_stem_rows(int, const void*, int, int, void*, int, void*);
int mve_dpt_maxpool(int, const void*, int, int, int, int, void*, void*);
int mve_dpt_gather_s2(int, const void*, int, int, int, int, void*, void*);
int mve_dpt_upsample2x(int, const void*, int, int, int, int, void*, void*);
int mve_dpt_add_relu(int, const void*, const void*, void*, size_t, void*);
int mve_loftr_stem_rows(int, const void*, int, int, int, void*, int, void*);
int mve_loftr_leaky_relu(int, const void*, void*, size_t, float, void*);
int mve_loftr_pos_add(int, const void*, const float*, void*, int, int, int, void*);
size_t mve_linattn_workspace_bytes(int, int, int, int);
int mve_linattn_kv(int, const void*, int, const void*, int, int, int, int, int, float*, void*, size_t, void*);
int mve_linattn_apply(int, const void*, int, const float*, void*, int, int, int, int, int, float, void*);
int mve_dsmax_stats(const float*, int, int, int, int, float*, float*, void*);
int mve_dsmax_conf(const float*, int, int, int, int, const float*, const float*, float*, void*);
size_t mve_dsmax_select_workspace_bytes(int, int, int);
int mve_dsmax_select(const float*, int, int, int, int, int, float, int, float, int64_t*, int64_t*, int64_t*, float*, float*, float*, int*, void*, size_t, void*);
int mve_loftr_unfold(int, const void*, int, int, int, int, const int64_t*, const int64_t*, int, void*, void*);
int mve_loftr_ln_add(int, const void*, int, const void*, int, void*, int, int, int, const float*, const float*, float, void*);
int mve_loftr_gather_rows(int, const void*, int, int, int, const int64_t*, const int64_t*, int, void*, void*);
int mve_loftr_fine_match(int, const void*, const void*, int, int, const float*, float, float*, float*, void*);
int mve_attention_relpos(int, const void*, int, const void*, int, const void*, int, const void*, const void*, void*, int, int, int, int, int, int, float, void*);
int mve_sam_window_partition(int, const void*, int, int, int, int, void*, void*);
int mve_sam_window_unpartition(int, const void*, int, int, int, int, void*, void*);
int mve_sam_pos_add(int, const void*, const void*, void*, int, int, int, void*);
}

namespace {

constexpr int MAX_LEVELS = 8;

// ---------------------------------------------------------------------------------------------------
// weight packing kernel: dst[d0*t0 + d1*t1 + d2*t2 + d3*t3] = (d3 < valid3) ? src[d0*s0 + d1*s1 + d2*s2 + d3*s3] : 0
// ---------------------------------------------------------------------------------------------------
struct PackDims { long long D[4], s[4], t[4]; long long valid3; float mul = 1.0f; };   // mul: applied in fp32 before the single rounding

template <class Src, class Dst>
__global__ void k_pack(const Src* __restrict__ src, Dst* __restrict__ dst, PackDims p) {
    const long long n = p.D[0] * p.D[1] * p.D[2] * p.D[3];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const long long d3 = r % p.D[3]; r /= p.D[3];
        const long long d2 = r % p.D[2]; r /= p.D[2];
        const long long d1 = r % p.D[1]; r /= p.D[1];
        const long long d0 = r;
        float v = 0.f;
        if (d3 < p.valid3) v = (float)src[d0 * p.s[0] + d1 * p.s[1] + d2 * p.s[2] + d3 * p.s[3]] * p.mul;
        dst[d0 * p.t[0] + d1 * p.t[1] + d2 * p.t[2] + d3 * p.t[3]] = (Dst)v;
    }
}

template <class Src>
int pack_to(int dst_dtype, const void* src, void* dst, const PackDims& p, hipStream_t s) {
    const long long n = p.D[0] * p.D[1] * p.D[2] * p.D[3];
    if (n == 0) return MVE_OK;
    const unsigned grid = (unsigned)((n + 255) / 256 > 65535 ? 65535 : (n + 255) / 256);
    if (dst_dtype == MVE_F32) k_pack<Src, float><<<grid, 256, 0, s>>>((const Src*)src, (float*)dst, p);
    else if (dst_dtype == MVE_F16) k_pack<Src, f16><<<grid, 256, 0, s>>>((const Src*)src, (f16*)dst, p);
    else if (dst_dtype == MVE_BF16) k_pack<Src, bf16><<<grid, 256, 0, s>>>((const Src*)src, (bf16*)dst, p);
    else { mve_set_error("pack: bad dst dtype"); return MVE_ERR_ARG; }
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int pack(int src_dtype, int dst_dtype, const void* src, void* dst, const PackDims& p, hipStream_t s) {
    if (src_dtype == MVE_F32) return pack_to<float>(dst_dtype, src, dst, p, s);
    if (src_dtype == MVE_F16) return pack_to<f16>(dst_dtype, src, dst, p, s);
    if (src_dtype == MVE_BF16) return pack_to<bf16>(dst_dtype, src, dst, p, s);
    mve_set_error("pack: bad src dtype %d", src_dtype);
    return MVE_ERR_ARG;
}

// mean over groups of n consecutive images: x [B, R] -> y [B/n, R]  (joint_attn.py:24 encoder_hidden_states_.mean(dim=1))
template <class Tag>
__global__ void k_group_mean(const typename Tag::T* __restrict__ x, typename Tag::T* __restrict__ y, long long R, int n,
                             long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long g = i / R, r = i - g * R;
    float a = 0.f;
    for (int k = 0; k < n; ++k) a += Tag::to_f32(x[(g * n + k) * R + r]);
    y[i] = Tag::from_f32(a / (float)n);
}

// ---------------------------------------------------------------------------------------------------
// configuration / parameter table
// ---------------------------------------------------------------------------------------------------
constexpr int CN_EMB[4] = {16, 32, 96, 256};      // diffusers ControlNetModel conditioning_embedding_out_channels (default)

// which network a handle runs: one executor, one plan builder per kind (builder_*.h)
enum class Kind { UNet, ControlNet, VaeDecoder, VaeEncoder, Srvgg, Lpips, ClipText, ClipVision, Resampler, Dpt, Loftr, Sam, SamDecoder };

// the noun of "handle is ..., not ..." messages
const char* kind_name(Kind k) {
    switch (k) {
        case Kind::UNet: return "a UNet";
        case Kind::ControlNet: return "a ControlNet";
        case Kind::VaeDecoder: case Kind::VaeEncoder: return "a VAE half";
        case Kind::Srvgg: return "an SRVGGNetCompact";
        case Kind::Lpips: return "an LPIPS engine";
        case Kind::ClipText: return "a CLIP text tower";
        case Kind::ClipVision: return "a CLIP vision tower";
        case Kind::Resampler: return "a Resampler";
        case Kind::Dpt: return "a DPT model";
        case Kind::Loftr: return "a LoFTR model";
        case Kind::Sam: return "a SAM image encoder";
        case Kind::SamDecoder: return "a SAM mask decoder";
    }
    return "an unknown engine";
}

struct Config {
    Kind kind = Kind::UNet;
    bool is_denoiser() const { return kind == Kind::UNet || kind == Kind::ControlNet; }
    bool is_vae() const { return kind == Kind::VaeDecoder || kind == Kind::VaeEncoder; }
    int cond_ch = 3;                   // ControlNetModel: encoder + mid of the UNet, conditioning embedding, zero convolutions
    int lpips_normalize = 1;           // LPIPS(net='vgg') forward + backward w.r.t. the prediction (lib/models/losses/lpips_loss.py)
    int sr_scale = 4;                  // SRVGGNetCompact (lib/models/decoders/image_space_ss.py): ch[0] = num_feat, layers_per_block = num_conv
    // AutoencoderKL halves: VaeDecoder = post_quant_conv + Decoder, VaeEncoder = Encoder + quant_conv (no time embedding, no transformers;
    // in_ch / out_ch are the half's own input / output channels, both <= 8)
    // CLIPTextModel(WithProjection) (transformers models/clip/modeling_clip.py): ch[0] = hidden_size, heads[0] = num_attention_heads,
    // layers_per_block = num_hidden_layers, eps = layer_norm_eps; clip_proj = projection_dim (0: no text_projection)
    int clip_vocab = 0, clip_max_pos = 0, clip_inter = 0, clip_act = 0, clip_proj = 0;
    // CLIPVisionModel(WithProjection): ch[0] / heads[0] / layers_per_block / eps / clip_inter / clip_act / clip_proj as for the text tower;
    // cv_image = image_size, cv_patch = patch_size (builder_clip_vision.h)
    int cv_image = 0, cv_patch = 0;
    // IP-Adapter Resampler (lib/models/architecture/ip_adapter/resampler.py): ch[0] = dim, heads[0] = heads (dim_head 64), layers_per_block = depth,
    // rs_queries = num_queries, rs_embed = embedding_dim, rs_out = output_dim, rs_inner = int(dim * ff_mult)
    int rs_queries = 0, rs_embed = 0, rs_out = 0, rs_inner = 0;
    // DPT-hybrid (omnidata_modules/midas/dpt_depth.py DPTDepthModel over vit_base_resnet50_384; builder_dpt.h): ch[0] = ViT width, heads[0],
    // layers_per_block = ViT depth, eps = LayerNorm eps, groups = GroupNorm groups of the ResNetV2, out_ch = num_channels; dp_image = image size,
    // dp_stem = stem width, dp_stage / dp_depth = the three stages' widths / depths, dp_tap = the two tapped ViT blocks (hooks[2], hooks[3]),
    // dp_inter = MLP width, dp_neck = channels of act_postprocess3 / 4, dp_features = decoder width
    int dp_image = 0, dp_stem = 0, dp_stage[3] = {0, 0, 0}, dp_depth[3] = {0, 0, 0}, dp_tap[2] = {0, 0}, dp_inter = 0, dp_neck[2] = {0, 0}, dp_features = 0;
    // SAM image encoder (segment_anything ImageEncoderViT = transformers SamVisionEncoder; builder_sam.h): ch[0] = hidden_size, heads[0],
    // layers_per_block = num_hidden_layers, eps = layer_norm_eps, clip_inter = mlp_dim; sm_image = image_size, sm_patch = patch_size, sm_window =
    // window_size, sm_out = output_channels (the neck's width), sm_global = bit k set: block k attends over the whole grid (global_attn_indexes)
    int sm_image = 0, sm_patch = 0, sm_window = 0, sm_out = 0;
    unsigned long long sm_global = 0;
    // SAM prompt encoder + mask decoder (transformers SamPromptEncoder + SamMaskDecoder; builder_sam_decoder.h), fp32 throughout: ch[0] = hidden_size,
    // heads[0], layers_per_block = num_hidden_layers of the two-way transformer, clip_inter = mlp_dim, eps = the eps of layer_norm1..4, sd_eps_final =
    // that of layer_norm_final_attn; sd_grid = G (image_embedding_size), sd_image = the prompt encoder's input_image_size, sd_masks = num_mask_tokens;
    // dtype = the dtype of the image embedding it reads
    int sd_grid = 0, sd_image = 0, sd_masks = 0;
    float sd_eps_final = 1e-5f;
    // LoFTR matcher (loftr/loftr.py with default_cfg; builder_loftr.h): a fixed topology, nothing to configure but the dtype
    int dtype, in_ch, out_ch, n_levels, layers_per_block, ctx_dim, groups, linear_proj;
    // UNet2DConditionModel / ControlNetModel addition_embed_type (mve_unet_set_addition_embed): 0 none, 1 'text_time' (SDXL);
    // add_time_dim = addition_time_embed_dim, add_P = projection_class_embeddings_input_dim (in_features of add_embedding.linear_1)
    int add_type = 0, add_time_dim = 0, add_P = 0;
    float eps;
    int ch[MAX_LEVELS], attn[MAX_LEVELS], heads[MAX_LEVELS], tlayers[MAX_LEVELS];
    int temb_dim() const { return ch[0] * 4; }
};

struct Param {   // one engine-owned packed tensor (or a slice view of one)
    size_t off = 0;       // byte offset in the weight slab
    size_t bytes = 0;
    bool f32 = false;
    float q_fold = 0.f;   // > 0: a to_q weight whose rows carry head_dim^-1/2 * log2(e) (the attention kernel then takes Q as it comes)
};

// One accepted state-dict tensor, as the layout describes it while it reserves the slot (executor_params.h): load_param looks the name up, checks
// the tensor against `numel` / `conv`, and runs the steps.  Everything is resolved from Config at layout time.
struct PackStep {
    std::string slot;          // destination slot ...
    size_t off = 0;            // ... and the element offset inside it
    long long src_off = 0;     // element offset into the source tensor
    PackDims d{};
    bool phase4 = false;       // instead of `d`: the upsampler's summed taps (mve_pack_upsample_phase_weights over the source's [O, I, 3, 3])
};
struct Source {
    long long numel = 0;               // required element count (any shape: [C, C] and [C, C, 1, 1] both load)
    long long conv[2] = {0, 0};        // 3 x 3 convolutions: the exact shape [O, I, 3, 3] is required
    bool zero = false;                 // the steps' slots are cleared first (padding rows / columns the tensor does not cover)
    bool optional = false;             // not in `expected`: the IP-Adapter's to_k_ip / to_v_ip, counted in n_ip_loaded
    std::vector<PackStep> steps;       // one, or two for a weight that is kept in two packings (LPIPS `.wt`, the upsamplers' `.w4`)
};

enum OpClass { OC_CONV = 0, OC_LINEAR = 1, OC_ATTN = 2, OC_NORM = 3, OC_OTHER = 4, OC_COUNT = 5 };

struct Ref {
    enum Kind { NUL, WS, WT, SAMPLE, TIMESTEPS, CTX, OUT, DOWNRES, MIDRES, REFSTORE, CNCOND, CNOUT } kind = NUL;
    size_t off = 0;
    int idx = 0;
};

struct Run {
    unsigned char* ws = nullptr; unsigned char* wt = nullptr;
    const void* sample = nullptr; const float* timesteps = nullptr; const void* ctx = nullptr; void* out = nullptr;
    const void* const* down_res = nullptr; const void* mid_res = nullptr;
    unsigned char* ref_store = nullptr;
    const void* cn_cond = nullptr;            // ControlNet: conditioning image [B, cond_ch, 8H, 8W] NCHW (io dtype)
    void* const* cn_out = nullptr;            // ControlNet: n_skips + 1 output tensors (NHWC, engine dtype)
    float cn_scale = 1.0f;                    // conditioning_scale
    int cn_accum = 0;                         // 1: add to what the outputs already hold (MultiControlNetModel's sum)
    const void* add_text = nullptr;           // 'text_time': text_embeds [B, add_text_dim] (add_text_dtype), time_ids f32 [B, add_n_ids]
    const float* add_ids = nullptr;           //              (mve_unet_bind_added_cond)
    int add_text_dtype = 0, add_text_dim = 0, add_n_ids = 0;
    int clip_eos = 0;                         // CLIP text tower: eos_token_id of this forward (pooling rule of mve_clip_pool)
    const float* sd_boxes = nullptr; const float* sd_points = nullptr; const int32_t* sd_labels = nullptr;      // SAM decoder: the prompts of this forward (null: none)
    int loftr_M = 0, loftr_border = 2;        // LoFTR: match count of the fine call (host value), border / threshold of the coarse selection
    float loftr_thr = 0.2f;
    hipStream_t stream = nullptr;
    void* p(const Ref& r) const {
        switch (r.kind) {
            case Ref::WS: return ws + r.off;
            case Ref::WT: return wt + r.off;
            case Ref::SAMPLE: return (void*)((const unsigned char*)sample + r.off);
            case Ref::TIMESTEPS: return (void*)timesteps;
            case Ref::CTX: return (void*)((const unsigned char*)ctx + r.off);
            case Ref::OUT: return out;
            case Ref::DOWNRES: return (void*)down_res[r.idx];
            case Ref::MIDRES: return (void*)mid_res;
            case Ref::REFSTORE: return ref_store + r.off;
            case Ref::CNCOND: return (void*)cn_cond;
            case Ref::CNOUT: return cn_out[r.idx];
            default: return nullptr;
        }
    }
};

struct Op {
    int cls;
    double flops;
    const char* what;
    std::function<int(const Run&)> fn;
};

// attention-processor options of the reference that change the op list
//   ip_tokens > 0 : IPAttnProcessor2_0 (lib/models/architecture/ip_adapter/attention_processor.py:301-396): the last ip_tokens rows
//                   of encoder_hidden_states go through to_k_ip/to_v_ip and a second softmax, added with ip_scale;
//   ref_mode      : ReferenceAttnProc / ReferenceOnlyAttnProc (lib/models/architecture/diffusers.py:646-673,
//                   lib/pipelines/zero123plus.py:43-77): 1 = 'w' (store the self-attention keys/values of every layer),
//                   2 = 'r'/'m' (append the stored tokens to every self-attention's keys/values); ref_skip leading batch items
//                   neither store nor read (is_cfg_guidance); ref_H x ref_W = latent size of the pass that wrote the store.
//   residual_pair : not a processor option but a plan option of this engine (mve_unet_set_residual_mode): the residual stream of ResnetBlock2D /
//                   BasicTransformerBlock / Transformer2DModel is kept as an unrounded (hi, lo) pair of 16-bit tensors (include/mvedit_amd.h).
//   cn_cond_repeat: ControlNet plans only (mve_controlnet_set_cond_repeat): the conditioning images are given for B / R items and item b uses image
//                   b mod (B / R) -- under classifier-free guidance both halves of the batch see the same control images
//                   (mvedit_3d_pipeline.py:1232: `ctrl_images.split(diff_bs) * 2`), so the conditioning embedding runs once, not R times.
//   ctx_tail      : mve_unet_set_context_tail: the last ctx_tail rows of every item's encoder_hidden_states are ignored -- CNAttnProcessor2_0
//                   (lib/models/architecture/ip_adapter/attention_processor.py:472-480) on a ControlNet under an IP-Adapter, whose context carries
//                   image tokens the ControlNet must not attend to.  Not combined with ip_tokens.
//   cfg_prefix    : UNet plans only (mve_unet_tune_cfg_prefix, default on): the ops in front of the first cross-attention run for the first half of
//                   the batch alone whenever a device-side probe finds the two halves of sample and time embedding identical (builder_unet.h).
struct AttnOpts {
    int ip_tokens = 0; float ip_scale = 1.0f;
    int ref_mode = 0, ref_H = 0, ref_W = 0, ref_skip = 0;
    int residual_pair = 0;
    int cn_cond_repeat = 1;
    int cfg_prefix = 1;
    int ctx_tail = 0;
    bool operator==(const AttnOpts& o) const {
        return ip_tokens == o.ip_tokens && ip_scale == o.ip_scale && ref_mode == o.ref_mode && ref_H == o.ref_H && ref_W == o.ref_W &&
               ref_skip == o.ref_skip && residual_pair == o.residual_pair && cn_cond_repeat == o.cn_cond_repeat && cfg_prefix == o.cfg_prefix && ctx_tail == o.ctx_tail;
    }
};

struct Plan {
    int B = 0, H = 0, W = 0, n_img = 1, has_res = 0, io_dtype = 0, res_nhwc = 0, ctx_len = 0;
    int add_type = 0;          // Config::add_type the plan was built for
    AttnOpts ao;
    size_t ref_store_bytes = 0;
    unsigned long long last_use = 0;
    unsigned long long uid = 0;       // unique per built plan (graph cache key: plan objects are recycled by the LRU)
    std::vector<Op> ops;
    size_t enc_end = 0;        // ops[0, enc_end) = unet_enc
    size_t ws_bytes = 0;
    bool cfg_prefix = false;   // the CFG prefix is planned (AttnOpts::cfg_prefix and the conditions in Builder::build)
    size_t cfg_flag_off = 0;   // its device flag: a word of the workspace's tail pad
    double flops[OC_COUNT] = {0, 0, 0, 0, 0};
};

// plan-time first-fit allocator with coalescing
struct Arena {
    struct Blk { size_t off, size; bool free; };
    std::vector<Blk> b;
    size_t top = 0, peak = 0;
    size_t alloc(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        for (size_t i = 0; i < b.size(); ++i)
            if (b[i].free && b[i].size >= bytes) {
                if (b[i].size > bytes) {
                    Blk rest{b[i].off + bytes, b[i].size - bytes, true};
                    b[i].size = bytes;
                    b.insert(b.begin() + i + 1, rest);
                }
                b[i].free = false;
                return b[i].off;
            }
        if (!b.empty() && b.back().free) {   // grow the trailing free block
            top += bytes - b.back().size;
            b.back().size = bytes;
            b.back().free = false;
            peak = top > peak ? top : peak;
            return b.back().off;
        }
        b.push_back({top, bytes, false});
        top += bytes;
        peak = top > peak ? top : peak;
        return b.back().off;
    }
    void release(size_t off) {
        for (size_t i = 0; i < b.size(); ++i)
            if (b[i].off == off && !b[i].free) {
                b[i].free = true;
                if (i + 1 < b.size() && b[i + 1].free) { b[i].size += b[i + 1].size; b.erase(b.begin() + i + 1); }
                if (i > 0 && b[i - 1].free) { b[i - 1].size += b[i].size; b.erase(b.begin() + i); }
                return;
            }
    }
};

struct Unet {
    Config cfg;
    std::map<std::string, Param> params;     // packed tensors, by engine name
    std::map<std::string, Source> sources;   // every accepted state-dict name -> where and how it is packed (written by the layout alone)
    std::map<std::string, bool> loaded;      // diffusers names seen
    std::vector<std::string> expected;       // diffusers names required
    unsigned char* slab = nullptr;
    size_t slab_bytes = 0;
    int sum_temb = 0, sum_kv = 0;
    std::map<std::string, int> temb_off, kv_off;   // resnet prefix -> column offset; attn2 prefix -> column offset
    std::vector<std::unique_ptr<Plan>> plans;   // small LRU cache: 2-pass mode alternates write/read/decode plans every step
    Plan* cur = nullptr;
    unsigned long long tick = 0;
    AttnOpts ao;
    unsigned char* ref_store = nullptr;
    size_t ref_store_bytes = 0;
    int n_ip_loaded = 0, n_xf_layers = 0;
    bool sd_pe_ready = false;                   // SAM decoder: the dense positional encoding slot is filled (mve_sam_decoder_finalize)
    bool fuse_sc = false;                       // conv_shortcut folded into conv2's K loop (all widths multiples of 64)
    std::string err;
    // added conditions of a 'text_time' handle, bound by mve_unet_bind_added_cond (caller-owned device memory)
    struct AddedCond { const void* text = nullptr; const float* ids = nullptr; int text_dtype = 0, text_dim = 0, n_ids = 0, B = 0; } added;
    // optional hipGraph replay of mve_unet_forward (mve_unet_graph): a call whose plan AND every pointer argument equal an earlier
    // call's is captured on its second sighting and replayed from then on (launch-bound small-batch forwards, e.g. 8 images per rank)
    struct GraphEntry {
        unsigned long long plan_uid = 0;
        int phase = 0, seen = 0;
        std::vector<const void*> ptrs;          // sample, timesteps, ctx, out, workspace, mid residual, ref store, stream, down residuals...
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        unsigned long long last_use = 0;
    };
    // CFG prefix: the flag of the last forward that ran a prologue (null: that plan had no prefix) and the stream it ran on (mve_unet_cfg_prefix_state)
    const int* cfg_flag = nullptr;
    hipStream_t cfg_stream = nullptr;
    bool graph_mode = false;
    std::vector<GraphEntry> graphs;
    unsigned long long plan_counter = 0;
};

int esz(int dtype) { return dtype == MVE_F32 ? 4 : 2; }

// torchvision VGG16 `features` indices of the 13 convolutions, their widths, and lpips' five slices (relu1_2 ... relu5_3)
constexpr int VGG_IDX[13] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};
constexpr int VGG_CIN[13] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int VGG_COUT[13] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int VGG_SLICE[13] = {1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5};
constexpr int VGG_BLK_FIRST[6] = {0, 2, 4, 7, 10, 13};
std::string vgg_name(int i) { return "net.slice" + std::to_string(VGG_SLICE[i]) + "." + std::to_string(VGG_IDX[i]); }

// enumerate blocks in execution order ------------------------------------------------------------------
struct ResnetDesc { std::string name; int cin, cout; };
struct XfDesc { std::string name; int c, heads, layers; };

void enumerate(const Config& c, std::vector<ResnetDesc>& rs, std::vector<XfDesc>& xs) {
    const int n = c.n_levels, L = c.layers_per_block;
    switch (c.kind) {
        case Kind::UNet: case Kind::ControlNet: case Kind::VaeDecoder: case Kind::VaeEncoder: break;      // resnets and transformers, listed below
        default: return;     // plain conv stacks / the CLIP towers, the Resampler (builder_clip*.h), DPT (builder_dpt.h), LoFTR (builder_loftr.h), SAM (builder_sam.h, builder_sam_decoder.h)
    }
    if (c.is_vae()) {      // diffusers Encoder / Decoder (autoencoders/vae.py): resnets only, one attention in the mid block
        const int Cm = c.ch[n - 1];
        if (c.kind == Kind::VaeEncoder) {
            int cin = c.ch[0];
            for (int i = 0; i < n; ++i) {
                for (int j = 0; j < L; ++j)
                    rs.push_back({"down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? cin : c.ch[i], c.ch[i]});
                cin = c.ch[i];
            }
        }
        rs.push_back({"mid_block.resnets.0", Cm, Cm});
        rs.push_back({"mid_block.resnets.1", Cm, Cm});
        if (c.kind == Kind::VaeDecoder) {
            int cin = Cm;
            for (int i = 0; i < n; ++i) {
                const int cout = c.ch[n - 1 - i];
                for (int j = 0; j < L + 1; ++j)
                    rs.push_back({"up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? cin : cout, cout});
                cin = cout;
            }
        }
        return;
    }
    int cin = c.ch[0];
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < L; ++j) {
            rs.push_back({"down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? cin : c.ch[i], c.ch[i]});
            if (c.attn[i]) xs.push_back({"down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), c.ch[i], c.heads[i], c.tlayers[i]});
        }
        cin = c.ch[i];
    }
    rs.push_back({"mid_block.resnets.0", c.ch[n - 1], c.ch[n - 1]});
    xs.push_back({"mid_block.attentions.0", c.ch[n - 1], c.heads[n - 1], c.tlayers[n - 1]});
    rs.push_back({"mid_block.resnets.1", c.ch[n - 1], c.ch[n - 1]});
    if (c.kind == Kind::ControlNet) return;
    int prev = c.ch[n - 1];
    for (int i = 0; i < n; ++i) {
        const int lvl = n - 1 - i, cout = c.ch[lvl];
        const int in_blk = c.ch[(lvl - 1) > 0 ? (lvl - 1) : 0];
        for (int j = 0; j < L + 1; ++j) {
            const int skip = (j == L) ? in_blk : cout;
            const int rin = (j == 0) ? prev : cout;
            rs.push_back({"up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), rin + skip, cout});
            if (c.attn[lvl]) xs.push_back({"up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), cout, c.heads[lvl], c.tlayers[lvl]});
        }
        prev = cout;
    }
}

}  // namespace
