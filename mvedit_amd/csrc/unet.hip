// UNet2DCondition executor: a native (C++) runtime behind the reference's `self.unet(...)` seam
// (lib/pipelines/adapter3d_mixin.py:117-125) and its two halves `unet_enc` / `unet_dec`
// (lib/models/architecture/diffusers.py:57-99, :102-164).
//
// Design (MI355X first, not a translation of diffusers' module tree):
//   * activations live in one caller-provided workspace, NHWC ([B*H*W, C] row-major, fp16/bf16), laid out by
//     a plan-time allocator with explicit lifetimes -- tokens for attention and pixels for convolution are
//     the same memory, so the reference's permute/reshape/contiguous traffic does not exist;
//   * the whole forward is a static op list ("plan") built once per (batch, H, W, n_cross_img): every op is
//     one launch of a kernel from gemm.hip / attention.hip / norm.hip / elementwise.hip on one stream;
//   * weights are engine-owned and packed at load time from diffusers' state-dict layout by a device
//     kernel (OIHW -> OHWI, q/k/v fused into one [3C,C] matrix, GEGLU value/gate rows interleaved so the
//     gate is applied in the GEMM epilogue, conv_in/conv_out channels padded 4 -> 8);
//   * work that only depends on (t, text) is hoisted and batched: ONE GEMM produces the time-embedding
//     projections of all ResnetBlocks, ONE GEMM produces K and V of all cross-attention layers;
//   * skip-concats are never materialised except as the GroupNorm output the next conv reads anyway;
//   * per-op HIP-event profiling and analytic FLOP accounting are built in (bench.py's roofline).
//
// Source layout (one translation unit): executor.h (types) -> executor_params.h (parameter slab + loader) -> executor_builder.h (plan
// builder: arena, op recording, and every block more than one network uses) -> builder_{unet,vae,sr,lpips,clip,clip_vision,dpt,loftr,sam,sam_decoder}.h (the plans:
// UNet and ControlNet, the two VAE halves, SRVGG, LPIPS, CLIP text, CLIP vision and the Resampler, DPT, LoFTR, the SAM image encoder, the SAM mask decoder) -> this file (plan cache + C ABI).
#include "executor_builder.h"
#include "builder_unet.h"
#include "builder_vae.h"
#include "builder_sr.h"
#include "builder_lpips.h"
#include "builder_clip.h"
#include "builder_clip_vision.h"
#include "builder_dpt.h"
#include "builder_loftr.h"
#include "builder_sam.h"
#include "builder_sam_decoder.h"

namespace {

// what a plan is built for and cached under, next to the handle's own options (AttnOpts, add_type).  The networks without conditioning use the first
// three and io_dtype; the CLIP text tower and the Resampler put their sequence length in H, LoFTR its phase in n_img, the SAM decoder its items in B, the prompts
// per image in H, the points per prompt in W and the presence of a box in has_res.
struct PlanKey { int B = 0, H = 0, W = 0, n_img = 1, has_res = 0, io_dtype = 0, res_nhwc = 0, ctx_len = 0; };

int ensure_plan(Unet& u, const PlanKey& k) {
    ++u.tick;
    for (auto& pp : u.plans) {
        const Plan& p = *pp;
        if (p.B == k.B && p.H == k.H && p.W == k.W && p.n_img == k.n_img && p.has_res == k.has_res && p.io_dtype == k.io_dtype &&
            p.res_nhwc == k.res_nhwc && p.ctx_len == k.ctx_len && p.add_type == u.cfg.add_type && p.ao == u.ao) {
            pp->last_use = u.tick;
            u.cur = pp.get();
            return MVE_OK;
        }
    }
    std::unique_ptr<Plan> np(new Plan());
    np->ao = u.ao;
    Builder b(u, *np);
    b.ctx_rows_per_img = k.ctx_len;
    u.cur = nullptr;
    int rc = MVE_ERR_ARG;
    switch (u.cfg.kind) {
        case Kind::UNet: case Kind::ControlNet: rc = b.build(k.B, k.H, k.W, k.n_img, k.has_res, k.io_dtype, k.res_nhwc); break;
        case Kind::VaeDecoder: case Kind::VaeEncoder: rc = b.build_vae(k.B, k.H, k.W, k.io_dtype); break;
        case Kind::Srvgg: rc = b.build_sr(k.B, k.H, k.W, k.io_dtype); break;
        case Kind::Lpips: rc = b.build_lpips(k.B, k.H, k.W, k.io_dtype); break;
        case Kind::ClipText: rc = b.build_clip(k.B, k.H); break;
        case Kind::ClipVision: rc = b.build_clip_vision(k.B); break;
        case Kind::Resampler: rc = b.build_resampler(k.B, k.H); break;
        case Kind::Dpt: rc = b.build_dpt(k.B); break;
        case Kind::Loftr: rc = b.build_loftr(k.B, k.H, k.W, k.n_img); break;
        case Kind::Sam: rc = b.build_sam(k.B); break;
        case Kind::SamDecoder: rc = b.build_sam_decoder(k.B, k.H, k.W, k.has_res); break;
    }
    if (rc != MVE_OK) return rc;
    np->ctx_len = k.ctx_len;
    np->last_use = u.tick;
    np->uid = ++u.plan_counter;
    if (u.plans.size() >= 8) {
        size_t lru = 0;
        for (size_t i = 1; i < u.plans.size(); ++i)
            if (u.plans[i]->last_use < u.plans[lru]->last_use) lru = i;
        u.plans.erase(u.plans.begin() + lru);
    }
    u.plans.push_back(std::move(np));
    u.cur = u.plans.back().get();
    return MVE_OK;
}

// added conditions of a forward that runs the prologue: checked against the handle and the batch, then handed to the ops through Run
int take_added_cond(const Unet& u, int B, Run& r, const char* who) {
    if (!u.cfg.add_type) return MVE_OK;
    const Unet::AddedCond& a = u.added;
    MVE_CHECK(a.text && a.ids, MVE_ERR_STATE, "%s: addition_embed_type 'text_time' needs text_embeds / time_ids (mve_unet_bind_added_cond) before the forward", who);
    MVE_CHECK(a.B == B, MVE_ERR_ARG, "%s: added conditions are bound for a batch of %d, the forward runs %d", who, a.B, B);
    r.add_text = a.text; r.add_ids = a.ids; r.add_text_dtype = a.text_dtype; r.add_text_dim = a.text_dim; r.add_n_ids = a.n_ids;
    return MVE_OK;
}

// the handle as an engine of one of the wanted kinds
int as_engine(void* handle, const char* who, std::initializer_list<Kind> wanted, Unet*& u) {
    MVE_CHECK(handle, MVE_ERR_ARG, "%s: null handle", who);
    u = (Unet*)handle;
    for (Kind k : wanted)
        if (u->cfg.kind == k) return MVE_OK;
    mve_set_error("%s: handle is %s, not %s", who, kind_name(u->cfg.kind), kind_name(*wanted.begin()));
    return MVE_ERR_ARG;
}

// the three outputs of every *_plan call, from the current plan
void report_plan(const Plan& pl, size_t* workspace_bytes, int* n_ops, double* flops) {
    if (workspace_bytes) *workspace_bytes = pl.ws_bytes;
    if (n_ops) *n_ops = (int)pl.ops.size();
    if (flops) for (int i = 0; i < OC_COUNT; ++i) flops[i] = pl.flops[i];
}

int plan_and_report(Unet& u, const PlanKey& key, size_t* workspace_bytes, int* n_ops, double* flops) {
    const int rc = ensure_plan(u, key);
    if (rc) return rc;
    report_plan(*u.cur, workspace_bytes, n_ops, flops);
    return MVE_OK;
}

// The front of every forward call, in this order: null handle, kind, every parameter loaded, the call's own argument checks, plan, workspace size.
// `args(u, key)` checks the arguments that are the call's own and fills the plan key (it may need the handle's configuration for either).
template <class Args>
int begin_forward(void* handle, const char* who, std::initializer_list<Kind> wanted, Args&& args, const void* d_workspace, size_t workspace_bytes, Unet*& u,
                  const Plan*& pl) {
    int rc = as_engine(handle, who, wanted, u);
    if (rc) return rc;
    char first[256];
    const int miss = mve_unet_missing_params(handle, first, sizeof(first));
    MVE_CHECK(miss == 0, MVE_ERR_STATE, "%s: %d parameters not loaded (first: %s)", who, miss, first);
    PlanKey key;
    rc = args(*u, key);
    if (rc) return rc;
    rc = ensure_plan(*u, key);
    if (rc) return rc;
    pl = u->cur;
    MVE_CHECK(d_workspace && workspace_bytes >= pl->ws_bytes, MVE_ERR_NOMEM, "%s: workspace %zu < required %zu", who, workspace_bytes, pl->ws_bytes);
    return MVE_OK;
}

// the events of a timed run: destroyed on every way out of it
struct OpEvents {
    std::vector<hipEvent_t> ev;
    ~OpEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    int create(size_t n) {
        ev.assign(n, nullptr);
        for (auto& e : ev) MVE_HIP(hipEventCreate(&e));
        return MVE_OK;
    }
};

// ops [lo, hi) of a plan on one stream; with op_ms (a host array indexed by the absolute op index) each op is timed and the stream is synchronised
int run_plan_ops(const Plan& pl, const Run& r, size_t lo, size_t hi, float* op_ms) {
    OpEvents t;
    if (op_ms) {
        const int rc = t.create(hi - lo + 1);
        if (rc) return rc;
        MVE_HIP(hipEventRecord(t.ev[0], r.stream));
    }
    for (size_t i = lo; i < hi; ++i) {
        const int rc = pl.ops[i].fn(r);
        if (rc) return rc;
        if (op_ms) MVE_HIP(hipEventRecord(t.ev[i - lo + 1], r.stream));
    }
    if (op_ms) {
        MVE_HIP(hipStreamSynchronize(r.stream));
        for (size_t i = lo; i < hi; ++i) MVE_HIP(hipEventElapsedTime(&op_ms[i], t.ev[i - lo], t.ev[i - lo + 1]));
    }
    return MVE_OK;
}

Run new_run(const Unet& u, void* d_workspace, void* stream) {
    Run r;
    r.ws = (unsigned char*)d_workspace; r.wt = u.slab; r.stream = (hipStream_t)stream;
    return r;
}

// mve_unet_create / mve_controlnet_create: the topology arguments the two share, checked and filled into a new handle
int create_denoiser(void** handle, const char* who, Kind kind, int dtype, int in_channels, int out_channels, int n_levels, const int* block_out_channels,
                    int layers_per_block, const int* down_attn, const int* num_heads, const int* transformer_layers, int cross_attention_dim,
                    int norm_num_groups, float norm_eps, int use_linear_projection) {
    MVE_CHECK(handle, MVE_ERR_ARG, "%s: null handle", who);
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "%s: dtype must be f16 or bf16", who);
    MVE_CHECK(n_levels >= 1 && n_levels <= MAX_LEVELS && layers_per_block >= 1, MVE_ERR_ARG, "%s: bad topology", who);
    MVE_CHECK(in_channels >= 1 && in_channels <= 8 && out_channels >= 1 && out_channels <= 8, MVE_ERR_ARG, "%s: in/out channels must be <= 8", who);
    MVE_CHECK(cross_attention_dim % 8 == 0, MVE_ERR_ARG, "%s: cross_attention_dim must be a multiple of 8", who);
    std::unique_ptr<Unet> u(new Unet());
    Config& c = u->cfg;
    c.kind = kind;
    c.dtype = dtype; c.in_ch = in_channels; c.out_ch = out_channels; c.n_levels = n_levels; c.layers_per_block = layers_per_block;
    c.ctx_dim = cross_attention_dim; c.groups = norm_num_groups; c.eps = norm_eps; c.linear_proj = use_linear_projection;
    for (int i = 0; i < n_levels; ++i) {
        c.ch[i] = block_out_channels[i]; c.attn[i] = down_attn[i]; c.heads[i] = num_heads[i]; c.tlayers[i] = transformer_layers[i];
        MVE_CHECK(c.ch[i] % 32 == 0 && c.ch[i] % c.groups == 0 && (!c.attn[i] || c.ch[i] % c.heads[i] == 0), MVE_ERR_ARG,
                  "%s: channel count %d incompatible with groups/heads", who, block_out_channels[i]);
    }
    *handle = u.release();
    return MVE_OK;
}

}  // namespace

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

int mve_unet_create(void** handle, int dtype, int in_channels, int out_channels, int n_levels, const int* block_out_channels,
                    int layers_per_block, const int* down_attn, const int* num_heads, const int* transformer_layers,
                    int cross_attention_dim, int norm_num_groups, float norm_eps, int use_linear_projection) {
    const int rc = create_denoiser(handle, "unet_create", Kind::UNet, dtype, in_channels, out_channels, n_levels, block_out_channels, layers_per_block, down_attn,
                                   num_heads, transformer_layers, cross_attention_dim, norm_num_groups, norm_eps, use_linear_projection);
    if (rc) return rc;
    Unet* u = (Unet*)*handle;
    layout_params(*u);   // host-side only; device storage is allocated by the first mve_unet_load_param
    // Round 5: the UNet's residual stream is an unrounded (hi, lo) pair BY DEFAULT -- the mode whose end-to-end error against fp32 arithmetic is
    // inside north_star's 1e-3 (8.7e-4 at the benchmark shape; the reference's rounding points give 1.2e-3).  MVE_RESIDUAL_PAIR=0 or
    // mve_unet_set_residual_mode(handle, 0) restore the 16-bit stream.  ControlNet / VAE handles keep the 16-bit stream unless asked.
    const char* e = getenv("MVE_RESIDUAL_PAIR");
    u->ao.residual_pair = e ? (atoi(e) != 0) : 1;
    return MVE_OK;
}

int mve_controlnet_create(void** handle, int dtype, int in_channels, int conditioning_channels, int n_levels, const int* block_out_channels,
                          int layers_per_block, const int* down_attn, const int* num_heads, const int* transformer_layers,
                          int cross_attention_dim, int norm_num_groups, float norm_eps, int use_linear_projection) {
    MVE_CHECK(conditioning_channels >= 1 && conditioning_channels <= 8, MVE_ERR_ARG, "controlnet_create: conditioning channels must be <= 8");
    // same topology arguments as the UNet; build the parameter table in ControlNet mode
    const int rc = create_denoiser(handle, "controlnet_create", Kind::ControlNet, dtype, in_channels, in_channels, n_levels, block_out_channels, layers_per_block,
                                   down_attn, num_heads, transformer_layers, cross_attention_dim, norm_num_groups, norm_eps, use_linear_projection);
    if (rc) return rc;
    Unet* u = (Unet*)*handle;
    u->cfg.cond_ch = conditioning_channels;
    layout_params(*u);
    return MVE_OK;
}

int mve_controlnet_forward(void* handle, const void* d_sample, int io_dtype, const float* d_timesteps, const void* d_ctx, const void* d_cond,
                           int B, int H, int W, int ctx_len, float conditioning_scale, int accumulate, void* const* d_outputs,
                           void* d_workspace, size_t workspace_bytes, float* op_ms, void* stream) {
    Unet* u;
    const Plan* pl;
    int rc = begin_forward(handle, "controlnet_forward", {Kind::ControlNet}, [&](const Unet&, PlanKey& k) -> int {
        MVE_CHECK(d_sample && d_timesteps && d_ctx && d_cond && d_outputs, MVE_ERR_ARG, "controlnet_forward: null pointer");
        k.B = B; k.H = H; k.W = W; k.io_dtype = io_dtype; k.ctx_len = ctx_len;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, pl);
    if (rc) return rc;
    const int n_out = u->cfg.n_levels * (u->cfg.layers_per_block + 1) + 1;
    for (int i = 0; i < n_out; ++i) MVE_CHECK(d_outputs[i], MVE_ERR_ARG, "controlnet_forward: null output %d", i);
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_sample; r.timesteps = d_timesteps; r.ctx = d_ctx;
    r.cn_cond = d_cond; r.cn_out = d_outputs; r.cn_scale = conditioning_scale; r.cn_accum = accumulate ? 1 : 0;
    rc = take_added_cond(*u, B, r, "controlnet_forward");
    if (rc) return rc;
    return run_plan_ops(*pl, r, 0, pl->ops.size(), op_ms);
}

int mve_vae_create(void** handle, int dtype, int half, int in_channels, int out_channels, int n_levels, const int* block_out_channels,
                   int layers_per_block, int norm_num_groups, float norm_eps) {
    MVE_CHECK(handle, MVE_ERR_ARG, "vae_create: null handle");
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "vae_create: dtype must be f16 or bf16");
    MVE_CHECK(half == 1 || half == 2, MVE_ERR_ARG, "vae_create: half must be 1 (decoder) or 2 (encoder)");
    MVE_CHECK(n_levels >= 1 && n_levels <= MAX_LEVELS && layers_per_block >= 1, MVE_ERR_ARG, "vae_create: bad topology");
    MVE_CHECK(in_channels >= 1 && in_channels <= 8 && out_channels >= 1 && out_channels <= 8, MVE_ERR_ARG,
              "vae_create: in/out channels must be <= 8 (encoder: out_channels = 2 * latent_channels)");
    Unet* u = new Unet();
    Config& c = u->cfg;
    c.kind = half == 1 ? Kind::VaeDecoder : Kind::VaeEncoder;
    c.dtype = dtype; c.in_ch = in_channels; c.out_ch = out_channels; c.n_levels = n_levels; c.layers_per_block = layers_per_block;
    c.ctx_dim = 8; c.groups = norm_num_groups; c.eps = norm_eps; c.linear_proj = 0;
    for (int i = 0; i < n_levels; ++i) {
        c.ch[i] = block_out_channels[i]; c.attn[i] = 0; c.heads[i] = 1; c.tlayers[i] = 0;
        if (c.ch[i] % 8 != 0 || c.groups <= 0 || c.ch[i] % c.groups != 0) {
            delete u;
            mve_set_error("vae_create: channel count %d incompatible with %d groups", block_out_channels[i], norm_num_groups);
            return MVE_ERR_ARG;
        }
    }
    layout_params(*u);
    *handle = u;
    return MVE_OK;
}

// image networks (VAE halves, SRVGGNetCompact): one NCHW tensor in, one out, no conditioning
static int imgnet_plan(void* handle, std::initializer_list<Kind> wanted, int B, int H, int W, int io_dtype, size_t* workspace_bytes, int* n_ops, double* flops) {
    MVE_CHECK(handle && B > 0 && H > 0 && W > 0, MVE_ERR_ARG, "plan: bad arguments");
    Unet* u;
    const int rc = as_engine(handle, "plan", wanted, u);
    if (rc) return rc;
    PlanKey k;
    k.B = B; k.H = H; k.W = W; k.io_dtype = io_dtype;
    return plan_and_report(*u, k, workspace_bytes, n_ops, flops);
}

static int imgnet_forward(void* handle, std::initializer_list<Kind> wanted, const void* d_in, int io_dtype, int B, int H, int W, void* d_out, void* d_workspace,
                          size_t workspace_bytes, float* op_ms, void* stream) {
    Unet* u;
    const Plan* pl;
    const int rc = begin_forward(handle, "forward", wanted, [&](const Unet&, PlanKey& k) -> int {
        MVE_CHECK(d_in && d_out, MVE_ERR_ARG, "forward: null pointer");
        k.B = B; k.H = H; k.W = W; k.io_dtype = io_dtype;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, pl);
    if (rc) return rc;
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_in; r.out = d_out;
    return run_plan_ops(*pl, r, 0, pl->ops.size(), op_ms);
}

int mve_vae_plan(void* handle, int B, int H, int W, int io_dtype, size_t* workspace_bytes, int* n_ops, double* flops) {
    return imgnet_plan(handle, {Kind::VaeDecoder, Kind::VaeEncoder}, B, H, W, io_dtype, workspace_bytes, n_ops, flops);
}
int mve_vae_forward(void* handle, const void* d_in, int io_dtype, int B, int H, int W, void* d_out, void* d_workspace,
                    size_t workspace_bytes, float* op_ms, void* stream) {
    return imgnet_forward(handle, {Kind::VaeDecoder, Kind::VaeEncoder}, d_in, io_dtype, B, H, W, d_out, d_workspace, workspace_bytes, op_ms, stream);
}

int mve_srvgg_create(void** handle, int dtype, int num_in_ch, int num_out_ch, int num_feat, int num_conv, int upscale) {
    MVE_CHECK(handle, MVE_ERR_ARG, "srvgg_create: null handle");
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "srvgg_create: dtype must be f16 or bf16");
    MVE_CHECK(num_in_ch >= 1 && num_in_ch <= 8 && num_out_ch == num_in_ch, MVE_ERR_ARG,
              "srvgg_create: 1..8 channels, num_out_ch == num_in_ch (the input is added to the output, image_space_ss.py:68-69)");
    MVE_CHECK(num_feat >= 8 && num_feat % 8 == 0 && num_conv >= 0 && upscale >= 1 && upscale <= 8, MVE_ERR_ARG, "srvgg_create: bad topology");
    Unet* u = new Unet();
    Config& c = u->cfg;
    c.kind = Kind::Srvgg; c.sr_scale = upscale;
    c.dtype = dtype; c.in_ch = num_in_ch; c.out_ch = num_out_ch; c.n_levels = 1; c.layers_per_block = num_conv;
    c.ctx_dim = 8; c.groups = 1; c.eps = 0.f; c.linear_proj = 0;
    c.ch[0] = num_feat; c.attn[0] = 0; c.heads[0] = 1; c.tlayers[0] = 0;
    layout_params(*u);
    *handle = u;
    return MVE_OK;
}
int mve_srvgg_plan(void* handle, int B, int H, int W, int io_dtype, size_t* workspace_bytes, int* n_ops, double* flops) {
    return imgnet_plan(handle, {Kind::Srvgg}, B, H, W, io_dtype, workspace_bytes, n_ops, flops);
}
int mve_srvgg_forward(void* handle, const void* d_in, int io_dtype, int B, int H, int W, void* d_out, void* d_workspace,
                      size_t workspace_bytes, float* op_ms, void* stream) {
    return imgnet_forward(handle, {Kind::Srvgg}, d_in, io_dtype, B, H, W, d_out, d_workspace, workspace_bytes, op_ms, stream);
}

int mve_clip_text_create(void** handle, int dtype, int vocab_size, int max_position_embeddings, int hidden_size, int num_layers, int num_heads,
                         int intermediate_size, int act, float layer_norm_eps, int projection_dim) {
    MVE_CHECK(handle, MVE_ERR_ARG, "clip_text_create: null handle");
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "clip_text_create: dtype must be f16 or bf16");
    MVE_CHECK(vocab_size >= 1 && max_position_embeddings >= 1, MVE_ERR_ARG, "clip_text_create: bad vocab_size %d / max_position_embeddings %d", vocab_size,
              max_position_embeddings);
    MVE_CHECK(num_layers >= 1 && num_heads >= 1, MVE_ERR_ARG, "clip_text_create: bad num_layers %d / num_heads %d", num_layers, num_heads);
    MVE_CHECK(hidden_size == num_heads * 64, MVE_ERR_ARG, "clip_text_create: hidden_size %d must be num_heads * 64 (head_dim 64 only; %d heads)", hidden_size, num_heads);
    MVE_CHECK(hidden_size <= 2048, MVE_ERR_ARG, "clip_text_create: hidden_size %d exceeds the 2048 channels of mve_layernorm", hidden_size);
    MVE_CHECK(intermediate_size >= 8 && intermediate_size % 8 == 0, MVE_ERR_ARG, "clip_text_create: intermediate_size %d must be a multiple of 8", intermediate_size);
    MVE_CHECK(act == MVE_ACT_QUICK_GELU || act == MVE_ACT_GELU, MVE_ERR_ARG, "clip_text_create: act %d (0 = quick_gelu, 1 = gelu)", act);
    MVE_CHECK(projection_dim >= 0 && projection_dim % 8 == 0, MVE_ERR_ARG, "clip_text_create: projection_dim %d must be a multiple of 8 (0 = none)", projection_dim);
    MVE_CHECK(layer_norm_eps > 0.f, MVE_ERR_ARG, "clip_text_create: layer_norm_eps must be positive");
    Unet* u = new Unet();
    Config& c = u->cfg;
    c.kind = Kind::ClipText; c.clip_vocab = vocab_size; c.clip_max_pos = max_position_embeddings; c.clip_inter = intermediate_size; c.clip_act = act;
    c.clip_proj = projection_dim;
    c.dtype = dtype; c.in_ch = 1; c.out_ch = 1; c.n_levels = 1; c.layers_per_block = num_layers;
    c.ctx_dim = 8; c.groups = 1; c.eps = layer_norm_eps; c.linear_proj = 0;
    c.ch[0] = hidden_size; c.attn[0] = 0; c.heads[0] = num_heads; c.tlayers[0] = 0;
    layout_params(*u);
    *handle = u;
    return MVE_OK;
}

// the CLIP towers' output table (Run::cn_out): last hidden state, pooled output, projected embeddings, then the optional hidden states
static int clip_outputs(const char* who, const Unet& u, void* d_last, void* d_pooled, void* d_embeds, void* const* d_hidden_states, std::vector<void*>& outs) {
    const int n_hidden = u.cfg.layers_per_block + 1;
    outs.assign(CLIP_OUT_HIDDEN0 + n_hidden, nullptr);
    outs[CLIP_OUT_LAST] = d_last; outs[CLIP_OUT_POOLED] = d_pooled; outs[CLIP_OUT_EMBEDS] = d_embeds;
    if (d_hidden_states)
        for (int i = 0; i < n_hidden; ++i) {
            MVE_CHECK(d_hidden_states[i], MVE_ERR_ARG, "%s: null d_hidden_states[%d]", who, i);
            outs[CLIP_OUT_HIDDEN0 + i] = d_hidden_states[i];
        }
    return MVE_OK;
}

int mve_clip_text_plan(void* handle, int B, int L, size_t* workspace_bytes, int* n_ops, double* flops) {
    MVE_CHECK(handle && B > 0 && L > 0, MVE_ERR_ARG, "clip_text_plan: bad arguments");
    Unet* u;
    const int rc = as_engine(handle, "clip_text_plan", {Kind::ClipText}, u);
    if (rc) return rc;
    PlanKey k;
    k.B = B; k.H = L; k.W = 1; k.io_dtype = u->cfg.dtype;
    return plan_and_report(*u, k, workspace_bytes, n_ops, flops);
}

int mve_clip_text_forward(void* handle, const int32_t* d_ids, int B, int L, int eos_token_id, void* d_last_hidden_state, void* d_pooler_output,
                          void* d_text_embeds, void* const* d_hidden_states, void* d_workspace, size_t workspace_bytes, float* op_ms, void* stream) {
    Unet* u;
    const Plan* pl;
    int rc = begin_forward(handle, "clip_text_forward", {Kind::ClipText}, [&](const Unet& e, PlanKey& k) -> int {
        MVE_CHECK(d_ids && d_last_hidden_state && d_pooler_output, MVE_ERR_ARG, "clip_text_forward: null pointer (d_ids / d_last_hidden_state / d_pooler_output)");
        MVE_CHECK(e.cfg.clip_proj ? d_text_embeds != nullptr : d_text_embeds == nullptr, MVE_ERR_ARG,
                  "clip_text_forward: d_text_embeds must be given exactly when the handle has a text_projection (projection_dim %d)", e.cfg.clip_proj);
        MVE_CHECK(B > 0 && L > 0, MVE_ERR_ARG, "clip_text_forward: bad B %d / L %d", B, L);
        k.B = B; k.H = L; k.W = 1; k.io_dtype = e.cfg.dtype;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, pl);
    if (rc) return rc;
    std::vector<void*> outs;
    rc = clip_outputs("clip_text_forward", *u, d_last_hidden_state, d_pooler_output, d_text_embeds, d_hidden_states, outs);
    if (rc) return rc;
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_ids;
    r.cn_out = outs.data();
    r.clip_eos = eos_token_id;
    return run_plan_ops(*pl, r, 0, pl->ops.size(), op_ms);
}

int mve_clip_vision_create(void** handle, int dtype, int image_size, int patch_size, int hidden_size, int num_layers, int num_heads, int intermediate_size,
                           int act, float layer_norm_eps, int projection_dim) {
    MVE_CHECK(handle, MVE_ERR_ARG, "clip_vision_create: null handle");
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "clip_vision_create: dtype must be f16 or bf16");
    MVE_CHECK(image_size >= 1 && patch_size >= 1 && patch_size <= image_size && image_size <= 4096, MVE_ERR_ARG, "clip_vision_create: bad image_size %d / patch_size %d",
              image_size, patch_size);
    MVE_CHECK(image_size % patch_size == 0, MVE_ERR_ARG, "clip_vision_create: image_size %d must be a multiple of patch_size %d", image_size, patch_size);
    MVE_CHECK(num_layers >= 1 && num_heads >= 1, MVE_ERR_ARG, "clip_vision_create: bad num_layers %d / num_heads %d", num_layers, num_heads);
    MVE_CHECK(hidden_size == num_heads * 64 || hidden_size == num_heads * 80, MVE_ERR_ARG,
              "clip_vision_create: hidden_size %d / num_heads %d: head_dim must be 64 or 80 (%d heads)", hidden_size, num_heads, num_heads);
    MVE_CHECK(hidden_size <= 2048, MVE_ERR_ARG, "clip_vision_create: hidden_size %d exceeds the 2048 channels of mve_layernorm", hidden_size);
    MVE_CHECK(intermediate_size >= 8 && intermediate_size % 8 == 0, MVE_ERR_ARG, "clip_vision_create: intermediate_size %d must be a multiple of 8", intermediate_size);
    MVE_CHECK(act == MVE_ACT_QUICK_GELU || act == MVE_ACT_GELU, MVE_ERR_ARG, "clip_vision_create: act %d (0 = quick_gelu, 1 = gelu)", act);
    MVE_CHECK(projection_dim >= 0 && projection_dim % 8 == 0, MVE_ERR_ARG, "clip_vision_create: projection_dim %d must be a multiple of 8 (0 = none)", projection_dim);
    MVE_CHECK(layer_norm_eps > 0.f, MVE_ERR_ARG, "clip_vision_create: layer_norm_eps must be positive");
    Unet* u = new Unet();
    Config& c = u->cfg;
    c.kind = Kind::ClipVision; c.cv_image = image_size; c.cv_patch = patch_size; c.clip_inter = intermediate_size; c.clip_act = act; c.clip_proj = projection_dim;
    c.dtype = dtype; c.in_ch = 3; c.out_ch = 1; c.n_levels = 1; c.layers_per_block = num_layers;
    c.ctx_dim = 8; c.groups = 1; c.eps = layer_norm_eps; c.linear_proj = 0;
    c.ch[0] = hidden_size; c.attn[0] = 0; c.heads[0] = num_heads; c.tlayers[0] = 0;
    layout_params(*u);
    *handle = u;
    return MVE_OK;
}

int mve_clip_vision_plan(void* handle, int B, size_t* workspace_bytes, int* n_ops, double* flops) {
    MVE_CHECK(handle && B > 0, MVE_ERR_ARG, "clip_vision_plan: bad arguments");
    Unet* u;
    const int rc = as_engine(handle, "clip_vision_plan", {Kind::ClipVision}, u);
    if (rc) return rc;
    PlanKey k;
    k.B = B; k.H = k.W = u->cfg.cv_image; k.io_dtype = u->cfg.dtype;
    return plan_and_report(*u, k, workspace_bytes, n_ops, flops);
}

int mve_clip_vision_forward(void* handle, const void* d_pixels, int B, void* d_last_hidden_state, void* d_pooler_output, void* d_image_embeds,
                            void* const* d_hidden_states, void* d_workspace, size_t workspace_bytes, float* op_ms, void* stream) {
    Unet* u;
    const Plan* pl;
    int rc = begin_forward(handle, "clip_vision_forward", {Kind::ClipVision}, [&](const Unet& e, PlanKey& k) -> int {
        MVE_CHECK(d_pixels && d_last_hidden_state && d_pooler_output, MVE_ERR_ARG, "clip_vision_forward: null pointer (d_pixels / d_last_hidden_state / d_pooler_output)");
        MVE_CHECK(e.cfg.clip_proj ? d_image_embeds != nullptr : d_image_embeds == nullptr, MVE_ERR_ARG,
                  "clip_vision_forward: d_image_embeds must be given exactly when the handle has a visual_projection (projection_dim %d)", e.cfg.clip_proj);
        MVE_CHECK(B > 0, MVE_ERR_ARG, "clip_vision_forward: bad B %d", B);
        MVE_CHECK(((uintptr_t)d_pixels & 15) == 0, MVE_ERR_ARG, "clip_vision_forward: d_pixels must be 16-byte aligned");
        k.B = B; k.H = k.W = e.cfg.cv_image; k.io_dtype = e.cfg.dtype;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, pl);
    if (rc) return rc;
    std::vector<void*> outs;
    rc = clip_outputs("clip_vision_forward", *u, d_last_hidden_state, d_pooler_output, d_image_embeds, d_hidden_states, outs);
    if (rc) return rc;
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_pixels;
    r.cn_out = outs.data();
    return run_plan_ops(*pl, r, 0, pl->ops.size(), op_ms);
}

int mve_ip_resampler_create(void** handle, int dtype, int dim, int depth, int heads, int num_queries, int embedding_dim, int output_dim, int ff_mult) {
    MVE_CHECK(handle, MVE_ERR_ARG, "ip_resampler_create: null handle");
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "ip_resampler_create: dtype must be f16 or bf16");
    MVE_CHECK(depth >= 1 && heads >= 1 && num_queries >= 1, MVE_ERR_ARG, "ip_resampler_create: bad depth %d / heads %d / num_queries %d", depth, heads, num_queries);
    MVE_CHECK(dim >= 8 && dim % 8 == 0 && dim <= 2048, MVE_ERR_ARG, "ip_resampler_create: dim %d must be a multiple of 8, at most the 2048 channels of mve_layernorm", dim);
    MVE_CHECK(embedding_dim >= 8 && embedding_dim % 8 == 0, MVE_ERR_ARG, "ip_resampler_create: embedding_dim %d must be a multiple of 8", embedding_dim);
    MVE_CHECK(output_dim >= 8 && output_dim % 8 == 0 && output_dim <= 2048, MVE_ERR_ARG,
              "ip_resampler_create: output_dim %d must be a multiple of 8, at most the 2048 channels of mve_layernorm", output_dim);
    MVE_CHECK(ff_mult >= 1 && ff_mult <= 16, MVE_ERR_ARG, "ip_resampler_create: ff_mult %d must be in [1, 16]", ff_mult);
    const int inner = dim * ff_mult;      // int(dim * mult), resampler.py:10
    Unet* u = new Unet();
    Config& c = u->cfg;
    c.kind = Kind::Resampler; c.rs_queries = num_queries; c.rs_embed = embedding_dim; c.rs_out = output_dim; c.rs_inner = inner;
    c.dtype = dtype; c.in_ch = 1; c.out_ch = 1; c.n_levels = 1; c.layers_per_block = depth;
    c.ctx_dim = 8; c.groups = 1; c.eps = 1e-5f; c.linear_proj = 0;
    c.ch[0] = dim; c.attn[0] = 0; c.heads[0] = heads; c.tlayers[0] = 0;
    layout_params(*u);
    *handle = u;
    return MVE_OK;
}

int mve_ip_resampler_plan(void* handle, int B, int n1, size_t* workspace_bytes, int* n_ops, double* flops) {
    MVE_CHECK(handle && B > 0 && n1 > 0, MVE_ERR_ARG, "ip_resampler_plan: bad arguments");
    Unet* u;
    const int rc = as_engine(handle, "ip_resampler_plan", {Kind::Resampler}, u);
    if (rc) return rc;
    PlanKey k;
    k.B = B; k.H = n1; k.W = 1; k.io_dtype = u->cfg.dtype;
    return plan_and_report(*u, k, workspace_bytes, n_ops, flops);
}

int mve_ip_resampler_forward(void* handle, const void* d_x, int B, int n1, void* d_out, void* d_workspace, size_t workspace_bytes, float* op_ms, void* stream) {
    Unet* u;
    const Plan* pl;
    const int rc = begin_forward(handle, "ip_resampler_forward", {Kind::Resampler}, [&](const Unet& e, PlanKey& k) -> int {
        MVE_CHECK(d_x && d_out, MVE_ERR_ARG, "ip_resampler_forward: null pointer (d_x / d_out)");
        MVE_CHECK(B > 0 && n1 > 0, MVE_ERR_ARG, "ip_resampler_forward: bad B %d / n1 %d", B, n1);
        MVE_CHECK(((uintptr_t)d_x & 15) == 0 && ((uintptr_t)d_out & 15) == 0, MVE_ERR_ARG, "ip_resampler_forward: d_x / d_out must be 16-byte aligned");
        k.B = B; k.H = n1; k.W = 1; k.io_dtype = e.cfg.dtype;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, pl);
    if (rc) return rc;
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_x; r.out = d_out;
    return run_plan_ops(*pl, r, 0, pl->ops.size(), op_ms);
}

int mve_dpt_create(void** handle, int dtype, int image_size, int stem_width, const int* stage_widths, const int* stage_depths, int num_groups, int hidden_size,
                   int num_layers, int num_heads, int intermediate_size, const int* tap_layers, const int* neck_channels, int features, int num_channels,
                   float layer_norm_eps) {
    MVE_CHECK(handle && stage_widths && stage_depths && tap_layers && neck_channels, MVE_ERR_ARG, "dpt_create: null pointer");
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "dpt_create: dtype must be f16 or bf16");
    MVE_CHECK(image_size >= 32 && image_size % 32 == 0 && image_size <= 2048, MVE_ERR_ARG, "dpt_create: image_size %d must be a multiple of 32 in [32, 2048]", image_size);
    MVE_CHECK(num_groups >= 1 && stem_width >= 8 && stem_width % 8 == 0 && stem_width % num_groups == 0, MVE_ERR_ARG,
              "dpt_create: stem_width %d must be a multiple of 8 and of num_groups %d", stem_width, num_groups);
    for (int s = 0; s < 3; ++s) {
        MVE_CHECK(stage_depths[s] >= 1, MVE_ERR_ARG, "dpt_create: stage_depths[%d] = %d", s, stage_depths[s]);
        MVE_CHECK(stage_widths[s] >= 32 && stage_widths[s] % 32 == 0 && (stage_widths[s] / 4) % num_groups == 0, MVE_ERR_ARG,
                  "dpt_create: stage_widths[%d] = %d must be a multiple of 32 whose quarter (the bottleneck width) is divisible by num_groups %d", s, stage_widths[s], num_groups);
    }
    MVE_CHECK(num_heads >= 1 && hidden_size == num_heads * 64, MVE_ERR_ARG, "dpt_create: hidden_size %d / num_heads %d: head_dim must be 64", hidden_size, num_heads);
    MVE_CHECK(hidden_size <= 2048, MVE_ERR_ARG, "dpt_create: hidden_size %d exceeds the 2048 channels of mve_layernorm", hidden_size);
    MVE_CHECK(intermediate_size >= 8 && intermediate_size % 8 == 0, MVE_ERR_ARG, "dpt_create: intermediate_size %d must be a multiple of 8", intermediate_size);
    MVE_CHECK(num_layers >= 1 && tap_layers[0] >= 0 && tap_layers[0] < tap_layers[1] && tap_layers[1] < num_layers, MVE_ERR_ARG,
              "dpt_create: tap_layers {%d, %d} must be increasing block indices below num_layers %d", tap_layers[0], tap_layers[1], num_layers);
    MVE_CHECK(neck_channels[0] >= 8 && neck_channels[0] % 8 == 0 && neck_channels[1] >= 8 && neck_channels[1] % 8 == 0, MVE_ERR_ARG,
              "dpt_create: neck_channels {%d, %d} must be multiples of 8", neck_channels[0], neck_channels[1]);
    MVE_CHECK(features >= 16 && features % 16 == 0, MVE_ERR_ARG, "dpt_create: features %d must be a multiple of 16 (the head halves it)", features);
    MVE_CHECK(num_channels >= 1 && num_channels <= 8, MVE_ERR_ARG, "dpt_create: num_channels %d must be in [1, 8]", num_channels);
    MVE_CHECK(layer_norm_eps > 0.f, MVE_ERR_ARG, "dpt_create: layer_norm_eps must be positive");
    Unet* u = new Unet();
    Config& c = u->cfg;
    c.kind = Kind::Dpt; c.dp_image = image_size; c.dp_stem = stem_width; c.dp_inter = intermediate_size; c.dp_features = features;
    for (int s = 0; s < 3; ++s) { c.dp_stage[s] = stage_widths[s]; c.dp_depth[s] = stage_depths[s]; }
    for (int k = 0; k < 2; ++k) { c.dp_tap[k] = tap_layers[k]; c.dp_neck[k] = neck_channels[k]; }
    c.dtype = dtype; c.in_ch = 3; c.out_ch = num_channels; c.n_levels = 1; c.layers_per_block = num_layers;
    c.ctx_dim = 8; c.groups = num_groups; c.eps = layer_norm_eps; c.linear_proj = 0;
    c.ch[0] = hidden_size; c.attn[0] = 0; c.heads[0] = num_heads; c.tlayers[0] = 0;
    layout_params(*u);
    *handle = u;
    return MVE_OK;
}

int mve_dpt_plan(void* handle, int B, size_t* workspace_bytes, int* n_ops, double* flops) {
    MVE_CHECK(handle && B > 0, MVE_ERR_ARG, "dpt_plan: bad arguments");
    Unet* u;
    const int rc = as_engine(handle, "dpt_plan", {Kind::Dpt}, u);
    if (rc) return rc;
    PlanKey k;
    k.B = B; k.H = k.W = u->cfg.dp_image; k.io_dtype = u->cfg.dtype;
    return plan_and_report(*u, k, workspace_bytes, n_ops, flops);
}

int mve_dpt_forward(void* handle, const void* d_pixels, int B, void* d_out, void* const* d_taps, void* d_workspace, size_t workspace_bytes, float* op_ms,
                    void* stream) {
    Unet* u;
    const Plan* pl;
    const int rc = begin_forward(handle, "dpt_forward", {Kind::Dpt}, [&](const Unet& e, PlanKey& k) -> int {
        MVE_CHECK(d_pixels && d_out, MVE_ERR_ARG, "dpt_forward: null pointer (d_pixels / d_out)");
        MVE_CHECK(B > 0, MVE_ERR_ARG, "dpt_forward: bad B %d", B);
        MVE_CHECK(((uintptr_t)d_pixels & 15) == 0 && ((uintptr_t)d_out & 15) == 0, MVE_ERR_ARG, "dpt_forward: d_pixels / d_out must be 16-byte aligned");
        k.B = B; k.H = k.W = e.cfg.dp_image; k.io_dtype = e.cfg.dtype;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, pl);
    if (rc) return rc;
    std::vector<void*> taps(DPT_TAPS, nullptr);
    if (d_taps)
        for (int i = 0; i < DPT_TAPS; ++i) taps[i] = d_taps[i];      // a null entry: that tap is not wanted
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_pixels; r.out = d_out;
    r.cn_out = taps.data();
    return run_plan_ops(*pl, r, 0, pl->ops.size(), op_ms);
}

int mve_loftr_create(void** handle, int dtype) {
    MVE_CHECK(handle, MVE_ERR_ARG, "loftr_create: null handle");
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "loftr_create: dtype must be f16 or bf16");
    Unet* u = new Unet();
    Config& c = u->cfg;
    c.kind = Kind::Loftr;
    c.dtype = dtype; c.in_ch = 1; c.out_ch = 1; c.n_levels = 1; c.layers_per_block = 8;
    c.ctx_dim = 8; c.groups = 1; c.eps = 1e-5f; c.linear_proj = 0;
    c.ch[0] = 256; c.attn[0] = 0; c.heads[0] = 8; c.tlayers[0] = 0;
    layout_params(*u);
    *handle = u;
    return MVE_OK;
}

static int loftr_check_shape(const char* who, int phase, int N, int H, int W) {
    MVE_CHECK(phase == 1 || phase == 2, MVE_ERR_ARG, "%s: phase %d (1 = coarse, 2 = fine)", who, phase);
    MVE_CHECK(N >= 1 && N <= 4096, MVE_ERR_ARG, "%s: bad N %d", who, N);
    MVE_CHECK(H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && H <= 2048 && W <= 2048, MVE_ERR_ARG,
              "%s: H %d / W %d must be multiples of 8 in [8, 2048] (the position table is 256 x 256 coarse cells)", who, H, W);
    return MVE_OK;
}

int mve_loftr_plan(void* handle, int phase, int N, int H, int W, size_t* workspace_bytes, int* n_ops, double* flops) {
    Unet* u;
    int rc = as_engine(handle, "loftr_plan", {Kind::Loftr}, u);
    if (rc) return rc;
    rc = loftr_check_shape("loftr_plan", phase, N, H, W);
    if (rc) return rc;
    PlanKey k;
    k.B = N; k.H = H; k.W = W; k.n_img = phase; k.io_dtype = u->cfg.dtype;
    return plan_and_report(*u, k, workspace_bytes, n_ops, flops);
}

static int loftr_run(void* handle, const char* who, int phase, int N, int H, int W, const void* d_images, const float* d_pos, int M, float thr, int border, void* const* d_io,
                     void* const* d_taps, int n_taps, void* d_workspace, size_t workspace_bytes, float* op_ms, void* stream) {
    Unet* u;
    const Plan* pl;
    const int rc = begin_forward(handle, who, {Kind::Loftr}, [&](const Unet& e, PlanKey& k) -> int {
        MVE_CHECK(d_io, MVE_ERR_ARG, "%s: null pointer (d_io)", who);
        for (int i = 0; i < LOFTR_IO; ++i) {
            const bool used = phase == 1 ? i <= 10 : (i <= 1 || (i >= 4 && i <= 6) || i == 9 || i >= 11);
            MVE_CHECK(!used || (d_io[i] && ((uintptr_t)d_io[i] & 15) == 0), MVE_ERR_ARG, "%s: d_io[%d] is null or not 16-byte aligned", who, i);
        }
        k.B = N; k.H = H; k.W = W; k.n_img = phase; k.io_dtype = e.cfg.dtype;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, pl);
    if (rc) return rc;
    std::vector<void*> ptrs(LOFTR_IO + LOFTR_TAPS_COARSE, nullptr);
    for (int i = 0; i < LOFTR_IO; ++i) ptrs[i] = d_io[i];
    if (d_taps)
        for (int i = 0; i < n_taps; ++i) ptrs[LOFTR_IO + i] = d_taps[i];      // a null entry: that tap is not wanted
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_images; r.ctx = d_pos;
    r.cn_out = ptrs.data();
    r.loftr_M = M; r.loftr_thr = thr; r.loftr_border = border;
    return run_plan_ops(*pl, r, 0, pl->ops.size(), op_ms);
}

int mve_loftr_forward_coarse(void* handle, const void* d_images, const float* d_pos, int N, int H, int W, float thr, int border, void* const* d_io, void* const* d_taps,
                             void* d_workspace, size_t workspace_bytes, float* op_ms, void* stream) {
    Unet* u;
    int rc = as_engine(handle, "loftr_forward_coarse", {Kind::Loftr}, u);
    if (rc) return rc;
    rc = loftr_check_shape("loftr_forward_coarse", 1, N, H, W);
    if (rc) return rc;
    MVE_CHECK(d_images && d_pos && ((uintptr_t)d_images & 15) == 0 && ((uintptr_t)d_pos & 15) == 0, MVE_ERR_ARG, "loftr_forward_coarse: d_images / d_pos null or not 16-byte aligned");
    return loftr_run(handle, "loftr_forward_coarse", 1, N, H, W, d_images, d_pos, 0, thr, border, d_io, d_taps, LOFTR_TAPS_COARSE, d_workspace, workspace_bytes, op_ms, stream);
}

int mve_loftr_forward_fine(void* handle, int N, int H, int W, int M, void* const* d_io, void* const* d_taps, void* d_workspace, size_t workspace_bytes, float* op_ms,
                           void* stream) {
    Unet* u;
    int rc = as_engine(handle, "loftr_forward_fine", {Kind::Loftr}, u);
    if (rc) return rc;
    rc = loftr_check_shape("loftr_forward_fine", 2, N, H, W);
    if (rc) return rc;
    MVE_CHECK(M >= 1 && (long long)M <= (long long)N * (H / 8) * (W / 8), MVE_ERR_ARG, "loftr_forward_fine: M %d must be in [1, N * L = %lld] (no fine call for an empty match set)", M,
              (long long)N * (H / 8) * (W / 8));
    return loftr_run(handle, "loftr_forward_fine", 2, N, H, W, nullptr, nullptr, M, 0.f, 0, d_io, d_taps, LOFTR_TAPS_FINE, d_workspace, workspace_bytes, op_ms, stream);
}

int mve_loftr_destroy(void* handle) { return mve_unet_destroy(handle); }

int mve_sam_encoder_create(void** handle, int dtype, int image_size, int patch_size, int hidden_size, int num_layers, int num_heads, int mlp_dim, int window_size,
                           const int* global_attn_indexes, int n_global, int output_channels, float layer_norm_eps, int use_rel_pos, int use_abs_pos) {
    MVE_CHECK(handle, MVE_ERR_ARG, "sam_encoder_create: null handle");
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "sam_encoder_create: dtype must be f16 or bf16");
    MVE_CHECK(image_size >= 1 && patch_size >= 1 && patch_size <= image_size && image_size <= 4096, MVE_ERR_ARG, "sam_encoder_create: bad image_size %d / patch_size %d",
              image_size, patch_size);
    MVE_CHECK(image_size % patch_size == 0, MVE_ERR_ARG, "sam_encoder_create: image_size %d must be a multiple of patch_size %d", image_size, patch_size);
    const int G = image_size / patch_size;
    MVE_CHECK(G <= 64, MVE_ERR_ARG, "sam_encoder_create: image_size / patch_size = %d exceeds the 64 x 64 grid of mve_attention_relpos", G);
    MVE_CHECK(num_layers >= 1 && num_layers <= 64 && num_heads >= 1, MVE_ERR_ARG, "sam_encoder_create: bad num_layers %d (1..64) / num_heads %d", num_layers, num_heads);
    MVE_CHECK(hidden_size == num_heads * 64 || hidden_size == num_heads * 80, MVE_ERR_ARG,
              "sam_encoder_create: hidden_size %d / num_heads %d: head_dim must be 64 or 80", hidden_size, num_heads);
    MVE_CHECK(hidden_size <= 2048, MVE_ERR_ARG, "sam_encoder_create: hidden_size %d exceeds the 2048 channels of mve_layernorm", hidden_size);
    MVE_CHECK(mlp_dim >= 8 && mlp_dim % 8 == 0, MVE_ERR_ARG, "sam_encoder_create: mlp_dim %d must be a multiple of 8", mlp_dim);
    MVE_CHECK(window_size >= 1 && window_size <= G, MVE_ERR_ARG, "sam_encoder_create: window_size %d must be in [1, %d] (the grid)", window_size, G);
    MVE_CHECK(n_global >= 0 && (n_global == 0 || global_attn_indexes), MVE_ERR_ARG, "sam_encoder_create: bad global_attn_indexes (n_global %d)", n_global);
    MVE_CHECK(output_channels >= 8 && output_channels % 8 == 0 && output_channels <= 2048, MVE_ERR_ARG,
              "sam_encoder_create: output_channels %d must be a multiple of 8 (GEMM / conv rows), at most the 2048 channels of mve_layernorm", output_channels);
    MVE_CHECK(layer_norm_eps > 0.f, MVE_ERR_ARG, "sam_encoder_create: layer_norm_eps must be positive");
    MVE_CHECK(use_rel_pos, MVE_ERR_ARG, "sam_encoder_create: use_rel_pos = 0 is not implemented (the attention kernel always adds the decomposed bias)");
    MVE_CHECK(use_abs_pos, MVE_ERR_ARG, "sam_encoder_create: use_abs_pos = 0 is not implemented (the plan always adds pos_embed)");
    unsigned long long mask = 0;
    for (int i = 0; i < n_global; ++i) {
        MVE_CHECK(global_attn_indexes[i] >= 0 && global_attn_indexes[i] < num_layers, MVE_ERR_ARG, "sam_encoder_create: global_attn_indexes[%d] = %d is not a block index below %d",
                  i, global_attn_indexes[i], num_layers);
        mask |= 1ull << global_attn_indexes[i];
    }
    Unet* u = new Unet();
    Config& c = u->cfg;
    c.kind = Kind::Sam; c.sm_image = image_size; c.sm_patch = patch_size; c.sm_window = window_size; c.sm_out = output_channels; c.sm_global = mask;
    c.clip_inter = mlp_dim; c.clip_act = MVE_ACT_GELU;
    c.dtype = dtype; c.in_ch = 3; c.out_ch = 1; c.n_levels = 1; c.layers_per_block = num_layers;
    c.ctx_dim = 8; c.groups = 1; c.eps = layer_norm_eps; c.linear_proj = 0;
    c.ch[0] = hidden_size; c.attn[0] = 0; c.heads[0] = num_heads; c.tlayers[0] = 0;
    layout_params(*u);
    *handle = u;
    return MVE_OK;
}

int mve_sam_encoder_plan(void* handle, int B, size_t* workspace_bytes, int* n_ops, double* flops) {
    MVE_CHECK(handle && B > 0, MVE_ERR_ARG, "sam_encoder_plan: bad arguments");
    Unet* u;
    const int rc = as_engine(handle, "sam_encoder_plan", {Kind::Sam}, u);
    if (rc) return rc;
    PlanKey k;
    k.B = B; k.H = k.W = u->cfg.sm_image; k.io_dtype = u->cfg.dtype;
    return plan_and_report(*u, k, workspace_bytes, n_ops, flops);
}

int mve_sam_encoder_forward(void* handle, const void* d_pixels, int B, void* d_out, void* const* d_hidden_states, void* d_workspace, size_t workspace_bytes,
                            float* op_ms, void* stream) {
    Unet* u;
    const Plan* pl;
    const int rc = begin_forward(handle, "sam_encoder_forward", {Kind::Sam}, [&](const Unet& e, PlanKey& k) -> int {
        MVE_CHECK(d_pixels && d_out, MVE_ERR_ARG, "sam_encoder_forward: null pointer (d_pixels / d_out)");
        MVE_CHECK(B > 0, MVE_ERR_ARG, "sam_encoder_forward: bad B %d", B);
        MVE_CHECK(((uintptr_t)d_pixels & 15) == 0 && ((uintptr_t)d_out & 15) == 0, MVE_ERR_ARG, "sam_encoder_forward: d_pixels / d_out must be 16-byte aligned");
        k.B = B; k.H = k.W = e.cfg.sm_image; k.io_dtype = e.cfg.dtype;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, pl);
    if (rc) return rc;
    const int n_hidden = u->cfg.layers_per_block + 1;
    std::vector<void*> taps(n_hidden, nullptr);
    if (d_hidden_states)
        for (int i = 0; i < n_hidden; ++i) {
            MVE_CHECK(d_hidden_states[i], MVE_ERR_ARG, "sam_encoder_forward: null d_hidden_states[%d]", i);
            taps[i] = d_hidden_states[i];
        }
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_pixels; r.out = d_out;
    r.cn_out = taps.data();
    return run_plan_ops(*pl, r, 0, pl->ops.size(), op_ms);
}

int mve_sam_encoder_destroy(void* handle) { return mve_unet_destroy(handle); }

int mve_sam_decoder_create(void** handle, int dtype, int hidden_size, int num_layers, int num_heads, int mlp_dim, int num_mask_tokens, int iou_head_hidden_dim,
                           int iou_head_depth, int attention_downsample_rate, int grid, int image_size, float layer_norm_eps, float final_layer_norm_eps) {
    MVE_CHECK(handle, MVE_ERR_ARG, "sam_decoder_create: null handle");
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "sam_decoder_create: dtype (of the image embedding) must be f16 or bf16");
    MVE_CHECK(attention_downsample_rate == 2, MVE_ERR_ARG, "sam_decoder_create: attention_downsample_rate %d is not implemented (2: the cross-attentions run at head_dim 16)",
              attention_downsample_rate);
    MVE_CHECK(hidden_size >= 8 && hidden_size % 8 == 0 && hidden_size <= 512, MVE_ERR_ARG, "sam_decoder_create: hidden_size %d must be a multiple of 8, at most 512", hidden_size);
    MVE_CHECK(num_heads >= 1 && hidden_size == num_heads * 32, MVE_ERR_ARG,
              "sam_decoder_create: hidden_size %d / num_heads %d: the head dims must be 32 (self-attention) and 16 (cross-attention)", hidden_size, num_heads);
    MVE_CHECK(num_layers >= 1 && num_layers <= 8, MVE_ERR_ARG, "sam_decoder_create: bad num_layers %d (1..8)", num_layers);
    MVE_CHECK(mlp_dim >= 1, MVE_ERR_ARG, "sam_decoder_create: bad mlp_dim %d", mlp_dim);
    MVE_CHECK(num_mask_tokens >= 1 && num_mask_tokens <= 8 && num_mask_tokens <= hidden_size / 8, MVE_ERR_ARG, "sam_decoder_create: num_mask_tokens %d must be in [1, 8]", num_mask_tokens);
    MVE_CHECK(iou_head_depth == 3 && iou_head_hidden_dim == hidden_size, MVE_ERR_ARG,
              "sam_decoder_create: iou head of depth %d / width %d: mve_sam_token_mlps runs it next to the hypernetwork MLPs (depth 3, width hidden_size)", iou_head_depth,
              iou_head_hidden_dim);
    MVE_CHECK(grid >= 1 && grid <= 128 && image_size >= 1, MVE_ERR_ARG, "sam_decoder_create: bad grid %d (1..128) / image_size %d", grid, image_size);
    MVE_CHECK(layer_norm_eps > 0.f && final_layer_norm_eps > 0.f, MVE_ERR_ARG, "sam_decoder_create: the LayerNorm eps values must be positive");
    Unet* u = new Unet();
    Config& c = u->cfg;
    c.kind = Kind::SamDecoder; c.sd_grid = grid; c.sd_image = image_size; c.sd_masks = num_mask_tokens; c.sd_eps_final = final_layer_norm_eps;
    c.clip_inter = mlp_dim;
    c.dtype = dtype; c.in_ch = 1; c.out_ch = 1; c.n_levels = 1; c.layers_per_block = num_layers;
    c.ctx_dim = 8; c.groups = 1; c.eps = layer_norm_eps; c.linear_proj = 0;
    c.ch[0] = hidden_size; c.attn[0] = 0; c.heads[0] = num_heads; c.tlayers[0] = 0;
    layout_params(*u);
    *handle = u;
    return MVE_OK;
}

int mve_sam_decoder_finalize(void* handle, void* stream) {
    Unet* u;
    const int rc = as_engine(handle, "sam_decoder_finalize", {Kind::SamDecoder}, u);
    if (rc) return rc;
    char first[256];
    const int miss = mve_unet_missing_params(handle, first, sizeof(first));
    MVE_CHECK(miss == 0 && u->slab, MVE_ERR_STATE, "sam_decoder_finalize: %d parameters not loaded (first: %s)", miss, first);
    const int rc2 = mve_sam_dense_pe((const float*)(u->slab + u->params["gaussian"].off), (float*)(u->slab + u->params["dense_pe"].off), u->cfg.sd_grid, u->cfg.ch[0], stream);
    if (rc2) return rc2;
    u->sd_pe_ready = true;
    return MVE_OK;
}

static int sam_decoder_check(const char* who, int B, int P, int n_points, int has_box) {
    MVE_CHECK(B >= 1 && P >= 1 && (long long)B * P <= 128, MVE_ERR_ARG, "%s: bad B %d / P %d (at most 128 items)", who, B, P);
    MVE_CHECK(n_points >= 0 && n_points <= 16 && (has_box == 0 || has_box == 1), MVE_ERR_ARG, "%s: bad n_points %d / has_box %d", who, n_points, has_box);
    return MVE_OK;
}

int mve_sam_decoder_plan(void* handle, int B, int P, int n_points, int has_box, size_t* workspace_bytes, int* n_ops, double* flops) {
    Unet* u;
    int rc = as_engine(handle, "sam_decoder_plan", {Kind::SamDecoder}, u);
    if (rc) return rc;
    rc = sam_decoder_check("sam_decoder_plan", B, P, n_points, has_box);
    if (rc) return rc;
    PlanKey k;
    k.B = B * P; k.H = P; k.W = n_points; k.has_res = has_box; k.io_dtype = u->cfg.dtype;
    return plan_and_report(*u, k, workspace_bytes, n_ops, flops);
}

int mve_sam_decoder_forward(void* handle, const void* d_embedding, int B, int P, const float* d_boxes, const float* d_points, const int32_t* d_labels, int n_points,
                            float* d_low_res, float* d_iou, void* const* d_taps, void* d_workspace, size_t workspace_bytes, float* op_ms, void* stream) {
    Unet* u;
    const Plan* pl;
    const int rc = begin_forward(handle, "sam_decoder_forward", {Kind::SamDecoder}, [&](const Unet& e, PlanKey& k) -> int {
        MVE_CHECK(e.sd_pe_ready, MVE_ERR_STATE, "sam_decoder_forward: mve_sam_decoder_finalize has not run since the parameters were loaded");
        MVE_CHECK(d_embedding && d_low_res && d_iou, MVE_ERR_ARG, "sam_decoder_forward: null pointer (d_embedding / d_low_res / d_iou)");
        MVE_CHECK(n_points == 0 || (d_points && d_labels), MVE_ERR_ARG, "sam_decoder_forward: %d points without d_points / d_labels", n_points);
        MVE_CHECK(n_points > 0 || (!d_points && !d_labels), MVE_ERR_ARG, "sam_decoder_forward: d_points / d_labels given with n_points 0");
        const int rc2 = sam_decoder_check("sam_decoder_forward", B, P, n_points, d_boxes ? 1 : 0);
        if (rc2) return rc2;
        k.B = B * P; k.H = P; k.W = n_points; k.has_res = d_boxes ? 1 : 0; k.io_dtype = e.cfg.dtype;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, pl);
    if (rc) return rc;
    const int n_taps = 2 * u->cfg.layers_per_block + 5;
    std::vector<void*> ptrs(1 + n_taps, nullptr);
    ptrs[0] = d_iou;
    if (d_taps)
        for (int i = 0; i < n_taps; ++i) ptrs[1 + i] = d_taps[i];      // a null entry: that tap is not wanted
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_embedding; r.out = d_low_res;
    r.sd_boxes = d_boxes; r.sd_points = d_points; r.sd_labels = d_labels;
    r.cn_out = ptrs.data();
    return run_plan_ops(*pl, r, 0, pl->ops.size(), op_ms);
}

int mve_sam_decoder_destroy(void* handle) { return mve_unet_destroy(handle); }

int mve_lpips_create(void** handle, int dtype, int normalize_inputs) {
    MVE_CHECK(handle, MVE_ERR_ARG, "lpips_create: null handle");
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "lpips_create: dtype must be f16 or bf16");
    Unet* u = new Unet();
    Config& c = u->cfg;
    c.kind = Kind::Lpips; c.lpips_normalize = normalize_inputs ? 1 : 0;
    c.dtype = dtype; c.in_ch = 3; c.out_ch = 3; c.n_levels = 1; c.layers_per_block = 1;
    c.ctx_dim = 8; c.groups = 1; c.eps = 0.f; c.linear_proj = 0;
    c.ch[0] = 64; c.attn[0] = 0; c.heads[0] = 1; c.tlayers[0] = 0;
    layout_params(*u);
    *handle = u;
    return MVE_OK;
}

int mve_lpips_plan(void* handle, int B, int H, int W, int io_dtype, size_t* workspace_bytes, int* n_ops, int* n_forward_ops, double* flops) {
    MVE_CHECK(handle && B > 0 && H > 0 && W > 0, MVE_ERR_ARG, "lpips_plan: bad arguments");
    Unet* u;
    int rc = as_engine(handle, "lpips_plan", {Kind::Lpips}, u);
    if (rc) return rc;
    PlanKey k;
    k.B = B; k.H = H; k.W = W; k.io_dtype = io_dtype;
    rc = plan_and_report(*u, k, workspace_bytes, n_ops, flops);
    if (rc) return rc;
    if (n_forward_ops) *n_forward_ops = (int)u->cur->enc_end;
    return MVE_OK;
}

// phase 1: loss[n] = LPIPS(pred[n], target[n]);  phase 2: grad_pred = d (sum_n grad_loss[n] * loss[n]) / d pred.  Phase 2 reads the
// activations phase 1 left in d_workspace: same workspace, same (B, H, W), no other call on it in between.
static int lpips_run(void* handle, int phase, const void* d_pred, const void* d_target, const float* d_grad_loss, int io_dtype, int B, int H,
                     int W, void* d_out, void* d_workspace, size_t workspace_bytes, void* stream) {
    Unet* u;
    const Plan* pl;
    const int rc = begin_forward(handle, "lpips", {Kind::Lpips}, [&](const Unet&, PlanKey& k) -> int {
        MVE_CHECK(d_out && (phase == 2 ? d_grad_loss != nullptr : (d_pred && d_target)), MVE_ERR_ARG, "lpips: null pointer");
        k.B = B; k.H = H; k.W = W; k.io_dtype = io_dtype;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, pl);
    if (rc) return rc;
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_pred; r.timesteps = d_grad_loss; r.ctx = d_target; r.out = d_out;
    return run_plan_ops(*pl, r, phase == 2 ? pl->enc_end : 0, phase == 1 ? pl->enc_end : pl->ops.size(), nullptr);
}

int mve_lpips_forward(void* handle, const void* d_pred, const void* d_target, int io_dtype, int B, int H, int W, float* d_loss,
                      void* d_workspace, size_t workspace_bytes, void* stream) {
    return lpips_run(handle, 1, d_pred, d_target, nullptr, io_dtype, B, H, W, d_loss, d_workspace, workspace_bytes, stream);
}

int mve_lpips_backward(void* handle, const float* d_grad_loss, int io_dtype, int B, int H, int W, void* d_grad_pred, void* d_workspace,
                       size_t workspace_bytes, void* stream) {
    return lpips_run(handle, 2, nullptr, nullptr, d_grad_loss, io_dtype, B, H, W, d_grad_pred, d_workspace, workspace_bytes, stream);
}

int mve_unet_tune(int fuse_shortcut) {
    const int old = g_fuse_shortcut;
    if (fuse_shortcut >= 0) g_fuse_shortcut = fuse_shortcut ? 1 : 0;
    return old;
}

int mve_unet_destroy(void* handle) {
    if (!handle) return MVE_OK;
    Unet* u = (Unet*)handle;
    for (auto& g : u->graphs) { if (g.exec) (void)hipGraphExecDestroy(g.exec); if (g.graph) (void)hipGraphDestroy(g.graph); }
    if (u->slab) (void)hipFree(u->slab);
    delete u;
    return MVE_OK;
}

size_t mve_unet_weight_bytes(void* handle) { return handle ? ((Unet*)handle)->slab_bytes : 0; }

int mve_unet_load_param(void* handle, const char* name, const void* d_src, int src_dtype, int ndim, const long long* shape,
                        void* stream) {
    MVE_CHECK(handle && name && d_src && shape && ndim >= 1 && ndim <= 4, MVE_ERR_ARG, "unet_load_param: bad arguments");
    Unet* u = (Unet*)handle;
    std::string nm = name;
    if (u->cfg.kind == Kind::Lpips && nm.compare(0, 5, "lins.") == 0) nm = "lin" + nm.substr(5);      // nn.ModuleList alias of lin0..lin4
    if (u->cfg.is_vae()) {     // AutoencoderKL state-dict names -> the half's own
        const bool dec = u->cfg.kind == Kind::VaeDecoder;
        const std::string own = dec ? "decoder." : "encoder.", pq = dec ? "post_quant_conv." : "quant_conv.";
        if (nm.compare(0, own.size(), own) == 0) nm = nm.substr(own.size());
        else if (nm.compare(0, pq.size(), pq) == 0) nm = "pq_conv." + nm.substr(pq.size());
        else {
            mve_set_error("vae_load_param: %s does not belong to the %s", name, dec ? "decoder" : "encoder");
            return MVE_ERR_ARG;
        }
    }
    return load_param(*u, nm, d_src, src_dtype, ndim, shape, (hipStream_t)stream);
}

int mve_unet_missing_params(void* handle, char* buf, int buf_len) {
    MVE_CHECK(handle, MVE_ERR_ARG, "unet_missing_params: null handle");
    Unet* u = (Unet*)handle;
    int missing = 0;
    std::string first;
    for (auto& n : u->expected)
        if (!u->loaded.count(n)) { if (!missing) first = n; ++missing; }
    if (buf && buf_len > 0) { strncpy(buf, first.c_str(), (size_t)buf_len - 1); buf[buf_len - 1] = 0; }
    return missing;
}

int mve_unet_plan(void* handle, int B, int H, int W, int ctx_len, int num_cross_attn_imgs, int has_residuals, int io_dtype,
                  int residuals_nhwc, size_t* workspace_bytes, int* n_ops, double* flops /* [5]: conv, linear, attention, norm, other */) {
    MVE_CHECK(handle && B > 0 && H > 0 && W > 0 && ctx_len > 0 && num_cross_attn_imgs >= 1, MVE_ERR_ARG, "unet_plan: bad arguments");
    Unet* u;
    const int rc = as_engine(handle, "unet_plan", {Kind::UNet, Kind::ControlNet}, u);
    if (rc) return rc;
    PlanKey k;
    k.B = B; k.H = H; k.W = W; k.n_img = num_cross_attn_imgs; k.has_res = has_residuals; k.io_dtype = io_dtype; k.res_nhwc = residuals_nhwc; k.ctx_len = ctx_len;
    return plan_and_report(*u, k, workspace_bytes, n_ops, flops);
}

int mve_unet_forward(void* handle, int phase, const void* d_sample, int io_dtype, const float* d_timesteps, const void* d_ctx,
                     int B, int H, int W, int ctx_len, int num_cross_attn_imgs, const void* const* down_residuals,
                     const void* d_mid_residual, int residuals_nhwc, void* d_out, void* d_workspace, size_t workspace_bytes,
                     float* op_ms /* optional host array [n_ops]: per-op milliseconds (synchronises) */, void* stream) {
    const int has_res = (down_residuals && d_mid_residual) ? 1 : 0;
    Unet* u;
    const Plan* plan;
    int rc = begin_forward(handle, "unet_forward", {Kind::UNet}, [&](const Unet&, PlanKey& k) -> int {
        k.B = B; k.H = H; k.W = W; k.n_img = num_cross_attn_imgs; k.has_res = has_res; k.io_dtype = io_dtype; k.res_nhwc = residuals_nhwc; k.ctx_len = ctx_len;
        return MVE_OK;
    }, d_workspace, workspace_bytes, u, plan);
    if (rc) return rc;
    const Plan& pl = *plan;
    MVE_CHECK(d_timesteps && d_ctx && (phase == 1 || d_out) && (phase == 2 || d_sample), MVE_ERR_ARG, "unet_forward: null pointer");
    Run r = new_run(*u, d_workspace, stream);
    r.sample = d_sample; r.timesteps = d_timesteps; r.ctx = d_ctx; r.out = d_out;
    r.down_res = down_residuals; r.mid_res = d_mid_residual;
    r.ref_store = u->ref_store;
    MVE_CHECK(pl.ref_store_bytes == 0 || (u->ref_store && u->ref_store_bytes >= pl.ref_store_bytes), MVE_ERR_NOMEM,
              "unet_forward: reference store %zu < required %zu bytes", u->ref_store_bytes, pl.ref_store_bytes);
    if (phase != 2) {      // unet_dec reuses the emb of its unet_enc state
        rc = take_added_cond(*u, B, r, "unet_forward");
        if (rc) return rc;
        u->cfg_flag = pl.cfg_prefix ? reinterpret_cast<const int*>(r.ws + pl.cfg_flag_off) : nullptr;
        u->cfg_stream = r.stream;
    }
    const size_t lo = phase == 2 ? pl.enc_end : 0, hi = phase == 1 ? pl.enc_end : pl.ops.size();
    if (u->graph_mode && !op_ms) {
        // hipGraph replay (opt-in): identical plan + pointers as an earlier call -> capture on the second sighting, replay afterwards
        MVE_CHECK(stream != nullptr, MVE_ERR_ARG,
                  "unet_forward: hipGraph replay cannot capture the legacy default stream -- run under a non-default stream (torch.cuda.stream(...))");
        std::vector<const void*> key = {d_sample, d_timesteps, d_ctx, d_out, d_workspace, d_mid_residual, u->ref_store, stream};
        if (has_res) for (int i = 0; i < u->cfg.n_levels * (u->cfg.layers_per_block + 1); ++i) key.push_back(down_residuals[i]);
        if (r.add_text) {      // bound added conditions: addresses and geometry (the graph's kernel arguments hold them)
            key.push_back(r.add_text); key.push_back(r.add_ids);
            key.push_back((const void*)(size_t)(((size_t)r.add_text_dim << 32) | ((size_t)r.add_n_ids << 8) | (size_t)r.add_text_dtype));
        }
        Unet::GraphEntry* ge = nullptr;
        for (auto& g : u->graphs)
            if (g.plan_uid == pl.uid && g.phase == phase && g.ptrs == key) { ge = &g; break; }
        if (ge && ge->exec) {
            ge->last_use = u->tick;
            MVE_HIP(hipGraphLaunch(ge->exec, r.stream));
            return MVE_OK;
        }
        if (ge) {           // second sighting: capture, instantiate, launch
            MVE_HIP(hipStreamBeginCapture(r.stream, hipStreamCaptureModeRelaxed));
            rc = run_plan_ops(pl, r, lo, hi, nullptr);
            hipGraph_t graph = nullptr;
            const hipError_t ce = hipStreamEndCapture(r.stream, &graph);
            if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
            MVE_HIP(ce);
            MVE_HIP(hipGraphInstantiate(&ge->exec, graph, nullptr, nullptr, 0));
            ge->graph = graph;
            ge->last_use = u->tick;
            MVE_HIP(hipGraphLaunch(ge->exec, r.stream));
            return MVE_OK;
        }
        if (u->graphs.size() >= 8) {          // evict the least recently used entry
            size_t lru = 0;
            for (size_t i = 1; i < u->graphs.size(); ++i) if (u->graphs[i].last_use < u->graphs[lru].last_use) lru = i;
            if (u->graphs[lru].exec) (void)hipGraphExecDestroy(u->graphs[lru].exec);
            if (u->graphs[lru].graph) (void)hipGraphDestroy(u->graphs[lru].graph);
            u->graphs.erase(u->graphs.begin() + lru);
        }
        Unet::GraphEntry ne;
        ne.plan_uid = pl.uid; ne.phase = phase; ne.seen = 1; ne.ptrs = key; ne.last_use = u->tick;
        u->graphs.push_back(ne);          // first sighting: run eagerly below (also performs any one-time kernel attribute set-up)
    }
    return run_plan_ops(pl, r, lo, hi, op_ms);
}

int mve_unet_graph(void* handle, int enable) {
    MVE_CHECK(handle, MVE_ERR_ARG, "unet_graph: null handle");
    Unet* u = (Unet*)handle;
    const int old = u->graph_mode ? 1 : 0;
    if (enable >= 0) {
        u->graph_mode = enable != 0;
        if (!u->graph_mode) {
            for (auto& g : u->graphs) { if (g.exec) (void)hipGraphExecDestroy(g.exec); if (g.graph) (void)hipGraphDestroy(g.graph); }
            u->graphs.clear();
        }
    }
    return old;
}

int mve_unet_set_attention(void* handle, int ip_tokens, float ip_scale, int ref_mode, int ref_H, int ref_W, int ref_skip,
                           void* d_ref_store, size_t ref_store_bytes) {
    MVE_CHECK(handle && ip_tokens >= 0 && ref_mode >= 0 && ref_mode <= 2 && ref_skip >= 0, MVE_ERR_ARG, "unet_set_attention: bad arguments");
    Unet* u = (Unet*)handle;
    u->ao.ip_tokens = ip_tokens; u->ao.ip_scale = ip_tokens ? ip_scale : 1.0f;
    u->ao.ref_mode = ref_mode; u->ao.ref_skip = ref_mode ? ref_skip : 0;
    u->ao.ref_H = ref_mode == 2 ? ref_H : 0; u->ao.ref_W = ref_mode == 2 ? ref_W : 0;
    u->ref_store = (unsigned char*)d_ref_store; u->ref_store_bytes = ref_store_bytes;
    return MVE_OK;
}

int mve_unet_set_residual_mode(void* handle, int pair) {
    MVE_CHECK(handle, MVE_ERR_ARG, "unet_set_residual_mode: null handle");
    Unet* u = (Unet*)handle;
    MVE_CHECK(u->cfg.is_denoiser(), MVE_ERR_ARG, "unet_set_residual_mode: a UNet / ControlNet handle is needed");
    const int old = u->ao.residual_pair;
    if (pair >= 0) u->ao.residual_pair = pair ? 1 : 0;     // part of the plan key: plans of either mode stay cached side by side
    return old;
}

int mve_unet_tune_cfg_prefix(void* handle, int on) {
    MVE_CHECK(handle, MVE_ERR_ARG, "unet_tune_cfg_prefix: null handle");
    Unet* u = (Unet*)handle;
    MVE_CHECK(u->cfg.kind == Kind::UNet, MVE_ERR_ARG, "unet_tune_cfg_prefix: a UNet handle is needed");
    const int old = u->ao.cfg_prefix;
    if (on >= 0) u->ao.cfg_prefix = on ? 1 : 0;            // part of the plan key, like the residual mode
    return old;
}

int mve_unet_cfg_prefix_state(void* handle) {
    MVE_CHECK(handle, MVE_ERR_STATE, "unet_cfg_prefix_state: null handle");      // (-1 means "not planned")
    Unet* u = (Unet*)handle;
    if (!u->cfg_flag) return -1;
    int v = 0;
    MVE_HIP(hipStreamSynchronize(u->cfg_stream));
    MVE_HIP(hipMemcpy(&v, u->cfg_flag, sizeof(int), hipMemcpyDeviceToHost));
    return v != 0 ? 1 : 0;
}

int mve_unet_set_addition_embed(void* handle, int addition_type, int addition_time_embed_dim, int projection_input_dim) {
    MVE_CHECK(handle, MVE_ERR_ARG, "unet_set_addition_embed: null handle");
    Unet* u = (Unet*)handle;
    Config& c = u->cfg;
    MVE_CHECK(c.is_denoiser(), MVE_ERR_ARG, "unet_set_addition_embed: a UNet / ControlNet handle is needed");
    MVE_CHECK(addition_type == 0 || addition_type == 1, MVE_ERR_ARG, "unet_set_addition_embed: addition type %d (0 = none, 1 = text_time)", addition_type);
    MVE_CHECK(!u->slab && u->loaded.empty(), MVE_ERR_STATE, "unet_set_addition_embed: parameters are already loaded; declare the embedding right after create");
    MVE_CHECK(!c.add_type, MVE_ERR_STATE, "unet_set_addition_embed: the handle already has an addition embedding");
    if (addition_type == 0) return MVE_OK;
    MVE_CHECK(addition_time_embed_dim > 0 && addition_time_embed_dim % 2 == 0, MVE_ERR_ARG, "unet_set_addition_embed: addition_time_embed_dim %d must be even",
              addition_time_embed_dim);
    MVE_CHECK(projection_input_dim > addition_time_embed_dim && projection_input_dim % 8 == 0, MVE_ERR_ARG,
              "unet_set_addition_embed: projection input width %d must be a multiple of 8 above addition_time_embed_dim", projection_input_dim);
    c.add_type = addition_type; c.add_time_dim = addition_time_embed_dim; c.add_P = projection_input_dim;
    layout_addition_embed(*u);
    return MVE_OK;
}

int mve_unet_bind_added_cond(void* handle, const void* d_text_embeds, int text_dtype, int text_dim, const float* d_time_ids, int n_ids, int B) {
    MVE_CHECK(handle, MVE_ERR_ARG, "unet_bind_added_cond: null handle");
    Unet* u = (Unet*)handle;
    const Config& c = u->cfg;
    MVE_CHECK(c.add_type == 1, MVE_ERR_STATE, "unet_bind_added_cond: the handle has no addition embedding (mve_unet_set_addition_embed)");
    if (!d_text_embeds && !d_time_ids) { u->added = Unet::AddedCond(); return MVE_OK; }
    MVE_CHECK(d_text_embeds && d_time_ids, MVE_ERR_ARG, "unet_bind_added_cond: text_embeds and time_ids come together");
    MVE_CHECK(text_dtype == MVE_F32 || text_dtype == MVE_F16 || text_dtype == MVE_BF16, MVE_ERR_ARG, "unet_bind_added_cond: bad text_embeds dtype %d", text_dtype);
    MVE_CHECK(B > 0 && text_dim > 0 && n_ids > 0, MVE_ERR_ARG, "unet_bind_added_cond: bad shape");
    MVE_CHECK((long long)text_dim + (long long)n_ids * c.add_time_dim == c.add_P, MVE_ERR_ARG,
              "unet_bind_added_cond: text width %d + %d time ids x %d != projection input width %d", text_dim, n_ids, c.add_time_dim, c.add_P);
    u->added.text = d_text_embeds; u->added.ids = d_time_ids; u->added.text_dtype = text_dtype; u->added.text_dim = text_dim;
    u->added.n_ids = n_ids; u->added.B = B;
    return MVE_OK;
}

int mve_controlnet_set_cond_repeat(void* handle, int repeat) {
    MVE_CHECK(handle, MVE_ERR_ARG, "controlnet_set_cond_repeat: null handle");
    Unet* u = (Unet*)handle;
    MVE_CHECK(u->cfg.kind == Kind::ControlNet, MVE_ERR_ARG, "controlnet_set_cond_repeat: a ControlNet handle is needed");
    const int old = u->ao.cn_cond_repeat;
    if (repeat >= 1) u->ao.cn_cond_repeat = repeat;        // part of the plan key
    return old;
}

int mve_unet_set_context_tail(void* handle, int rows) {
    MVE_CHECK(handle, MVE_ERR_ARG, "unet_set_context_tail: null handle");
    Unet* u = (Unet*)handle;
    MVE_CHECK(u->cfg.is_denoiser(), MVE_ERR_ARG, "unet_set_context_tail: a UNet / ControlNet handle is needed");
    const int old = u->ao.ctx_tail;
    if (rows >= 0) u->ao.ctx_tail = rows;                  // part of the plan key (and through the plan's uid of the graph key)
    return old;
}

size_t mve_unet_ref_store_bytes(void* handle, int B, int ref_H, int ref_W, int ref_skip) {
    if (!handle || B <= ref_skip) return 0;
    const Config& c = ((Unet*)handle)->cfg;
    std::vector<ResnetDesc> rs;
    std::vector<XfDesc> xs;
    enumerate(c, rs, xs);
    size_t total = 0;
    for (auto& x : xs) {
        int lvl = 0;
        if (x.name.compare(0, 12, "down_blocks.") == 0) lvl = atoi(x.name.c_str() + 12);
        else if (x.name.compare(0, 10, "up_blocks.") == 0) lvl = c.n_levels - 1 - atoi(x.name.c_str() + 10);
        else lvl = c.n_levels - 1;
        const size_t L = (size_t)(ref_H >> lvl) * (ref_W >> lvl);
        total += (size_t)x.layers * (B - ref_skip) * L * 2 * x.c * 2;
    }
    return total;
}

/* describe op i of the current plan: class (0 conv,1 linear,2 attention,3 norm,4 other), flops, label */
int mve_unet_op_info(void* handle, int i, int* cls, double* flops, char* label, int label_len) {
    MVE_CHECK(handle, MVE_ERR_ARG, "unet_op_info: null handle");
    Unet* u = (Unet*)handle;
    MVE_CHECK(u->cur && i >= 0 && i < (int)u->cur->ops.size(), MVE_ERR_ARG, "unet_op_info: no such op %d", i);
    const Op& o = u->cur->ops[i];
    if (cls) *cls = o.cls;
    if (flops) *flops = o.flops;
    if (label && label_len > 0) { strncpy(label, o.what, (size_t)label_len - 1); label[label_len - 1] = 0; }
    return (i < (int)u->cur->enc_end) ? 1 : 2;   // which phase the op belongs to
}

}  // extern "C"
