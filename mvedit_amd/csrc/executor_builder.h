// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): the plan builder -- workspace arena, op recording, and the blocks shared by the networks (GEMM / conv / norm / attention ops, the prologue / epilogue and small ops every builder uses, the pre-norm encoder layer, ResnetBlock2D, Transformer2DModel).
#pragma once
#include "executor_params.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// CFG prefix kernels (Builder::begin_prefix / end_prefix): the device-side probe and the broadcast of the boundary tensors
// ---------------------------------------------------------------------------------------------------
__global__ void k_cfg_probe_init(int* __restrict__ flag) { *flag = 1; }

// true: bytes [0, half) and [half, 2 half) of x differ somewhere in this thread's share
__device__ __forceinline__ bool cfg_halves_differ(const unsigned char* __restrict__ x, size_t half, size_t t, size_t nt) {
    const unsigned char* y = x + half;
    unsigned d = 0;
    if ((((size_t)x | half) & 15) == 0) {
        const u32x4* X = reinterpret_cast<const u32x4*>(x);
        const u32x4* Y = reinterpret_cast<const u32x4*>(y);
        for (size_t i = t; i < half / 16; i += nt) {
            const u32x4 a = X[i], b = Y[i];
            d |= (a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3]);
        }
    } else {
        for (size_t i = t; i < half; i += nt) d |= (unsigned)(x[i] ^ y[i]);
    }
    return d != 0;
}

// Bitwise comparison of the two halves of `sample` (io dtype) and of the time-embedding projection rows (fp32).  The flag was set to 1 by
// k_cfg_probe_init; every thread that sees a difference stores 0 (all writers store the same value: no ordering is needed).
__global__ __launch_bounds__(256) void k_cfg_probe(const unsigned char* __restrict__ sample, size_t sample_half, const unsigned char* __restrict__ tproj,
                                                   size_t tproj_half, int* __restrict__ flag) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, nt = (size_t)gridDim.x * 256;
    if (cfg_halves_differ(sample, sample_half, t, nt) || cfg_halves_differ(tproj, tproj_half, t, nt)) *flag = 0;
}

// Tensor j = blockIdx.y: bytes [0, half) copied onto [half, 2 half) when the flag is 1 (16-byte aligned; half a multiple of 16)
constexpr int CFG_BCAST_MAX = 8;
struct CfgBcast { unsigned char* p[CFG_BCAST_MAX]; unsigned long long half[CFG_BCAST_MAX]; };

__global__ __launch_bounds__(256) void k_cfg_broadcast(const CfgBcast c, const int* __restrict__ flag) {
    if (__builtin_amdgcn_readfirstlane(*flag) == 0) return;
    const unsigned long long half = c.half[blockIdx.y], n16 = half / 16;
    const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(c.p[blockIdx.y]);
    u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(c.p[blockIdx.y] + half);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (unsigned long long)gridDim.x * 256) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------------
// plan builder
// ---------------------------------------------------------------------------------------------------
struct Builder {
    Unet& u;
    Plan& pl;
    Arena ar;
    const Config& c;
    int B, dt;
    int ld_temb, ld_kv;
    Ref tproj, ctxkv, ipkv;  // hoisted projections
    int ctx_rows_per_img = 0, ctxB = 0;
    int Lt = 0;              // text rows of the context (ctx_rows_per_img - ip_tokens - ctx_tail)
    int H0 = 0;              // latent height of this pass (reference-store geometry)
    size_t ref_off = 0;      // running offset into the reference K/V store

    Builder(Unet& u_, Plan& p) : u(u_), pl(p), c(u_.cfg) {}

    Ref ws(size_t bytes) {
        Ref r; r.kind = Ref::WS; r.off = ar.alloc(bytes);
        if (pfx_on) pfx_live[r.off] = bytes;
        return r;
    }
    // residual_pair mode (AttnOpts::residual_pair): a tensor of the residual stream gets a companion of half its size for its 8-bit low half.  The
    // companion is found through the high half's workspace offset, so the ops below pick it up by themselves: an output with a companion is
    // written as a pair, a residual / normalised input with a companion is read as one.  Everything else -- every MFMA operand read -- sees the
    // high half alone, exactly the tensor of the plain mode.
    std::map<size_t, Ref> lo_of;
    Ref ws_stream(size_t bytes) {
        Ref r = ws(bytes);
        if (pl.ao.residual_pair) lo_of[r.off] = ws(bytes / 2);      // lo8: one byte per 16-bit element (common.h)
        return r;
    }
    Ref lo(const Ref& r) const {
        if (r.kind != Ref::WS) return Ref();
        auto it = lo_of.find(r.off);
        return it == lo_of.end() ? Ref() : it->second;
    }
    void rel(const Ref& r) {
        if (r.kind != Ref::WS) return;
        auto it = lo_of.find(r.off);
        if (it != lo_of.end()) { ar.release(it->second.off); pfx_live.erase(it->second.off); lo_of.erase(it); }
        ar.release(r.off);
        pfx_live.erase(r.off);
    }
    Ref wt(const std::string& n, size_t elem_off = 0) {
        auto it = u.params.find(n);
        Ref r;
        if (it == u.params.end()) { u.err = "missing packed parameter " + n; return r; }
        r.kind = Ref::WT;
        r.off = it->second.off + elem_off * (it->second.f32 ? 4 : 2);
        return r;
    }
    static Ref at(Ref r, size_t bytes) { r.off += bytes; return r; }
    // plan-time guard: every workspace operand of an op must lie inside a block that is allocated right now
    void live(const Ref& r, const char* what) {
        if (r.kind != Ref::WS) return;
        for (auto& blk : ar.b)
            if (!blk.free && r.off >= blk.off && r.off < blk.off + blk.size) return;
        if (u.err.empty()) u.err = std::string("operand used after release in ") + what;
    }
    void op(int cls, double flops, const char* what, std::function<int(const Run&)> fn) {
        pl.ops.push_back({cls, flops, what, std::move(fn)});
        pl.flops[cls] += flops;
    }

    // ---- CFG prefix -------------------------------------------------------------------------------------
    // Under classifier-free guidance the batch is [uncond | text]: both halves carry the same latents and timesteps and differ in the text context
    // alone, so every op in front of the first cross-attention produces bit-identical rows for image b and image b + B / 2.  The ops recorded
    // between begin_prefix() and end_prefix() stay what they are -- one op-list entry each, the launches of the full-batch problem -- but run under
    // the second-half predicate (common.h): their blocks for images [B / 2, B) return at once when the plan's device flag is 1.  The first of them
    // is preceded by the probe that writes the flag (bitwise comparison of the halves of sample and of the time-embedding projection rows, which
    // covers per-image timesteps and added conditions), the last one is followed by the broadcast of the boundary tensors: every tensor allocated
    // inside the prefix that is still live at its end (residual stream, prescaled q of the first cross-attention, skips) gets its first half copied
    // onto its second.  Tensors that die inside the prefix keep a stale second half nobody reads.  Nothing is decided on the host: the flag is
    // re-evaluated by every forward and every graph replay.
    bool pfx_on = false;
    size_t pfx_first = 0;                                       // first op of the prefix
    std::map<size_t, size_t> pfx_live;                          // workspace offset -> bytes of every tensor allocated inside the prefix and not released yet
    std::shared_ptr<size_t> pfx_flag;                           // workspace offset of the flag: known when the arena's peak is (build())
    size_t pfx_sample_half = 0, pfx_tproj_half = 0;
    void begin_prefix(size_t sample_half_bytes, size_t tproj_half_bytes) {
        pfx_on = true;
        pfx_first = pl.ops.size();
        pfx_live.clear();
        pfx_flag = std::make_shared<size_t>(0);
        pfx_sample_half = sample_half_bytes; pfx_tproj_half = tproj_half_bytes;
    }
    void end_prefix() {
        if (!pfx_on) return;
        pfx_on = false;
        const size_t first = pfx_first, end = pl.ops.size();
        if (end == first) return;
        std::vector<std::pair<Ref, size_t>> bt;                 // boundary tensors: (tensor, bytes of one half)
        for (auto& kv : pfx_live) {
            if (kv.second % 32 != 0 && u.err.empty()) u.err = "cfg prefix: a boundary tensor does not split into 16-byte aligned halves";
            Ref r; r.kind = Ref::WS; r.off = kv.first;
            bt.push_back({r, kv.second / 2});
        }
        pfx_live.clear();
        pl.cfg_prefix = true;
        const std::shared_ptr<size_t> fo = pfx_flag;
        const Ref tp = tproj;
        const size_t sh = pfx_sample_half, th = pfx_tproj_half;
        for (size_t i = first; i < end; ++i) {
            const std::function<int(const Run&)> inner = std::move(pl.ops[i].fn);
            const bool is_first = i == first, is_last = i + 1 == end;
            pl.ops[i].fn = [=](const Run& r) -> int {
                int* flag = reinterpret_cast<int*>(r.ws + *fo);
                if (is_first) {
                    const size_t units = (sh > th ? sh : th) / 16 + 1;
                    k_cfg_probe_init<<<1, 1, 0, r.stream>>>(flag);
                    k_cfg_probe<<<units > 64 * 256 ? 64u : mve_cdiv(units, 256), 256, 0, r.stream>>>((const unsigned char*)r.sample, sh, (const unsigned char*)r.p(tp), th, flag);
                    MVE_LAUNCH_CHECK();
                }
                int rc;
                { MveSkipScope scope(flag); rc = inner(r); }
                if (rc || !is_last) return rc;
                for (size_t j = 0; j < bt.size(); j += CFG_BCAST_MAX) {
                    CfgBcast cb;
                    memset(&cb, 0, sizeof(cb));
                    const size_t n = bt.size() - j < (size_t)CFG_BCAST_MAX ? bt.size() - j : (size_t)CFG_BCAST_MAX;
                    size_t most = 0;
                    for (size_t k = 0; k < n; ++k) {
                        cb.p[k] = (unsigned char*)r.p(bt[j + k].first); cb.half[k] = bt[j + k].second;
                        most = bt[j + k].second > most ? bt[j + k].second : most;
                    }
                    const unsigned gx = most / 16 > 2048ull * 256 ? 2048u : mve_cdiv(most / 16 + 1, 256);
                    k_cfg_broadcast<<<dim3(gx, (unsigned)n), 256, 0, r.stream>>>(cb, flag);
                    MVE_LAUNCH_CHECK();
                }
                return (int)MVE_OK;
            };
        }
    }

    int rows_img = 0;        // rows per image of the level being emitted (split-K granularity); 0: never split
    void gemm(Ref A, int lda, Ref W, int ldw, Ref out, int ldc, int M, int N, int K, Ref bias, Ref rowvec, int ldrv,
              int rpv, Ref res, int ldr, int flags, const char* what, float out_scale = 1.0f) {
        const int rimg = rows_img;
        const int d = dt;
        live(A, what); live(out, what); live(res, what); live(rowvec, what);
        const size_t skb = mve_gemm_workspace_bytes(M, N, K, rimg);
        Ref sk = skb ? ws(skb) : Ref();
        const Ref res_lo = lo(res), out_lo = lo(out);
        op(OC_LINEAR, 2.0 * M * N * K, what, [=](const Run& r) {
            return mve_gemm_pair(d, r.p(A), lda, r.p(W), ldw, r.p(out), ldc, M, N, K, (const float*)r.p(bias), (const float*)r.p(rowvec),
                                 ldrv, rpv, r.p(res), ldr, flags, out_scale, r.p(sk), skb, rimg, r.p(res_lo), r.p(out_lo), r.stream);
        });
        rel(sk);
    }
    // GEMM whose output rows go straight into a LayerNorm (BasicTransformerBlock norm1 / norm2 / norm3 behind proj_in / attn1.to_out / attn2.to_out):
    // mve_gemm_pair_ln normalises the rows in the producing tile's epilogue where the launch allows (N = 320 on the pair tile) and runs the LayerNorm
    // kernel behind the GEMM otherwise -- bit-identical either way, so the op list does not depend on the batch.  Counted as one linear op.
    void gemm_ln(Ref A, int lda, Ref W, int ldw, Ref out, int ldc, int M, int N, int K, Ref bias, Ref res, int ldr, Ref ln_out, Ref ln_g, Ref ln_b,
                 const char* what) {
        const int rimg = rows_img;
        const int d = dt;
        live(A, what); live(out, what); live(res, what); live(ln_out, what);
        const size_t skb = mve_gemm_workspace_bytes(M, N, K, rimg);
        Ref sk = skb ? ws(skb) : Ref();
        const Ref res_lo = lo(res), out_lo = lo(out);
        op(OC_LINEAR, 2.0 * M * N * K, what, [=](const Run& r) {
            return mve_gemm_pair_ln(d, r.p(A), lda, r.p(W), ldw, r.p(out), ldc, M, N, K, (const float*)r.p(bias), r.p(res), ldr, r.p(sk), skb, rimg,
                                    r.p(res_lo), r.p(out_lo), r.p(ln_out), N, (const float*)r.p(ln_g), (const float*)r.p(ln_b), 1e-5f, r.stream);
        });
        rel(sk);
    }
    void conv(Ref x, int C1, int Bn, int H, int W, int stride, int ups, Ref Wt, int Cout, Ref out, Ref bias, Ref rowvec,
              int ldrv, Ref res, int flags, const char* what) {
        const int d = dt;
        const int Hv = ups ? 2 * H : H, Wv = ups ? 2 * W : W;
        const int Ho = (Hv - 1) / stride + 1, Wo = (Wv - 1) / stride + 1;
        live(x, what); live(out, what); live(res, what); live(rowvec, what);
        const int fl = flags | (C1 % 64 == 0 ? MVE_CONV_W_CHUNK64 : 0);   // must mirror the layout's packing rule (pack_conv)
        const size_t skb = mve_gemm_workspace_bytes(Bn * Ho * Wo, Cout, 9 * C1, Ho * Wo);
        Ref sk = skb ? ws(skb) : Ref();
        const Ref res_lo = lo(res), out_lo = (flags & MVE_GEMM_OUT_F32) ? Ref() : lo(out);
        op(OC_CONV, 2.0 * Bn * Ho * Wo * (double)Cout * 9 * C1, what, [=](const Run& r) {
            return mve_conv3x3_pair(d, r.p(x), C1, nullptr, 0, Bn, H, W, stride, ups, r.p(Wt), Cout, r.p(out), Cout,
                                    (const float*)r.p(bias), (const float*)r.p(rowvec), ldrv, r.p(res), Cout, fl, 1.0f, r.p(sk), skb, r.p(res_lo),
                                    r.p(out_lo), r.stream);
        });
        rel(sk);
    }
    // Upsample2D: nearest 2x + conv 3x3.  Default: four 2 x 2 phase convs over the source (mve_upsample_conv_phases: 4 / 9 of the flops, one extra
    // rounding on the summed weights) wherever the shape allows; the 3 x 3 conv over the virtual upsampled image otherwise and with
    // MVE_UPSAMPLE_PHASES=0.  Round 5: also in residual_pair mode (now the default mode) -- the summed-weight rounding costs the end-to-end error
    // 8.5e-4 -> 8.7e-4 against fp32 (tests/rounding_budget_experiment.py --phase), inside north_star's 1e-3; the pair output needs the 320-wide
    // tile (C % 320 == 0: every UNet width).  The choice depends on the shape and the mode only, except below 64 source pixels per launch (tiny
    // test sizes at batch 1), where the 3 x 3 form runs.
    static bool upsample_phases_on() {
        static int on = -1;
        if (on < 0) { const char* e = getenv("MVE_UPSAMPLE_PHASES"); on = e ? (atoi(e) != 0) : 1; }
        return on != 0;
    }
    void upsample_conv(Ref x, int C, int Bn, int H, int W, const std::string& slot, Ref out) {
        const bool have4 = u.params.count(slot + ".w4") != 0;
        if (!have4 || !upsample_phases_on() || (pl.ao.residual_pair && C % 320 != 0) || !mve_upsample_conv_phases_supported(C, C, Bn, H, W)) {
            conv(x, C, Bn, H, W, 1, 1, wt(slot + ".w"), C, out, wt(slot + ".b"), Ref(), 0, Ref(), 0, "upsample+conv");
            return;
        }
        const int d = dt;
        const char* what = "upsample+conv (4 phases)";
        live(x, what); live(out, what);
        const size_t skb = mve_upsample_conv_phases_workspace_bytes(C, C, Bn, H, W);
        Ref sk = skb ? ws(skb) : Ref();
        const Ref W4 = wt(slot + ".w4"), bias = wt(slot + ".b"), out_lo = lo(out);
        // (flops: the op's ALGORITHMIC count -- the 3 x 3 conv over the upsampled image the reference computes, SURVEY.md 8(d) -- of which this form
        // executes 4 / 9; bench.py reports both)
        op(OC_CONV, 2.0 * Bn * (4.0 * H * W) * (double)C * 9 * C, what, [=](const Run& r) {
            return mve_upsample_conv_phases(d, r.p(x), C, Bn, H, W, r.p(W4), C, r.p(out), (const float*)r.p(bias), 0, r.p(sk), skb, r.p(out_lo), r.stream);
        });
        rel(sk);
    }
    void gn(Ref x1, int C1, Ref x2, int C2, int Bn, int HW, float eps, Ref g, Ref b, int silu, Ref out, const char* what) {
        const int d = dt, G = c.groups;
        const size_t wsb = mve_groupnorm_workspace_bytes(Bn, HW, C1 + C2, G);
        Ref scratch = ws(wsb);
        live(x1, what); live(x2, what); live(out, what);
        const Ref x1_lo = lo(x1), x2_lo = lo(x2);
        op(OC_NORM, 0, what, [=](const Run& r) {
            return mve_groupnorm_silu_pair(d, r.p(x1), C1, r.p(x2), C2, Bn, HW, G, eps, (const float*)r.p(g), (const float*)r.p(b), silu,
                                           r.p(out), r.p(scratch), r.p(x1_lo), r.p(x2_lo), r.stream);
        });
        rel(scratch);
    }
    void ln(Ref x, Ref y, int M, int C, Ref g, Ref b) {
        const int d = dt;
        live(x, "layernorm"); live(y, "layernorm");
        const Ref x_lo = lo(x);
        op(OC_NORM, 0, "layernorm", [=](const Run& r) {
            return mve_layernorm_pair(d, r.p(x), C, r.p(y), C, M, C, (const float*)r.p(g), (const float*)r.p(b), 1e-5f, r.p(x_lo), r.stream);
        });
    }
    // Q as mve_attention_prescaled wants it: the output of a GEMM over a to_q weight slot that carries the softmax scale.  The only way to get one
    // is prescaled(): a caller that projects Q with unfolded weights cannot reach attn() by accident.
    struct PrescaledQ { Ref q; };
    PrescaledQ prescaled(Ref q, const std::string& weight_slot, int hd) {
        auto it = u.params.find(weight_slot);
        const float want = 1.4426950408889634f / sqrtf((float)hd);
        if (it == u.params.end() || !(fabsf(it->second.q_fold - want) <= 1e-6f * want))
            u.err = "attention: Q is not produced by a to_q slot folded with head_dim^-1/2 * log2(e) (" + weight_slot + ")";
        return PrescaledQ{q};
    }
    void attn(PrescaledQ pq, int ldq, Ref k, int ldk, Ref v, int ldv, Ref o, int ldo, int Bn, int Lq, int Lk, int heads, int hd,
              Ref k2 = Ref(), int ldk2 = 0, Ref v2 = Ref(), int ldv2 = 0, int Lk2 = 0, const char* what = "attention") {
        const int d = dt;
        const Ref q = pq.q;
        if (Bn <= 0) return;
        live(q, what); live(k, what); live(v, what); live(o, what);
        op(OC_ATTN, 4.0 * Bn * heads * (double)Lq * (Lk + Lk2) * hd, what, [=](const Run& r) {
            // Q comes out of to_q already multiplied by hd^-1/2 * log2(e) (executor_params.h: q_fold)
            return mve_attention_prescaled(d, r.p(q), ldq, r.p(k), ldk, r.p(v), ldv, r.p(k2), ldk2, r.p(v2), ldv2, r.p(o), ldo, Bn, Lq, Lk, Lk2,
                                           heads, hd, r.stream);
        });
    }
    // device-to-device 2-D copy (rows x width bytes) between pitched buffers
    void copy2d(Ref dst, size_t dpitch, Ref src, size_t spitch, size_t width, size_t rows, const char* what) {
        if (!rows || !width) return;
        live(dst, what); live(src, what);
        op(OC_OTHER, 0, what, [=](const Run& r) {
            return hipMemcpy2DAsync(r.p(dst), dpitch, r.p(src), spitch, width, rows, hipMemcpyDeviceToDevice, r.stream) == hipSuccess
                       ? MVE_OK : MVE_ERR_HIP;
        });
    }

    // ---- pieces shared by the network builders ----------------------------------------------------------------------------------------------------
    // Every op below copies what its closure needs into locals first: the closures outlive the Builder and must not capture `this`.
    // A plan starts with begin() and ends with `return finish(name)`.  finish() leaves alone an enc_end the builder has set itself (UNet, LPIPS).
    void begin(int B_, int H, int W, int n_img, int io_dtype) {
        B = B_; dt = c.dtype;
        pl = Plan();
        pl.B = B_; pl.H = H; pl.W = W; pl.n_img = n_img; pl.io_dtype = io_dtype;
        ld_temb = 0; ld_kv = 0;
        rows_img = 0;
    }
    int finish(const char* name) {
        if (!pl.enc_end) pl.enc_end = pl.ops.size();
        pl.ws_bytes = ar.peak + 256;
        if (!u.err.empty()) { mve_set_error("%s plan: %s", name, u.err.c_str()); u.err.clear(); return MVE_ERR_STATE; }
        return MVE_OK;
    }
    static Ref arg(Ref::Kind kind, int idx = 0) { Ref r; r.kind = kind; r.idx = idx; return r; }      // a tensor of the call (Run::p)
    static Ref cn_out(int idx) { return arg(Ref::CNOUT, idx); }
    // dense linear: out [rows, N] = A [rows, K] . W [N, K]^T (+ bias) (+ res [rows, N]); every leading dimension is the one K and N imply
    void dense(Ref A, Ref W, Ref bias, Ref out, int rows, int N, int K, Ref res, const char* what, int flags = 0) {
        gemm(A, K, W, K, out, N, rows, N, K, bias, Ref(), 0, 0, res, res.kind == Ref::NUL ? 0 : N, flags, what);
    }
    // LayerNorm of `rows` rows of x (pitch ldx) into dense rows of y, with the parameters slot.g / slot.b (plain stream; ln() above is the pair stream's)
    void layernorm(Ref x, int ldx, Ref y, int rows, int C, const std::string& slot, float eps) {
        const int d = dt;
        const Ref g = wt(slot + ".g"), b = wt(slot + ".b");
        live(x, "layernorm"); live(y, "layernorm");
        op(OC_NORM, 0, "layernorm", [=](const Run& r) { return mve_layernorm(d, r.p(x), ldx, r.p(y), C, rows, C, (const float*)r.p(g), (const float*)r.p(b), eps, r.stream); });
    }
    // optional output: x is copied into Run::cn_out[slot] only when the caller gave a tensor for it
    void copy_out(Ref x, size_t bytes, int slot, const char* what) {
        live(x, what);
        op(OC_OTHER, 0, what, [=](const Run& r) {
            void* dst = r.cn_out ? r.cn_out[slot] : nullptr;
            if (!dst) return (int)MVE_OK;
            return hipMemcpyAsync(dst, r.p(x), bytes, hipMemcpyDeviceToDevice, r.stream) == hipSuccess ? (int)MVE_OK : (int)MVE_ERR_HIP;
        });
    }
    void act(Ref x, size_t nel, int selector, const char* what) {      // in place; selector: MVE_ACT_*
        const int d = dt;
        live(x, what);
        op(OC_OTHER, 0, what, [=](const Run& r) { return mve_act(d, selector, r.p(x), r.p(x), nel, r.stream); });
    }
    void add_relu(Ref a, Ref b, Ref y, size_t nel, const char* what) {      // y = max(a + b, 0); b may be null
        const int d = dt;
        live(a, what); live(b, what); live(y, what);
        op(OC_OTHER, 0, what, [=](const Run& r) { return mve_dpt_add_relu(d, r.p(a), r.p(b), r.p(y), nel, r.stream); });
    }
    void relu(Ref x, size_t nel, const char* what) { add_relu(x, Ref(), x, nel, what); }
    // NHWC convolutions into a new buffer: 1 x 1 (a GEMM over the pixels) and 3 x 3 (flags: MVE_CONV_*)
    Ref conv1x1(Ref x, int rows, int Cin, const std::string& w, Ref bias, int Cout, const char* what) {
        Ref y = ws((size_t)rows * Cout * 2);
        dense(x, wt(w), bias, y, rows, Cout, Cin, Ref(), what);
        return y;
    }
    Ref conv3x3(Ref x, int Cin, int Bn, int H, int W, int stride, const std::string& w, Ref bias, int Cout, Ref res, int flags, const char* what) {
        Ref y = ws((size_t)Bn * (H / stride) * (W / stride) * Cout * 2);
        conv(x, Cin, Bn, H, W, stride, 0, wt(w), Cout, y, bias, Ref(), 0, res, flags, what);
        return y;
    }
    Ref upsample2x(Ref x, int Bn, int H, int W, int C, const char* what) {      // bilinear, align_corners -> new buffer
        const int d = dt;
        Ref y = ws((size_t)Bn * 4 * H * W * C * 2);
        live(x, what); live(y, what);
        op(OC_OTHER, 0, what, [=](const Run& r) { return mve_dpt_upsample2x(d, r.p(x), Bn, H, W, C, r.p(y), r.stream); });
        return y;
    }
    Ref gather_s2(Ref x, int Bn, int H, int W, int C) {      // every second pixel of every second row (the input of a strided 1 x 1 shortcut) -> new buffer
        const int d = dt;
        Ref y = ws((size_t)Bn * (H / 2) * (W / 2) * C * 2);
        live(x, "shortcut stride-2 gather"); live(y, "shortcut stride-2 gather");
        op(OC_OTHER, 0, "shortcut stride-2 gather", [=](const Run& r) { return mve_dpt_gather_s2(d, r.p(x), Bn, H, W, C, r.p(y), r.stream); });
        return y;
    }
    // layout ops at the ends of a network: a call tensor (NCHW, io_dtype) into NHWC rows of Cpad channels, and NHWC rows back into Run::out
    void to_nhwc(Ref src, int Bn, int C, int H, int W, int Cpad, Ref dst, const char* what = "nchw->nhwc") {
        const int d = dt, io = pl.io_dtype;
        live(dst, what);
        op(OC_OTHER, 0, what, [=](const Run& r) { return mve_nchw_to_nhwc(d, io, r.p(src), Bn, C, H, W, Cpad, r.p(dst), r.stream); });
    }
    void to_nchw(Ref x, int x_dtype, int ldx, int Bn, int C, int H, int W, const char* what = "nhwc->nchw") {
        const int io = pl.io_dtype;
        const Ref dst = arg(Ref::OUT);
        live(x, what);
        op(OC_OTHER, 0, what, [=](const Run& r) { return mve_nhwc_to_nchw(io, x_dtype, r.p(x), ldx, Bn, C, H, W, r.p(dst), r.stream); });
    }

    // One pre-norm transformer encoder layer over x [M = B * T, C] -> new buffer (x is released): x += out(attention(qkv(norm1(x)))), then
    // x += fc2(act(fc1(norm2(x)))).  The callers differ in the parameter names and two labels (EncoderNames) and in the attention step: causal
    // (CLIP text tower: head_dim 64, scale 1 / 8, mve_attention_causal) or full with head_dim^-1/2.
    struct EncoderNames { const char *n1, *qkv, *o, *n2, *fc1, *fc2, *qkv_what, *o_what; };
    Ref encoder_layer(const EncoderNames& nm, const std::string& p, Ref x, int M, int C, int I, int act_sel, bool causal) {
        const int e = 2, d = dt, Bn = B, T = M / B, heads = c.heads[0], hd = causal ? 64 : C / heads;
        const float eps = c.eps, scale = causal ? 0.125f : 1.0f / sqrtf((float)hd);
        Ref n1 = ws((size_t)M * C * e);
        layernorm(x, C, n1, M, C, p + nm.n1, eps);
        Ref qkv = ws((size_t)M * 3 * C * e);
        dense(n1, wt(p + nm.qkv + ".w"), wt(p + nm.qkv + ".b"), qkv, M, 3 * C, C, Ref(), nm.qkv_what);
        rel(n1);
        Ref a = ws((size_t)M * C * e);
        {
            const Ref q = qkv, kk = at(qkv, (size_t)C * e), v = at(qkv, (size_t)2 * C * e);
            const char* what = causal ? "causal attention" : "attention";
            live(qkv, what); live(a, what);
            op(OC_ATTN, 4.0 * Bn * heads * (double)T * T * hd, what, [=](const Run& r) {
                if (causal) return mve_attention_causal(d, r.p(q), 3 * C, r.p(kk), 3 * C, r.p(v), 3 * C, r.p(a), C, Bn, T, heads, hd, scale, r.stream);
                return mve_attention(d, r.p(q), 3 * C, r.p(kk), 3 * C, r.p(v), 3 * C, nullptr, 0, nullptr, 0, r.p(a), C, Bn, T, T, 0, heads, hd, scale, r.stream);
            });
        }
        rel(qkv);
        Ref x2 = ws((size_t)M * C * e);
        dense(a, wt(p + nm.o + ".w"), wt(p + nm.o + ".b"), x2, M, C, C, x, nm.o_what);
        rel(a); rel(x);
        Ref n2 = ws((size_t)M * C * e);
        layernorm(x2, C, n2, M, C, p + nm.n2, eps);
        Ref f = ws((size_t)M * I * e);
        dense(n2, wt(p + nm.fc1 + ".w"), wt(p + nm.fc1 + ".b"), f, M, I, C, Ref(), "mlp.fc1");
        rel(n2);
        act(f, (size_t)M * I, act_sel, act_sel == MVE_ACT_GELU ? "gelu" : "quick_gelu");
        Ref x3 = ws((size_t)M * C * e);
        dense(f, wt(p + nm.fc2 + ".w"), wt(p + nm.fc2 + ".b"), x3, M, C, I, x2, "mlp.fc2+residual");
        rel(f); rel(x2);
        return x3;
    }

    // ControlNet output k: out_k (+)= conditioning_scale * (W x + b), a 1x1 "zero convolution" (diffusers ControlNetModel
    // controlnet_down_blocks / controlnet_mid_block, then the `* conditioning_scale` and MultiControlNetModel's running sum)
    void zero_conv(Ref x, int C, int M, int hw, const std::string& name, int out_idx) {
        const int d = dt;
        Ref W = wt(name + ".w"), bias = wt(name + ".b");
        Ref out; out.kind = Ref::CNOUT; out.idx = out_idx;
        live(x, "controlnet zero conv");
        const size_t skb = mve_gemm_workspace_bytes(M, C, C, hw);
        Ref sk = skb ? ws(skb) : Ref();
        op(OC_LINEAR, 2.0 * M * (double)C * C, "controlnet zero conv", [=](const Run& r) {
            void* o = r.p(out);
            return mve_gemm(d, r.p(x), C, r.p(W), C, o, C, M, C, C, (const float*)r.p(bias), nullptr, 0, 0, r.cn_accum ? o : nullptr, C,
                            MVE_GEMM_RES_AFTER_SCALE, r.cn_scale, r.p(sk), skb, hw, r.stream);
        });
        rel(sk);
    }

    // ResnetBlock2D.  x [M,C1] (+ skip [M,C2]) -> new buffer [M,Cout]
    Ref resnet(const std::string& name, Ref x, int C1, Ref skip, int C2, int Cout, int H, int W) {
        const int M = B * H * W, Cin = C1 + C2, e = 2;
        rows_img = H * W;
        Ref h0 = ws((size_t)M * Cin * e);
        gn(x, C1, skip, C2, B, H * W, c.eps, wt(name + ".norm1.g"), wt(name + ".norm1.b"), 1, h0, "resnet.norm1+silu");
        Ref h1 = ws((size_t)M * Cout * e);
        Ref tv = c.is_vae() ? Ref() : at(tproj, (size_t)u.temb_off[name] * 4);      // the VAE's resnets have no time embedding
        conv(h0, Cin, B, H, W, 1, 0, wt(name + ".conv1.w"), Cout, h1, wt(name + ".conv1.b"), tv, ld_temb, Ref(), 0, "resnet.conv1");
        rel(h0);
        Ref h2 = ws((size_t)M * Cout * e);
        gn(h1, Cout, Ref(), 0, B, H * W, c.eps, wt(name + ".norm2.g"), wt(name + ".norm2.b"), 1, h2, "resnet.norm2+silu");
        rel(h1);
        if (Cin != Cout && u.fuse_sc) {
            // conv2 and the 1x1 conv_shortcut over [x | skip] share one K loop (mve_conv3x3_shortcut); no shortcut tensor exists
            Ref out = ws_stream((size_t)M * Cout * e);
            const Ref out_lo = lo(out);
            const int d = dt, Bn = B;
            Ref Wt = wt(name + ".conv2.w"), b2 = wt(name + ".conv2.b"), bs = wt(name + ".sc.b");
            live(h2, "resnet.conv2+shortcut"); live(x, "resnet.conv2+shortcut"); live(skip, "resnet.conv2+shortcut");
            const size_t skb = mve_gemm_workspace_bytes(M, Cout, 9 * Cout + Cin, H * W);
            Ref sk = skb ? ws(skb) : Ref();
            op(OC_CONV, 2.0 * M * (double)Cout * (9 * Cout + Cin), "resnet.conv2+shortcut", [=](const Run& r) {
                return mve_conv3x3_shortcut_pair(d, r.p(h2), Cout, r.p(x), C1, r.p(skip), C2, Bn, H, W, r.p(Wt), Cout, r.p(out), Cout,
                                                 (const float*)r.p(b2), (const float*)r.p(bs), 0, 1.0f, r.p(sk), skb, r.p(out_lo), r.stream);
            });
            rel(sk);
            rel(h2);
            return out;
        }
        Ref res = x, sc;
        if (Cin != Cout) {
            sc = ws((size_t)M * Cout * e);
            gemm(x, C1, wt(name + ".sc.w"), Cin, sc, Cout, M, Cout, C1, wt(name + ".sc.b"), Ref(), 0, 0, Ref(), 0, 0, "resnet.shortcut");
            if (C2) gemm(skip, C2, wt(name + ".sc.w", C1), Cin, sc, Cout, M, Cout, C2, Ref(), Ref(), 0, 0, sc, Cout, 0, "resnet.shortcut(skip)");
            res = sc;
        }
        Ref out = ws_stream((size_t)M * Cout * e);
        conv(h2, Cout, B, H, W, 1, 0, wt(name + ".conv2.w"), Cout, out, wt(name + ".conv2.b"), Ref(), 0, res, 0, "resnet.conv2");
        rel(h2);
        rel(sc);
        return out;
    }

    // Transformer2DModel.  x [M,C] -> new buffer [M,C]
    Ref transformer(const std::string& name, Ref x, int C, int heads, int layers, int H, int W) {
        const int M = B * H * W, e = 2, hd = C / heads;
        rows_img = H * W;
        const int nb = B / pl.n_img, L = H * W * pl.n_img;     // cross-image attention: [n*b, L, C] seen as [b, n*L, C]
        Ref n0 = ws((size_t)M * C * e);
        gn(x, C, Ref(), 0, B, H * W, 1e-6f, wt(name + ".norm.g"), wt(name + ".norm.b"), 0, n0, "transformer.norm");
        Ref h = ws_stream((size_t)M * C * e);
        // (round 6) a GEMM that writes the residual stream also writes the LayerNorm of its rows (gemm_ln): the row's next reader never fetches it back
        const bool fuse_ln = layers >= 1;      // (either stream mode: the op list does not depend on it; without a pair the LayerNorm kernel runs behind the GEMM)
        Ref n1_first;
        if (fuse_ln) {
            const std::string b0 = name + ".transformer_blocks.0";
            n1_first = ws((size_t)M * C * e);
            gemm_ln(n0, C, wt(name + ".proj_in.w"), C, h, C, M, C, C, wt(name + ".proj_in.b"), Ref(), 0, n1_first, wt(b0 + ".norm1.g"), wt(b0 + ".norm1.b"),
                    "transformer.proj_in+norm1");
        } else {
            dense(n0, wt(name + ".proj_in.w"), wt(name + ".proj_in.b"), h, M, C, C, Ref(), "transformer.proj_in");
        }
        rel(n0);
        for (int k = 0; k < layers; ++k) {
            const std::string b = name + ".transformer_blocks." + std::to_string(k);
            // self attention
            Ref n1;
            if (fuse_ln && k == 0) n1 = n1_first;
            else {
                n1 = ws((size_t)M * C * e);
                ln(h, n1, M, C, wt(b + ".norm1.g"), wt(b + ".norm1.b"));
            }
            Ref qkv = ws((size_t)M * 3 * C * e);
            dense(n1, wt(b + ".qkv.w"), Ref(), qkv, M, 3 * C, C, Ref(), "attn1.qkv");
            rel(n1);
            Ref a = ws((size_t)M * C * e);
            const AttnOpts& ao = pl.ao;
            if (ao.ref_mode == 0) {
                attn(prescaled(qkv, b + ".qkv.w", hd), 3 * C, at(qkv, (size_t)C * e), 3 * C, at(qkv, (size_t)2 * C * e), 3 * C, a, C, nb, L, L, heads, hd);
            } else {
                // reference attention: the store holds, per self-attention layer in execution order, the keys|values
                // [B - ref_skip][Lref][2C] of the pass that ran in 'w' mode (to_k / to_v act per token, so K(cat[x, ref]) =
                // cat[K(x), K(ref)] and the projected rows can be stored instead of the layer input)
                const int div = H0 / H;
                const int Lref = ao.ref_mode == 1 ? L : (ao.ref_H / div) * (ao.ref_W / div);
                const int skip = ao.ref_skip, nr = nb - skip;
                Ref st; st.kind = Ref::REFSTORE; st.off = ref_off;
                ref_off += (size_t)nr * Lref * 2 * C * e;
                if (ao.ref_mode == 1) {
                    attn(prescaled(qkv, b + ".qkv.w", hd), 3 * C, at(qkv, (size_t)C * e), 3 * C, at(qkv, (size_t)2 * C * e), 3 * C, a, C, nb, L, L, heads, hd);
                    copy2d(st, (size_t)2 * C * e, at(qkv, ((size_t)skip * L * 3 * C + C) * e), (size_t)3 * C * e, (size_t)2 * C * e,
                           (size_t)nr * L, "reference K,V -> store");
                } else {
                    attn(prescaled(qkv, b + ".qkv.w", hd), 3 * C, at(qkv, (size_t)C * e), 3 * C, at(qkv, (size_t)2 * C * e), 3 * C, a, C, skip, L, L, heads, hd);
                    const size_t o = (size_t)skip * L * 3 * C * e;
                    attn(prescaled(at(qkv, o), b + ".qkv.w", hd), 3 * C, at(qkv, o + (size_t)C * e), 3 * C, at(qkv, o + (size_t)2 * C * e), 3 * C,
                         at(a, (size_t)skip * L * C * e), C, nr, L, L, heads, hd, st, 2 * C, at(st, (size_t)C * e), 2 * C, Lref,
                         "attention (+reference tokens)");
                }
            }
            rel(qkv);
            Ref h2 = ws_stream((size_t)M * C * e);
            Ref n2 = ws((size_t)M * C * e);
            if (fuse_ln) {
                gemm_ln(a, C, wt(b + ".o1.w"), C, h2, C, M, C, C, wt(b + ".o1.b"), h, C, n2, wt(b + ".norm2.g"), wt(b + ".norm2.b"), "attn1.to_out+residual+norm2");
                rel(a); rel(h); h = h2;
            } else {
                dense(a, wt(b + ".o1.w"), wt(b + ".o1.b"), h2, M, C, C, h, "attn1.to_out+residual");
                rel(a); rel(h); h = h2;
                // cross attention (K/V hoisted)
                ln(h, n2, M, C, wt(b + ".norm2.g"), wt(b + ".norm2.b"));
            }
            Ref q = ws((size_t)M * C * e);
            dense(n2, wt(b + ".q2.w"), Ref(), q, M, C, C, Ref(), "attn2.to_q");
            rel(n2);
            end_prefix();          // the first cross-attention: from here on the halves of the batch differ
            Ref a2 = ws((size_t)M * C * e);
            const size_t ko = (size_t)u.kv_off[b] * e;
            attn(prescaled(q, b + ".q2.w", hd), C, at(ctxkv, ko), ld_kv, at(ctxkv, ko + (size_t)C * e), ld_kv, a2, C, nb, L, Lt, heads, hd);
            if (ao.ip_tokens > 0) {     // hidden_states + scale * SDPA(q, to_k_ip(ip), to_v_ip(ip))  (attention_processor.py:366-383)
                Ref aip = ws((size_t)M * C * e);
                attn(prescaled(q, b + ".q2.w", hd), C, at(ipkv, ko), ld_kv, at(ipkv, ko + (size_t)C * e), ld_kv, aip, C, nb, L, ao.ip_tokens, heads, hd, Ref(), 0, Ref(), 0,
                     0, "attention (ip tokens)");
                const int d = dt;
                const float sc = ao.ip_scale;
                const size_t nel = (size_t)M * C;
                op(OC_OTHER, 0, "attn2 += scale * ip", [=](const Run& r) { return mve_axpy(d, r.p(a2), r.p(aip), sc, r.p(a2), nel, r.stream); });
                rel(aip);
            }
            rel(q);
            Ref h3 = ws_stream((size_t)M * C * e);
            Ref n3 = ws((size_t)M * C * e);
            if (fuse_ln) {
                gemm_ln(a2, C, wt(b + ".o2.w"), C, h3, C, M, C, C, wt(b + ".o2.b"), h, C, n3, wt(b + ".norm3.g"), wt(b + ".norm3.b"), "attn2.to_out+residual+norm3");
                rel(a2); rel(h); h = h3;
            } else {
                dense(a2, wt(b + ".o2.w"), wt(b + ".o2.b"), h3, M, C, C, h, "attn2.to_out+residual");
                rel(a2); rel(h); h = h3;
                // feed forward (GEGLU fused in the first GEMM's epilogue)
                ln(h, n3, M, C, wt(b + ".norm3.g"), wt(b + ".norm3.b"));
            }
            Ref f = ws((size_t)M * 4 * C * e);
            gemm(n3, C, wt(b + ".ff1.w"), C, f, 4 * C, M, 8 * C, C, wt(b + ".ff1.b"), Ref(), 0, 0, Ref(), 0, MVE_GEMM_GEGLU, "ff.geglu");
            rel(n3);
            Ref h4 = ws_stream((size_t)M * C * e);
            dense(f, wt(b + ".ff2.w"), wt(b + ".ff2.b"), h4, M, C, 4 * C, h, "ff.out+residual");
            rel(f); rel(h); h = h4;
        }
        Ref out = ws_stream((size_t)M * C * e);
        dense(h, wt(name + ".proj_out.w"), wt(name + ".proj_out.b"), out, M, C, C, x, "transformer.proj_out+residual");
        rel(h);
        return out;
    }

    // network-specific plan builders: build, mid_block, add_residual (builder_unet.h); vae_attention, build_vae (builder_vae.h); build_sr (builder_sr.h);
    // build_lpips (builder_lpips.h); build_clip (builder_clip.h); build_clip_vision, build_resampler (builder_clip_vision.h); build_dpt (builder_dpt.h);
    // build_loftr (builder_loftr.h); build_sam (builder_sam.h); build_sam_decoder (builder_sam_decoder.h)
    Ref mid_block(Ref x, int C, int h, int w);
    Ref add_residual(Ref a, Ref src, int C, int h, int w, const char* label);
    Ref vae_attention(const std::string& name, Ref x, int C, int H, int W);
    int build_lpips(int B_, int H, int W, int io_dtype);
    int build_clip(int B_, int L);
    int build_clip_vision(int B_);
    int build_resampler(int B_, int n1);
    int build_dpt(int B_);
    int build_loftr(int N_, int H, int W, int phase);
    int build_sam(int B_);
    int build_sam_decoder(int N_, int P, int n_points, int has_box);
    int build_sr(int B_, int H, int W, int io_dtype);
    int build_vae(int B_, int H, int W, int io_dtype);
    int build(int B_, int H, int W, int n_img, int has_res, int io_dtype, int res_nhwc);
};

}  // namespace
