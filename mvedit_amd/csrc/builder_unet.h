// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): UNet2DConditionModel / ControlNetModel plan (prologue, down path, ControlNet outputs or residuals, mid, up path, head).
#pragma once
#include "executor_builder.h"

namespace {

// mid block: resnet, transformer, resnet.  x stays the caller's to release.
Ref Builder::mid_block(Ref x, int C, int h, int w) {
    const int n = c.n_levels;
    Ref y = resnet("mid_block.resnets.0", x, C, Ref(), 0, C, h, w);
    Ref z = transformer("mid_block.attentions.0", y, C, c.heads[n - 1], c.tlayers[n - 1], h, w);
    rel(y);
    Ref m = resnet("mid_block.resnets.1", z, C, Ref(), 0, C, h, w);
    rel(z);
    return m;
}

// a + ControlNet residual `src` ([B, C, h, w] in the io dtype, or NHWC in the engine dtype: Plan::res_nhwc) -> new buffer of the residual stream
Ref Builder::add_residual(Ref a, Ref src, int C, int h, int w, const char* label) {
    const int d = dt;
    const size_t elems = (size_t)B * h * w * C;
    Ref sum = ws_stream(elems * 2);
    const Ref a_lo = lo(a), sum_lo = lo(sum);
    Ref add = src;
    if (!pl.res_nhwc) {
        add = ws(elems * 2);
        to_nhwc(src, B, C, h, w, C, add, "residual nchw->nhwc");
    }
    op(OC_OTHER, 0, label, [=](const Run& r) { return mve_axpy_pair(d, r.p(a), r.p(a_lo), r.p(add), 1.0f, r.p(sum), r.p(sum_lo), elems, r.stream); });
    rel(add);
    return sum;
}

int Builder::build(int B_, int H, int W, int n_img, int has_res, int io_dtype, int res_nhwc) {
    // the closures below must not capture `this`: they take B_ and the other locals by value
    { const AttnOpts keep = pl.ao; begin(B_, H, W, n_img, io_dtype); pl.ao = keep; }
    pl.has_res = has_res; pl.res_nhwc = res_nhwc; pl.add_type = c.add_type;
    const int e = 2, n = c.n_levels, L = c.layers_per_block, T = c.temb_dim();
    const int d = dt;
    ld_temb = u.sum_temb; ld_kv = u.sum_kv;
    MVE_CHECK(B_ % n_img == 0, MVE_ERR_ARG, "unet: batch %d not divisible by num_cross_attn_imgs %d", B_, n_img);
    MVE_CHECK((H % (1 << (n - 1))) == 0 && (W % (1 << (n - 1))) == 0, MVE_ERR_ARG,
              "unet: latent size %dx%d must be divisible by %d", H, W, 1 << (n - 1));
    for (int i = 0; i < n; ++i) {
        const int hd = c.ch[i] / c.heads[i];
        MVE_CHECK(!c.attn[i] || hd == 40 || hd == 64 || hd == 80 || hd == 160, MVE_ERR_ARG, "unet: unsupported head dim %d", hd);
    }
    // ---- prologue: layout conversion, time embedding, hoisted projections --------------------------
    const int M0 = B_ * H * W;
    Ref x_in = ws((size_t)M0 * 8 * e);
    to_nhwc(arg(Ref::SAMPLE), B_, c.in_ch, H, W, 8, x_in);
    Ref tsin = ws((size_t)B_ * c.ch[0] * e);
    {
        const Ref tt = arg(Ref::TIMESTEPS);
        const int dim = c.ch[0];
        op(OC_OTHER, 0, "timestep_embedding", [=](const Run& r) { return mve_timestep_embedding(d, (const float*)r.p(tt), B_, dim, r.p(tsin), r.stream); });
    }
    Ref e1 = ws((size_t)B_ * T * e);
    dense(tsin, wt("time.w1"), wt("time.b1"), e1, B_, T, c.ch[0], Ref(), "time_embedding.linear_1");
    rel(tsin);
    op(OC_OTHER, 0, "silu", [=](const Run& r) { return mve_silu(d, r.p(e1), r.p(e1), (size_t)B_ * T, r.stream); });
    Ref emb = ws((size_t)B_ * T * e);
    dense(e1, wt("time.w2"), wt("time.b2"), emb, B_, T, T, Ref(), "time_embedding.linear_2");
    rel(e1);
    if (c.add_type == 1) {
        // addition_embed_type='text_time' (diffusers UNet2DConditionModel.get_aug_embed, ControlNetModel alike): emb += add_embedding(cat([text_embeds,
        // add_time_proj(time_ids.flatten()).reshape(B, -1)])).  The sum is the second GEMM's fused residual: one rounding where the half modules round
        // the embedding and the sum separately.
        const int P = c.add_P, td = c.add_time_dim;
        Ref row = ws((size_t)B_ * P * e);
        op(OC_OTHER, 0, "add_embedding.text_time", [=](const Run& r) {
            if (!r.add_text || !r.add_ids || r.add_text_dim + r.add_n_ids * td != P) {
                mve_set_error("unet: a text_time engine needs text_embeds / time_ids (mve_unet_bind_added_cond) before every forward");
                return (int)MVE_ERR_STATE;
            }
            return mve_text_time_embedding(d, r.add_text, r.add_text_dtype, r.add_text_dim, r.add_ids, r.add_n_ids, td, B_, r.p(row), r.stream);
        });
        Ref a1 = ws((size_t)B_ * T * e);
        dense(row, wt("add.w1"), wt("add.b1"), a1, B_, T, P, Ref(), "add_embedding.linear_1");
        rel(row);
        op(OC_OTHER, 0, "silu", [=](const Run& r) { return mve_silu(d, r.p(a1), r.p(a1), (size_t)B_ * T, r.stream); });
        Ref emb_sum = ws((size_t)B_ * T * e);
        dense(a1, wt("add.w2"), wt("add.b2"), emb_sum, B_, T, T, emb, "add_embedding.linear_2");
        rel(a1);
        rel(emb);
        emb = emb_sum;
    }
    op(OC_OTHER, 0, "silu", [=](const Run& r) { return mve_silu(d, r.p(emb), r.p(emb), (size_t)B_ * T, r.stream); });
    tproj = ws((size_t)B_ * ld_temb * 4);
    dense(emb, wt("temb_proj.w"), wt("temb_proj.b"), tproj, B_, ld_temb, T, Ref(), "time_emb_proj (all resnets, one GEMM)", MVE_GEMM_OUT_F32);
    rel(emb);
    // encoder_hidden_states [B_, Lc, ctx_dim]; under cross-image attention the text context is the mean of each group
    // (joint_attn.py:19-24).  K/V of every cross-attention layer in one GEMM.
    const Ref ctx_src = arg(Ref::CTX);
    ctxB = B_ / n_img;
    Ref ctx_in = ctx_src, ctx_tmp;
    const int Lc = ctx_rows_per_img;
    const bool ctx_needs_copy = (io_dtype != dt) || n_img > 1;
    if (ctx_needs_copy) {
        ctx_tmp = ws((size_t)B_ * Lc * c.ctx_dim * e);
        // dtype conversion via the packing kernel semantics: reuse nchw->nhwc with H=W=1 treats [B_*Lc, ctx] as NC11
        to_nhwc(ctx_src, B_ * Lc, c.ctx_dim, 1, 1, c.ctx_dim, ctx_tmp, "ctx->dtype");
        ctx_in = ctx_tmp;
        if (n_img > 1) {
            Ref cm = ws((size_t)ctxB * Lc * c.ctx_dim * e);
            const long long R = (long long)Lc * c.ctx_dim, total = (long long)ctxB * R;
            Ref in = ctx_tmp;
            op(OC_OTHER, 0, "ctx group mean", [=](const Run& r) {
                const unsigned grid = (unsigned)((total + 255) / 256);
                if (d == MVE_F16) k_group_mean<F16Tag><<<grid, 256, 0, r.stream>>>((const f16*)r.p(in), (f16*)r.p(cm), R, n_img, total);
                else k_group_mean<BF16Tag><<<grid, 256, 0, r.stream>>>((const bf16*)r.p(in), (bf16*)r.p(cm), R, n_img, total);
                return hipGetLastError() == hipSuccess ? MVE_OK : MVE_ERR_HIP;
            });
            ctx_in = cm;
        }
    }
    const AttnOpts ao = pl.ao;
    MVE_CHECK(ao.ctx_tail >= 0 && ao.ctx_tail < Lc, MVE_ERR_ARG, "unet: cannot ignore the last %d rows of a context of %d rows", ao.ctx_tail, Lc);
    MVE_CHECK(!ao.ctx_tail || !ao.ip_tokens, MVE_ERR_ARG, "unet: an ignored context tail (%d rows) is not combined with ip tokens", ao.ctx_tail);
    Lt = Lc - ao.ip_tokens - ao.ctx_tail;
    H0 = H;
    ref_off = 0;
    if (ao.ip_tokens > 0) {
        MVE_CHECK(Lt > 0, MVE_ERR_ARG, "unet: context of %d rows cannot hold %d ip tokens", Lc, ao.ip_tokens);
        MVE_CHECK(u.n_ip_loaded == 2 * u.n_xf_layers, MVE_ERR_STATE, "unet: IP-Adapter enabled but only %d of %d to_k_ip/to_v_ip weights loaded",
                  u.n_ip_loaded, 2 * u.n_xf_layers);
        // split [text | ip] rows of every item into two dense matrices (attention_processor.py:338-341)
        const size_t rowb = (size_t)c.ctx_dim * e;
        Ref ctx_text = ws((size_t)ctxB * Lt * rowb), ctx_ip = ws((size_t)ctxB * ao.ip_tokens * rowb);
        copy2d(ctx_text, Lt * rowb, ctx_in, Lc * rowb, Lt * rowb, ctxB, "ctx text rows");
        copy2d(ctx_ip, ao.ip_tokens * rowb, at(ctx_in, Lt * rowb), Lc * rowb, ao.ip_tokens * rowb, ctxB, "ctx ip rows");
        ipkv = ws((size_t)ctxB * ao.ip_tokens * ld_kv * e);
        dense(ctx_ip, wt("ip_kv.w"), Ref(), ipkv, ctxB * ao.ip_tokens, ld_kv, c.ctx_dim, Ref(), "ip-adapter K,V (all layers, one GEMM)");
        rel(ctx_ip);
        ctx_in = ctx_text;
    } else if (ao.ctx_tail > 0) {
        // the first Lt rows of every item, densely: the K/V GEMM below then never sees the tail (attention_processor.py:519-520)
        const size_t rowb = (size_t)c.ctx_dim * e;
        Ref ctx_text = ws((size_t)ctxB * Lt * rowb);
        copy2d(ctx_text, Lt * rowb, ctx_in, Lc * rowb, Lt * rowb, ctxB, "ctx rows without the tail");
        ctx_in = ctx_text;
    }
    if (ao.ref_mode) {
        MVE_CHECK(n_img == 1, MVE_ERR_ARG, "unet: reference attention and cross-image attention are exclusive (adapter3d_mixin.py:194)");
        MVE_CHECK(ao.ref_skip >= 0 && ao.ref_skip < B_, MVE_ERR_ARG, "unet: ref_skip %d out of range", ao.ref_skip);
        if (ao.ref_mode == 2)
            MVE_CHECK(ao.ref_H > 0 && ao.ref_W > 0 && ao.ref_H % (1 << (n - 1)) == 0 && ao.ref_W % (1 << (n - 1)) == 0, MVE_ERR_ARG,
                      "unet: bad reference latent size %dx%d", ao.ref_H, ao.ref_W);
    }
    ctxkv = ws((size_t)ctxB * Lt * ld_kv * e);
    dense(ctx_in, wt("ctx_kv.w"), Ref(), ctxkv, ctxB * Lt, ld_kv, c.ctx_dim, Ref(), "cross-attention K,V (all layers, one GEMM)");
    // ---- conv_in + down path ---------------------------------------------------------------------------
    struct Skip { Ref r; int C, H, W; };
    std::vector<Skip> skips;
    Ref x = ws_stream((size_t)M0 * c.ch[0] * e);
    if (c.kind == Kind::ControlNet) {
        // controlnet_cond_embedding on the 8H x 8W conditioning image, added to conv_in(sample)
        const int Hc = 8 * H, Wc = 8 * W, cc = c.cond_ch;
        // cn_cond_repeat = R: Bc = B_ / R conditioning images, item b of the batch uses image b mod Bc (the two halves of a CFG batch share them)
        const int R = pl.ao.cn_cond_repeat > 1 ? pl.ao.cn_cond_repeat : 1;
        MVE_CHECK(B_ % R == 0, MVE_ERR_ARG, "controlnet: batch %d is not a multiple of the conditioning repeat %d", B_, R);
        MVE_CHECK(R == 1 || !pl.ao.residual_pair, MVE_ERR_ARG, "controlnet: shared conditioning images are not combined with the residual-pair mode");
        const int Bc = B_ / R;
        Ref cimg = ws((size_t)Bc * Hc * Wc * 8 * e);
        to_nhwc(arg(Ref::CNCOND), Bc, cc, Hc, Wc, 8, cimg, "cond nchw->nhwc");
        const std::string en = "controlnet_cond_embedding.";
        int hc = Hc, wc = Wc, ci = 8;
        Ref cur = cimg;
        auto emb_conv = [&](const std::string& nm, int co, int stride, bool act) {
            const int ho = (hc - 1) / stride + 1, wo = (wc - 1) / stride + 1;
            Ref y = ws((size_t)Bc * ho * wo * co * e);
            conv(cur, ci, Bc, hc, wc, stride, 0, wt(nm + ".w"), co, y, wt(nm + ".b"), Ref(), 0, Ref(), 0, "cond_embedding.conv");
            rel(cur);
            if (act) {
                const size_t nel = (size_t)Bc * ho * wo * co;
                op(OC_OTHER, 0, "silu", [=](const Run& r) { return mve_silu(d, r.p(y), r.p(y), nel, r.stream); });
            }
            cur = y; hc = ho; wc = wo; ci = co;
        };
        emb_conv(en + "conv_in", CN_EMB[0], 1, true);
        for (int k = 0; k < 6; ++k) emb_conv(en + "blocks." + std::to_string(k), CN_EMB[(k + 1) / 2], (k & 1) ? 2 : 1, true);
        emb_conv(en + "conv_out", c.ch[0], 1, false);
        MVE_CHECK(hc == H && wc == W, MVE_ERR_ARG, "controlnet: conditioning image must be 8x the latent size");
        for (int rep = 0; rep < R; ++rep) {      // one conv_in launch per group of Bc items: each adds the same embedding in its epilogue
            Ref xi = x_in, xo = x;
            xi.off += (size_t)rep * Bc * H * W * 8 * e;
            xo.off += (size_t)rep * Bc * H * W * c.ch[0] * e;
            conv(xi, 8, Bc, H, W, 1, 0, wt("conv_in.w"), c.ch[0], xo, wt("conv_in.b"), Ref(), 0, cur, 0, "conv_in + cond_embedding");
        }
        rel(cur);
    } else {
        conv(x_in, 8, B_, H, W, 1, 0, wt("conv_in.w"), c.ch[0], x, wt("conv_in.b"), Ref(), 0, Ref(), 0, "conv_in");
    }
    rel(x_in);
    // CFG prefix (executor_builder.h): planned for a UNet batch of two equal halves whose cross-image groups do not straddle the middle.  Reference
    // attention exempts the CFG-first item (ref_skip), so its halves differ; ControlNet engines are the follow-up.  conv_in stays outside: its output
    // is a skip the last up-block reads at full batch, and it costs less than broadcasting it would.
    if (c.kind != Kind::ControlNet && pl.ao.cfg_prefix && B_ % 2 == 0 && (B_ / 2) % n_img == 0 && pl.ao.ref_mode == 0)
        begin_prefix((size_t)(B_ / 2) * c.in_ch * H * W * esz(io_dtype), (size_t)(B_ / 2) * ld_temb * 4);
    skips.push_back({x, c.ch[0], H, W});
    int h = H, w = W, cin = c.ch[0];
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < L; ++j) {
            const std::string rn = "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
            Ref y = resnet(rn, x, cin, Ref(), 0, c.ch[i], h, w);
            cin = c.ch[i];
            if (c.attn[i]) {
                Ref z = transformer("down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), y, cin, c.heads[i], c.tlayers[i], h, w);
                rel(y);
                y = z;
            }
            x = y;
            skips.push_back({x, cin, h, w});
        }
        if (i + 1 < n) {
            const std::string dn = "down_blocks." + std::to_string(i) + ".downsamplers.0.conv";
            Ref y = ws_stream((size_t)B_ * (h / 2) * (w / 2) * cin * e);
            conv(x, cin, B_, h, w, 2, 0, wt(dn + ".w"), cin, y, wt(dn + ".b"), Ref(), 0, Ref(), 0, "downsample");
            h /= 2; w /= 2;
            x = y;
            skips.push_back({x, cin, h, w});
        }
    }
    end_prefix();          // (a network without cross-attention in its down path: the prefix does not reach into unet_dec)
    pl.enc_end = pl.ops.size();
    if (c.kind == Kind::ControlNet) {
        const int C = c.ch[n - 1];
        for (size_t i = 0; i < skips.size(); ++i)
            zero_conv(skips[i].r, skips[i].C, B_ * skips[i].H * skips[i].W, skips[i].H * skips[i].W, "controlnet_down_blocks." + std::to_string(i), (int)i);
        zero_conv(mid_block(x, C, h, w), C, B_ * h * w, h * w, "controlnet_mid_block", (int)skips.size());
        pl.ref_store_bytes = ref_off;
        return finish("controlnet");
    }
    // ---- ControlNet residuals (diffusers.py:110-121 of the reference) -----------------------------------
    if (has_res)
        for (size_t i = 0; i < skips.size(); ++i)      // the un-summed skip stays allocated: unet_enc state must survive unet_dec
            skips[i].r = add_residual(skips[i].r, arg(Ref::DOWNRES, (int)i), skips[i].C, skips[i].H, skips[i].W, "skip += controlnet residual");
    // ---- mid ------------------------------------------------------------------------------------------------
    x = mid_block(x, c.ch[n - 1], h, w);
    if (has_res) {
        Ref sum = add_residual(x, arg(Ref::MIDRES), c.ch[n - 1], h, w, "mid += controlnet residual");
        rel(x);
        x = sum;
    }
    // ---- up path ----------------------------------------------------------------------------------------------
    int cur = c.ch[n - 1];
    for (int i = 0; i < n; ++i) {
        const int lvl = n - 1 - i, cout = c.ch[lvl];
        for (int j = 0; j < L + 1; ++j) {
            Skip sk = skips.back();
            skips.pop_back();
            const std::string rn = "up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
            Ref y = resnet(rn, x, cur, sk.r, sk.C, cout, h, w);
            rel(x);
            if (has_res) rel(sk.r);     // the summed copy; the original skip is enc state
            cur = cout;
            if (c.attn[lvl]) {
                Ref z = transformer("up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), y, cout, c.heads[lvl], c.tlayers[lvl], h, w);
                rel(y);
                y = z;
            }
            x = y;
        }
        if (i + 1 < n) {
            const std::string un = "up_blocks." + std::to_string(i) + ".upsamplers.0.conv";
            Ref y = ws_stream((size_t)B_ * (2 * h) * (2 * w) * cout * e);
            upsample_conv(x, cout, B_, h, w, un, y);
            rel(x);
            h *= 2; w *= 2;
            x = y;
        }
    }
    // ---- head ---------------------------------------------------------------------------------------------------
    Ref hn = ws((size_t)M0 * c.ch[0] * e);
    gn(x, c.ch[0], Ref(), 0, B_, H * W, c.eps, wt("norm_out.g"), wt("norm_out.b"), 1, hn, "conv_norm_out+silu");
    rel(x);
    Ref o8 = ws((size_t)M0 * 8 * 4);
    conv(hn, c.ch[0], B_, H, W, 1, 0, wt("conv_out.w"), 8, o8, wt("conv_out.b"), Ref(), 0, Ref(), MVE_GEMM_OUT_F32, "conv_out");
    rel(hn);
    to_nchw(o8, MVE_F32, 8, B_, c.out_ch, H, W);
    if (pl.cfg_prefix) { *pfx_flag = ar.peak; pl.cfg_flag_off = ar.peak; }      // the flag lives in the tail pad: the workspace size does not move
    pl.ref_store_bytes = ref_off;
    return finish("unet");
}

}  // namespace
