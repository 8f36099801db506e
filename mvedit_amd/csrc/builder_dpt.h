// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): the DPT-hybrid plan -- the
// Omnidata normal predictor behind `MVEdit3DPipeline.normal_model`.
#pragma once
#include "executor_builder.h"

namespace {

// DPTDepthModel(backbone='vitb_rn50_384').forward (omnidata_modules/midas/dpt_depth.py:67-107, vit.py:61-155, blocks.py:231-341) with the
// backbone arithmetic of transformers' DPTViTHybridEmbeddings over a BitBackbone (models/bit/modeling_bit.py, models/dpt/modeling_dpt.py).
// Pixels arrive as Run::sample ([B,3,S,S] NCHW, engine dtype) and the prediction leaves through Run::out ([B,num_channels,S,S] NCHW);
// everything in between is NHWC.  Run::cn_out carries DPT_TAPS optional tap tensors (copied out only when the caller gave a pointer):
// stem, stage 1-3 (NHWC), the two token taps [B,T,C], the four fusion outputs in execution order (refinenet4 ... refinenet1, NHWC).
// Every convolution of the backbone is bias-free with weights that were standardised when they were packed (mvedit_amd/normal_model.py), so
// it is a plain GEMM / conv here.  Dense GEMMs never split K (rows_img = 0).
constexpr int DPT_TAPS = 10;

int Builder::build_dpt(int B_) {
    B = B_; dt = c.dtype;
    pl = Plan();
    const int S = c.dp_image, e = 2, d = dt, Bn = B_, C = c.ch[0], heads = c.heads[0], hd = C / heads, I = c.dp_inter, F = c.dp_features;
    const int Gd = S / 16, G2 = Gd * Gd, T = G2 + 1, M = Bn * T, Cs = c.dp_stem, NC = c.out_ch;
    pl.B = B_; pl.H = S; pl.W = S; pl.n_img = 1; pl.io_dtype = c.dtype;
    const float eps = c.eps, gn_eps = 1e-5f /* BitGroupNormActivation's default */, scale = 1.0f / sqrtf((float)hd);
    MVE_CHECK((size_t)Bn * S * S * 32 < ((size_t)1 << 31) && (size_t)Bn * (S / 2) * (S / 2) * 152 < ((size_t)1 << 31) &&
                  (size_t)Bn * (S / 2) * (S / 2) * (size_t)(F > Cs ? F : Cs) < ((size_t)1 << 31) && (size_t)M * (size_t)(I > 3 * C ? I : 3 * C) < ((size_t)1 << 31),
              MVE_ERR_ARG, "dpt: batch %d overflows 32-bit activation indexing", Bn);
    ld_temb = 0; ld_kv = 0;
    rows_img = 0;
    Ref px; px.kind = Ref::SAMPLE;
    Ref out; out.kind = Ref::OUT;
    auto tap = [&](Ref x, size_t bytes, int k, const char* what) {      // copied out only when the caller gave a tensor for it
        live(x, what);
        op(OC_OTHER, 0, what, [=](const Run& r) {
            void* dst = r.cn_out ? r.cn_out[k] : nullptr;
            if (!dst) return (int)MVE_OK;
            return hipMemcpyAsync(dst, r.p(x), bytes, hipMemcpyDeviceToDevice, r.stream) == hipSuccess ? (int)MVE_OK : (int)MVE_ERR_HIP;
        });
    };
    auto norm = [&](Ref x, int Cx, int HW, const std::string& n, int act, const char* what) {      // GroupNorm (+ ReLU: selector 2) -> new buffer
        Ref y = ws((size_t)Bn * HW * Cx * e);
        gn(x, Cx, Ref(), 0, Bn, HW, gn_eps, wt(n + ".g"), wt(n + ".b"), act, y, what);
        return y;
    };
    auto conv1 = [&](Ref x, int rows, int Cin, const std::string& w, Ref bias, int Cout, const char* what) {      // 1 x 1 convolution = GEMM -> new buffer
        Ref y = ws((size_t)rows * Cout * e);
        gemm(x, Cin, wt(w), Cin, y, Cout, rows, Cout, Cin, bias, Ref(), 0, 0, Ref(), 0, 0, what);
        return y;
    };
    auto conv3 = [&](Ref x, int Cin, int H, int W, int stride, int flags, const std::string& w, Ref bias, int Cout, Ref res, const char* what) {
        const int Ho = H / stride, Wo = W / stride;
        Ref y = ws((size_t)Bn * Ho * Wo * Cout * e);
        conv(x, Cin, Bn, H, W, stride, 0, wt(w), Cout, y, bias, Ref(), 0, res, flags, what);
        return y;
    };
    auto add_relu = [&](Ref a, Ref b, Ref y, size_t nel, const char* what) {      // y = max(a + b, 0); b may be null
        live(a, what); live(b, what); live(y, what);
        op(OC_OTHER, 0, what, [=](const Run& r) { return mve_dpt_add_relu(d, r.p(a), r.p(b), r.p(y), nel, r.stream); });
    };
    auto layernorm = [&](Ref x, Ref y, const std::string& n) {
        const Ref g = wt(n + ".g"), b = wt(n + ".b");
        live(x, "layernorm"); live(y, "layernorm");
        op(OC_NORM, 0, "layernorm", [=](const Run& r) { return mve_layernorm(d, r.p(x), C, r.p(y), C, M, C, (const float*)r.p(g), (const float*)r.p(b), eps, r.stream); });
    };

    // ---- stem: 7 x 7 / 2 "same" convolution as a GEMM over gathered rows, GroupNorm + ReLU, 3 x 3 / 2 "same" max-pool --------------------------
    int H = S / 2;
    Ref x;
    {
        Ref rows = ws((size_t)Bn * H * H * 152 * e);
        op(OC_OTHER, 0, "stem window rows", [=](const Run& r) { return mve_dpt_stem_rows(d, r.p(px), Bn, S, r.p(rows), 152, r.stream); });
        Ref s0 = conv1(rows, Bn * H * H, 152, "stem.w", Ref(), Cs, "stem.conv 7x7/2");
        rel(rows);
        Ref s1 = norm(s0, Cs, H * H, "stem", 2, "stem.norm+relu");
        rel(s0);
        x = ws((size_t)Bn * (H / 2) * (H / 2) * Cs * e);
        const int Hs = H;
        live(s1, "stem.maxpool"); live(x, "stem.maxpool");
        op(OC_OTHER, 0, "stem.maxpool 3x3/2", [=](const Run& r) { return mve_dpt_maxpool(d, r.p(s1), Bn, Hs, Hs, Cs, r.p(x), r.stream); });
        rel(s1);
        H /= 2;
        tap(x, (size_t)Bn * H * H * Cs * e, 0, "stem -> tap");
    }

    // ---- three stages of BitBottleneckLayer (non-pre-activation): the stride sits in the 3 x 3 convolution ("same": the extra row / column after =
    // MVE_CONV_PAD_BR), the first layer's shortcut is a (strided) 1 x 1 convolution + GroupNorm WITHOUT activation --------------------------------
    Ref stage_out[3];
    int stage_H[3];
    int cin = Cs;
    for (int s = 0; s < 3; ++s) {
        const int cout = c.dp_stage[s], mid = cout / 4;
        for (int m = 0; m < c.dp_depth[s]; ++m) {
            const std::string b = "s" + std::to_string(s) + ".b" + std::to_string(m);
            const int stride = (m == 0 && s > 0) ? 2 : 1, Ho = H / stride;
            Ref t1 = conv1(x, Bn * H * H, cin, b + ".c1.w", Ref(), mid, "bottleneck.conv1");
            Ref t1n = norm(t1, mid, H * H, b + ".n1", 2, "bottleneck.norm1+relu");
            rel(t1);
            Ref t2 = conv3(t1n, mid, H, H, stride, stride == 2 ? MVE_CONV_PAD_BR : 0, b + ".c2.w", Ref(), mid, Ref(), "bottleneck.conv2 3x3");
            rel(t1n);
            Ref t2n = norm(t2, mid, Ho * Ho, b + ".n2", 2, "bottleneck.norm2+relu");
            rel(t2);
            Ref t3 = conv1(t2n, Bn * Ho * Ho, mid, b + ".c3.w", Ref(), cout, "bottleneck.conv3");
            rel(t2n);
            Ref t3n = norm(t3, cout, Ho * Ho, b + ".n3", 0, "bottleneck.norm3");
            rel(t3);
            Ref sc = x;
            if (m == 0) {
                Ref xs = x;
                if (stride == 2) {
                    xs = ws((size_t)Bn * Ho * Ho * cin * e);
                    const int Hi = H, ci = cin;
                    live(x, "shortcut stride-2 gather"); live(xs, "shortcut stride-2 gather");
                    op(OC_OTHER, 0, "shortcut stride-2 gather", [=](const Run& r) { return mve_dpt_gather_s2(d, r.p(x), Bn, Hi, Hi, ci, r.p(xs), r.stream); });
                }
                Ref ds = conv1(xs, Bn * Ho * Ho, cin, b + ".ds.w", Ref(), cout, "bottleneck.downsample.conv");
                if (stride == 2) rel(xs);
                sc = norm(ds, cout, Ho * Ho, b + ".dn", 0, "bottleneck.downsample.norm");
                rel(ds);
            }
            Ref y = ws((size_t)Bn * Ho * Ho * cout * e);
            add_relu(t3n, sc, y, (size_t)Bn * Ho * Ho * cout, "bottleneck add+relu");
            rel(t3n);
            if (m == 0) rel(sc);
            if (!(m == 0 && s > 0)) rel(x);      // the outputs of stages 1 and 2 stay live for the decoder (layer1_rn / layer2_rn below)
            x = y; cin = cout; H = Ho;
        }
        stage_out[s] = x; stage_H[s] = H;
        tap(x, (size_t)Bn * H * H * cout * e, 1 + s, "stage -> tap");
    }

    // ---- the decoder's inputs from the two feature maps: layer1_rn / layer2_rn --------------------------------------------------------------------
    Ref rn[4];
    rn[0] = conv3(stage_out[0], c.dp_stage[0], stage_H[0], stage_H[0], 1, 0, "rn1.w", Ref(), F, Ref(), "layer1_rn");
    rel(stage_out[0]);
    rn[1] = conv3(stage_out[1], c.dp_stage[1], stage_H[1], stage_H[1], 1, 0, "rn2.w", Ref(), F, Ref(), "layer2_rn");
    rel(stage_out[1]);

    // ---- tokens: 1 x 1 projection of stage 3, class token + position table, pre-norm ViT blocks ---------------------------------------------------
    MVE_CHECK(H == Gd, MVE_ERR_STATE, "dpt plan: stage 3 is %d x %d, the token grid %d x %d", H, H, Gd, Gd);
    {
        Ref patch = conv1(x, Bn * G2, c.dp_stage[2], "proj.w", wt("proj.b"), C, "patch_embed.proj");
        rel(x);
        x = ws((size_t)M * C * e);
        const Ref cls = wt("cls"), pos = wt("pos");
        live(patch, "class + position embedding"); live(x, "class + position embedding");
        op(OC_OTHER, 0, "class + position embedding", [=](const Run& r) { return mve_clip_vision_embed(d, r.p(patch), r.p(cls), r.p(pos), r.p(x), Bn, G2, C, r.stream); });
        rel(patch);
    }
    // Reassemble (vit.py:36-47, :431-462): ProjectReadout = GELU(Linear(cat(token, cls))) as ONE GEMM over the patch tokens -- the class token's half
    // of the weight gives a per-image row vector (a B-row GEMM over the class rows, fp32 out, the bias folded in) that the token GEMM's epilogue adds
    // -- then the 1 x 1 convolution, for tap 4 the 3 x 3 / 2 convolution with padding 1, and layerN_rn.
    auto reassemble = [&](Ref xt, int which) {
        const std::string r_ = which == 3 ? "r3" : "r4";
        const int N = which == 3 ? c.dp_neck[0] : c.dp_neck[1];
        Ref tok = ws((size_t)Bn * G2 * C * e);
        copy2d(tok, (size_t)G2 * C * e, at(xt, (size_t)C * e), (size_t)T * C * e, (size_t)G2 * C * e, Bn, "patch tokens");
        Ref rv = ws((size_t)Bn * C * 4);
        gemm(xt, T * C, wt(r_ + ".wc"), C, rv, C, Bn, C, C, wt(r_ + ".b"), Ref(), 0, 0, Ref(), 0, MVE_GEMM_OUT_F32, "readout (class half + bias)");
        Ref ro = ws((size_t)Bn * G2 * C * e);
        gemm(tok, C, wt(r_ + ".wt"), C, ro, C, Bn * G2, C, C, Ref(), rv, C, G2, Ref(), 0, 0, "readout (token half + class row)");
        rel(tok); rel(rv);
        {
            const size_t nel = (size_t)Bn * G2 * C;
            live(ro, "readout gelu");
            op(OC_OTHER, 0, "readout gelu", [=](const Run& r) { return mve_act(d, MVE_ACT_GELU, r.p(ro), r.p(ro), nel, r.stream); });
        }
        Ref p = conv1(ro, Bn * G2, C, r_ + ".p.w", wt(r_ + ".p.b"), N, "act_postprocess conv1x1");
        rel(ro);
        int Hp = Gd;
        if (which == 4) {
            Ref z = conv3(p, N, Gd, Gd, 2, 0, "r4.z.w", wt("r4.z.b"), N, Ref(), "act_postprocess4 conv3x3/2");
            rel(p); p = z; Hp = Gd / 2;
        }
        Ref y = conv3(p, N, Hp, Hp, 1, 0, which == 3 ? "rn3.w" : "rn4.w", Ref(), F, Ref(), which == 3 ? "layer3_rn" : "layer4_rn");
        rel(p);
        return y;
    };
    for (int k = 0; k <= c.dp_tap[1]; ++k) {
        const std::string b = "l" + std::to_string(k);
        Ref n1 = ws((size_t)M * C * e);
        layernorm(x, n1, b + ".n1");
        Ref qkv = ws((size_t)M * 3 * C * e);
        gemm(n1, C, wt(b + ".qkv.w"), C, qkv, 3 * C, M, 3 * C, C, wt(b + ".qkv.b"), Ref(), 0, 0, Ref(), 0, 0, "attn.qkv");
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
        gemm(a, C, wt(b + ".o.w"), C, x2, C, M, C, C, wt(b + ".o.b"), Ref(), 0, 0, x, C, 0, "attn.proj+residual");
        rel(a); rel(x); x = x2;
        Ref n2 = ws((size_t)M * C * e);
        layernorm(x, n2, b + ".n2");
        Ref f = ws((size_t)M * I * e);
        gemm(n2, C, wt(b + ".fc1.w"), C, f, I, M, I, C, wt(b + ".fc1.b"), Ref(), 0, 0, Ref(), 0, 0, "mlp.fc1");
        rel(n2);
        {
            const size_t nel = (size_t)M * I;
            live(f, "gelu");
            op(OC_OTHER, 0, "gelu", [=](const Run& r) { return mve_act(d, MVE_ACT_GELU, r.p(f), r.p(f), nel, r.stream); });
        }
        Ref x3 = ws((size_t)M * C * e);
        gemm(f, I, wt(b + ".fc2.w"), I, x3, C, M, C, I, wt(b + ".fc2.b"), Ref(), 0, 0, x, C, 0, "mlp.fc2+residual");
        rel(f); rel(x); x = x3;
        // the taps are block outputs: the backbone's final LayerNorm never reaches the prediction
        if (k == c.dp_tap[0]) { tap(x, (size_t)M * C * e, 4, "token tap 3 -> tap"); rn[2] = reassemble(x, 3); }
        if (k == c.dp_tap[1]) { tap(x, (size_t)M * C * e, 5, "token tap 4 -> tap"); rn[3] = reassemble(x, 4); }
    }
    rel(x);

    // ---- decoder: FeatureFusionBlock_custom x 4 (blocks.py:291-341), bn=False, ReLU(inplace=False), align_corners=True ----------------------------
    auto rcu = [&](const std::string& n, Ref xin, int Hf) {      // ResidualConvUnit_custom: conv2(relu(conv1(relu(x)))) + x
        const size_t nel = (size_t)Bn * Hf * Hf * F;
        Ref r0 = ws(nel * e);
        add_relu(xin, Ref(), r0, nel, "relu");
        Ref h = conv3(r0, F, Hf, Hf, 1, 0, n + ".c1.w", wt(n + ".c1.b"), F, Ref(), "resConfUnit.conv1");
        rel(r0);
        add_relu(h, Ref(), h, nel, "relu");
        Ref y = conv3(h, F, Hf, Hf, 1, 0, n + ".c2.w", wt(n + ".c2.b"), F, xin, "resConfUnit.conv2+residual");
        rel(h);
        return y;
    };
    auto upsample = [&](Ref xin, int Hf, int Cx, const char* what) {
        Ref y = ws((size_t)Bn * 4 * Hf * Hf * Cx * e);
        live(xin, what); live(y, what);
        op(OC_OTHER, 0, what, [=](const Run& r) { return mve_dpt_upsample2x(d, r.p(xin), Bn, Hf, Hf, Cx, r.p(y), r.stream); });
        return y;
    };
    Ref path;
    int Hf = Gd / 2;
    for (int k = 3; k >= 0; --k) {      // refinenet4 (one input) ... refinenet1
        const std::string f = "f" + std::to_string(k + 1);
        Ref s = rn[k];
        if (k < 3) {
            Ref res = rcu(f + ".u1", rn[k], Hf);
            rel(rn[k]);
            const size_t nel = (size_t)Bn * Hf * Hf * F;
            live(path, "fusion add"); live(res, "fusion add");
            op(OC_OTHER, 0, "fusion add", [=](const Run& r) { return mve_axpy(d, r.p(path), r.p(res), 1.0f, r.p(res), nel, r.stream); });
            rel(path);
            s = res;
        }
        Ref o = rcu(f + ".u2", s, Hf);
        rel(s);
        Ref up = upsample(o, Hf, F, "fusion upsample x2 (align_corners)");
        rel(o);
        Hf *= 2;
        path = conv1(up, Bn * Hf * Hf, F, f + ".out.w", wt(f + ".out.b"), F, "fusion out_conv");
        rel(up);
        tap(path, (size_t)Bn * Hf * Hf * F * e, 6 + (3 - k), "fusion -> tap");
    }

    // ---- head (dpt_depth.py:91-99): conv3x3, x2 bilinear, conv3x3, ReLU, conv1x1 (output channels padded to 8 for the GEMM), ReLU; NHWC -> NCHW ------
    MVE_CHECK(Hf == S / 2, MVE_ERR_STATE, "dpt plan: the decoder ends at %d, expected %d", Hf, S / 2);
    {
        Ref h0 = conv3(path, F, Hf, Hf, 1, 0, "h0.w", wt("h0.b"), F / 2, Ref(), "head.conv0 3x3");
        rel(path);
        Ref up = upsample(h0, Hf, F / 2, "head upsample x2 (align_corners)");
        rel(h0);
        Ref h2 = conv3(up, F / 2, S, S, 1, 0, "h2.w", wt("h2.b"), 32, Ref(), "head.conv2 3x3");
        rel(up);
        const size_t npx = (size_t)Bn * S * S;
        add_relu(h2, Ref(), h2, npx * 32, "relu");
        Ref h4 = conv1(h2, (int)npx, 32, "h4.w", wt("h4.b"), 8, "head.conv4 1x1");
        rel(h2);
        add_relu(h4, Ref(), h4, npx * 8, "relu");
        live(h4, "NHWC -> NCHW");
        op(OC_OTHER, 0, "NHWC -> NCHW", [=](const Run& r) { return mve_nhwc_to_nchw(d, d, r.p(h4), 8, Bn, NC, S, S, r.p(out), r.stream); });
        rel(h4);
    }
    pl.enc_end = pl.ops.size();
    pl.ws_bytes = ar.peak + 256;
    if (!u.err.empty()) { mve_set_error("dpt plan: %s", u.err.c_str()); u.err.clear(); return MVE_ERR_STATE; }
    return MVE_OK;
}

}  // namespace
