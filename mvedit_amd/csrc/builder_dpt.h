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

// parameter names and labels of Builder::encoder_layer in the packed ViT scheme of mvedit_amd/normal_model.py
constexpr Builder::EncoderNames DPT_ENCODER = {".n1", ".qkv", ".o", ".n2", ".fc1", ".fc2", "attn.qkv", "attn.proj+residual"};

int Builder::build_dpt(int B_) {
    const int S = c.dp_image, e = 2, Bn = B_, C = c.ch[0], I = c.dp_inter, F = c.dp_features;
    const int Gd = S / 16, G2 = Gd * Gd, T = G2 + 1, M = Bn * T, Cs = c.dp_stem, NC = c.out_ch;
    begin(B_, S, S, 1, c.dtype);
    const int d = dt;
    const float gn_eps = 1e-5f;      // BitGroupNormActivation's default
    MVE_CHECK((size_t)Bn * S * S * 32 < ((size_t)1 << 31) && (size_t)Bn * (S / 2) * (S / 2) * 152 < ((size_t)1 << 31) &&
                  (size_t)Bn * (S / 2) * (S / 2) * (size_t)(F > Cs ? F : Cs) < ((size_t)1 << 31) && (size_t)M * (size_t)(I > 3 * C ? I : 3 * C) < ((size_t)1 << 31),
              MVE_ERR_ARG, "dpt: batch %d overflows 32-bit activation indexing", Bn);
    const Ref px = arg(Ref::SAMPLE);
    auto norm = [&](Ref x, int Cx, int HW, const std::string& n, int act, const char* what) {      // GroupNorm (+ ReLU: selector 2) -> new buffer
        Ref y = ws((size_t)Bn * HW * Cx * e);
        gn(x, Cx, Ref(), 0, Bn, HW, gn_eps, wt(n + ".g"), wt(n + ".b"), act, y, what);
        return y;
    };

    // ---- stem: 7 x 7 / 2 "same" convolution as a GEMM over gathered rows, GroupNorm + ReLU, 3 x 3 / 2 "same" max-pool --------------------------
    int H = S / 2;
    Ref x;
    {
        Ref rows = ws((size_t)Bn * H * H * 152 * e);
        op(OC_OTHER, 0, "stem window rows", [=](const Run& r) { return mve_dpt_stem_rows(d, r.p(px), Bn, S, r.p(rows), 152, r.stream); });
        Ref s0 = conv1x1(rows, Bn * H * H, 152, "stem.w", Ref(), Cs, "stem.conv 7x7/2");
        rel(rows);
        Ref s1 = norm(s0, Cs, H * H, "stem", 2, "stem.norm+relu");
        rel(s0);
        x = ws((size_t)Bn * (H / 2) * (H / 2) * Cs * e);
        const int Hs = H;
        live(s1, "stem.maxpool"); live(x, "stem.maxpool");
        op(OC_OTHER, 0, "stem.maxpool 3x3/2", [=](const Run& r) { return mve_dpt_maxpool(d, r.p(s1), Bn, Hs, Hs, Cs, r.p(x), r.stream); });
        rel(s1);
        H /= 2;
        copy_out(x, (size_t)Bn * H * H * Cs * e, 0, "stem -> tap");
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
            Ref t1 = conv1x1(x, Bn * H * H, cin, b + ".c1.w", Ref(), mid, "bottleneck.conv1");
            Ref t1n = norm(t1, mid, H * H, b + ".n1", 2, "bottleneck.norm1+relu");
            rel(t1);
            Ref t2 = conv3x3(t1n, mid, Bn, H, H, stride, b + ".c2.w", Ref(), mid, Ref(), stride == 2 ? MVE_CONV_PAD_BR : 0, "bottleneck.conv2 3x3");
            rel(t1n);
            Ref t2n = norm(t2, mid, Ho * Ho, b + ".n2", 2, "bottleneck.norm2+relu");
            rel(t2);
            Ref t3 = conv1x1(t2n, Bn * Ho * Ho, mid, b + ".c3.w", Ref(), cout, "bottleneck.conv3");
            rel(t2n);
            Ref t3n = norm(t3, cout, Ho * Ho, b + ".n3", 0, "bottleneck.norm3");
            rel(t3);
            Ref sc = x;
            if (m == 0) {
                Ref xs = stride == 2 ? gather_s2(x, Bn, H, H, cin) : x;
                Ref ds = conv1x1(xs, Bn * Ho * Ho, cin, b + ".ds.w", Ref(), cout, "bottleneck.downsample.conv");
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
        copy_out(x, (size_t)Bn * H * H * cout * e, 1 + s, "stage -> tap");
    }

    // ---- the decoder's inputs from the two feature maps: layer1_rn / layer2_rn --------------------------------------------------------------------
    Ref rn[4];
    rn[0] = conv3x3(stage_out[0], c.dp_stage[0], Bn, stage_H[0], stage_H[0], 1, "rn1.w", Ref(), F, Ref(), 0, "layer1_rn");
    rel(stage_out[0]);
    rn[1] = conv3x3(stage_out[1], c.dp_stage[1], Bn, stage_H[1], stage_H[1], 1, "rn2.w", Ref(), F, Ref(), 0, "layer2_rn");
    rel(stage_out[1]);

    // ---- tokens: 1 x 1 projection of stage 3, class token + position table, pre-norm ViT blocks ---------------------------------------------------
    MVE_CHECK(H == Gd, MVE_ERR_STATE, "dpt plan: stage 3 is %d x %d, the token grid %d x %d", H, H, Gd, Gd);
    {
        Ref patch = conv1x1(x, Bn * G2, c.dp_stage[2], "proj.w", wt("proj.b"), C, "patch_embed.proj");
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
        act(ro, (size_t)Bn * G2 * C, MVE_ACT_GELU, "readout gelu");
        Ref p = conv1x1(ro, Bn * G2, C, r_ + ".p.w", wt(r_ + ".p.b"), N, "act_postprocess conv1x1");
        rel(ro);
        int Hp = Gd;
        if (which == 4) {
            Ref z = conv3x3(p, N, Bn, Gd, Gd, 2, "r4.z.w", wt("r4.z.b"), N, Ref(), 0, "act_postprocess4 conv3x3/2");
            rel(p); p = z; Hp = Gd / 2;
        }
        Ref y = conv3x3(p, N, Bn, Hp, Hp, 1, which == 3 ? "rn3.w" : "rn4.w", Ref(), F, Ref(), 0, which == 3 ? "layer3_rn" : "layer4_rn");
        rel(p);
        return y;
    };
    for (int k = 0; k <= c.dp_tap[1]; ++k) {
        x = encoder_layer(DPT_ENCODER, "l" + std::to_string(k), x, M, C, I, MVE_ACT_GELU, false);
        // the taps are block outputs: the backbone's final LayerNorm never reaches the prediction
        if (k == c.dp_tap[0]) { copy_out(x, (size_t)M * C * e, 4, "token tap 3 -> tap"); rn[2] = reassemble(x, 3); }
        if (k == c.dp_tap[1]) { copy_out(x, (size_t)M * C * e, 5, "token tap 4 -> tap"); rn[3] = reassemble(x, 4); }
    }
    rel(x);

    // ---- decoder: FeatureFusionBlock_custom x 4 (blocks.py:291-341), bn=False, ReLU(inplace=False), align_corners=True ----------------------------
    auto rcu = [&](const std::string& n, Ref xin, int Hf) {      // ResidualConvUnit_custom: conv2(relu(conv1(relu(x)))) + x
        const size_t nel = (size_t)Bn * Hf * Hf * F;
        Ref r0 = ws(nel * e);
        add_relu(xin, Ref(), r0, nel, "relu");
        Ref h = conv3x3(r0, F, Bn, Hf, Hf, 1, n + ".c1.w", wt(n + ".c1.b"), F, Ref(), 0, "resConfUnit.conv1");
        rel(r0);
        relu(h, nel, "relu");
        Ref y = conv3x3(h, F, Bn, Hf, Hf, 1, n + ".c2.w", wt(n + ".c2.b"), F, xin, 0, "resConfUnit.conv2+residual");
        rel(h);
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
        Ref up = upsample2x(o, Bn, Hf, Hf, F, "fusion upsample x2 (align_corners)");
        rel(o);
        Hf *= 2;
        path = conv1x1(up, Bn * Hf * Hf, F, f + ".out.w", wt(f + ".out.b"), F, "fusion out_conv");
        rel(up);
        copy_out(path, (size_t)Bn * Hf * Hf * F * e, 6 + (3 - k), "fusion -> tap");
    }

    // ---- head (dpt_depth.py:91-99): conv3x3, x2 bilinear, conv3x3, ReLU, conv1x1 (output channels padded to 8 for the GEMM), ReLU; NHWC -> NCHW ------
    MVE_CHECK(Hf == S / 2, MVE_ERR_STATE, "dpt plan: the decoder ends at %d, expected %d", Hf, S / 2);
    {
        Ref h0 = conv3x3(path, F, Bn, Hf, Hf, 1, "h0.w", wt("h0.b"), F / 2, Ref(), 0, "head.conv0 3x3");
        rel(path);
        Ref up = upsample2x(h0, Bn, Hf, Hf, F / 2, "head upsample x2 (align_corners)");
        rel(h0);
        Ref h2 = conv3x3(up, F / 2, Bn, S, S, 1, "h2.w", wt("h2.b"), 32, Ref(), 0, "head.conv2 3x3");
        rel(up);
        const size_t npx = (size_t)Bn * S * S;
        relu(h2, npx * 32, "relu");
        Ref h4 = conv1x1(h2, (int)npx, 32, "h4.w", wt("h4.b"), 8, "head.conv4 1x1");
        rel(h2);
        relu(h4, npx * 8, "relu");
        to_nchw(h4, d, 8, Bn, NC, S, S, "NHWC -> NCHW");
        rel(h4);
    }
    return finish("dpt");
}

}  // namespace
