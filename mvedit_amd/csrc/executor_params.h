// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): slab layout of the packed parameters
// (every network mode).  The layout is the ONLY description of a parameter: the call that reserves a slot also records, under the state-dict name
// that fills it, where the tensor goes and how it is packed (Unet::sources); load_param at the end of the file only looks the name up.
#pragma once
#include "executor.h"

namespace {

// [N][K] rows as they come, to rows `dst_stride` apart; mul: applied in fp32 before the single rounding
PackDims pack_rows(long long N, long long K, long long dst_stride, float mul = 1.0f) {
    PackDims d{{1, 1, N, K}, {0, 0, K, 1}, {0, 0, dst_stride, 1}, K};
    d.mul = mul;
    return d;
}
PackDims pack_flat(long long n) { return pack_rows(1, n, n); }

// OIHW -> [O][3][3][Ipad], or with I a multiple of 64 the channel-slab-major K order [O][I/64][9][64] (MVE_CONV_W_CHUNK64); row: the destination
// row length when the row also holds a fused shortcut behind the 9 * I columns (0: 9 * I)
PackDims pack_conv(long long O, long long I, long long Ipad, long long row = 0) {
    if (I % 64 == 0 && Ipad == I) return PackDims{{O, I / 64, 9, 64}, {I * 9, 64 * 9, 1, 9}, {row ? row : 9 * I, 9 * 64, 64, 1}, 64};
    return PackDims{{O, 3, 3, Ipad}, {I * 9, 3, 1, 9}, {9 * Ipad, 3 * Ipad, Ipad, 1}, I};
}

int g_fuse_shortcut = 1;     // engines created afterwards fold conv_shortcut into conv2 (mve_unet_tune; A/B measurements)

// ---------------------------------------------------------------------------------------------------
// parameter layout: reserve slab space for every packed tensor and record the state-dict tensors that fill it
// ---------------------------------------------------------------------------------------------------
struct SlabBuilder {
    Unet& u;
    size_t top = 0;
    const Config& c = u.cfg;

    // reserve a slot
    void add(const std::string& slot, size_t elems, bool f32, float q_fold = 0.f) {
        Param p;
        p.off = top; p.f32 = f32; p.bytes = elems * (f32 ? 4 : 2); p.q_fold = q_fold;
        top += (p.bytes + 255) & ~(size_t)255;
        u.params[slot] = p;
    }
    // record the tensor `from` (n elements) that `d` packs into `slot` from element `off` on; required tensors join `expected` in layout order
    Source& part(const std::string& slot, size_t off, const std::string& from, size_t n, const PackDims& d, bool required = true) {
        Source& s = u.sources[from];
        s.numel = (long long)n; s.optional = !required;
        s.steps.push_back({slot, off, 0, d});
        if (required) u.expected.push_back(from);
        return s;
    }

    // a slot and the one tensor that fills it ---------------------------------------------------------
    // a tensor that leaves part of its slot uncovered (padded: the slot's size when larger than n; Opad / Ipad below) clears the slot first
    Source& vec(const std::string& slot, const std::string& from, size_t n, bool f32 = true, size_t padded = 0) {
        add(slot, padded ? padded : n, f32);
        Source& s = part(slot, 0, from, n, pack_flat(n));
        s.zero = padded && padded != n;
        return s;
    }
    // q_fold > 0: a to_q weight.  Its rows carry softmax_scale * log2(e) = head_dim^-1/2 * log2(e), so the attention kernel works in log2 units
    // without a multiply per logit (mve_attention_prescaled); the factor is recorded on the slot (Builder::attn requires it) and applied here.
    Source& mat(const std::string& slot, const std::string& from, size_t N, size_t K, float q_fold = 0.f) {
        add(slot, N * K, false, q_fold);
        return part(slot, 0, from, N * K, pack_rows(N, K, K, q_fold > 0.f ? q_fold : 1.0f));
    }
    // 3 x 3 convolution [O, I, 3, 3] into Opad rows of 9 * Ipad (+ tail: the columns of a fused shortcut) elements
    Source& conv(const std::string& slot, const std::string& from, size_t O, size_t I, size_t Opad, size_t Ipad, size_t tail = 0) {
        add(slot, Opad * (9 * Ipad + tail), false);
        Source& s = part(slot, 0, from, O * I * 9, pack_conv(O, I, Ipad, tail ? 9 * Ipad + tail : 0));
        s.conv[0] = (long long)O; s.conv[1] = (long long)I;
        s.zero = Opad != O || Ipad != I;
        return s;
    }
    Source& conv(const std::string& slot, const std::string& from, size_t O, size_t I) { return conv(slot, from, O, I, O, I); }
    // `<p>.weight|bias` -> `<p>.g|b` (fp32) / `<p>.w|b`; from: the state-dict prefix when it differs from the slots'
    void norm(const std::string& p, size_t C, const std::string& from = "") {
        const std::string& f = from.empty() ? p : from;
        vec(p + ".g", f + ".weight", C);
        vec(p + ".b", f + ".bias", C);
    }
    void linear(const std::string& p, size_t rows, size_t cols, const std::string& from = "") {
        const std::string& f = from.empty() ? p : from;
        mat(p + ".w", f + ".weight", rows, cols);
        vec(p + ".b", f + ".bias", rows);
    }
    void conv_bias(const std::string& p, size_t O, size_t I) {
        conv(p + ".w", p + ".weight", O, I);
        vec(p + ".b", p + ".bias", O);
    }
    // DPT / LoFTR: engine-side names, the Python side hands over a flat tensor of the slot's size
    void w16(const std::string& n, size_t elems) { add(n, elems, false); part(n, 0, n, elems, pack_flat(elems)); }
    void f32(const std::string& n, size_t elems) { add(n, elems, true); part(n, 0, n, elems, pack_flat(elems)); }

    // blocks -----------------------------------------------------------------------------------------
    // transformers' CLIP encoder layers of `tower` (text_model / vision_model): q_proj / k_proj / v_proj share one [3C, C] matrix and one [3C]
    // bias (one GEMM per layer)
    void clip_layers(const std::string& tower) {
        const size_t C = c.ch[0], I = c.clip_inter;
        for (int k = 0; k < c.layers_per_block; ++k) {
            const std::string b = tower + ".encoder.layers." + std::to_string(k), a = b + ".self_attn.";
            norm(b + ".layer_norm1", C);
            add(a + "qkv.w", 3 * C * C, false);
            add(a + "qkv.b", 3 * C, true);
            int j = 0;
            for (const char* pj : {"q_proj", "k_proj", "v_proj"}) {
                part(a + "qkv.w", j * C * C, a + pj + ".weight", C * C, pack_rows(C, C, C));
                part(a + "qkv.b", j * C, a + pj + ".bias", C, pack_flat(C));
                ++j;
            }
            linear(a + "out_proj", C, C);
            norm(b + ".layer_norm2", C);
            linear(b + ".mlp.fc1", I, C);
            linear(b + ".mlp.fc2", C, I);
        }
    }
    // diffusers ResnetBlock2D; time_emb_proj of every resnet is a row block of ONE matrix (temb_proj.w / .b, reserved by the caller: one GEMM per
    // forward); with all widths multiples of 64 conv_shortcut is the tail columns of conv2's rows (fuse_sc)
    void resnet(const ResnetDesc& r, bool time_embedding) {
        const size_t ci = r.cin, co = r.cout, T = c.temb_dim();
        const std::string& p = r.name;
        norm(p + ".norm1", ci);
        conv_bias(p + ".conv1", co, ci);
        if (time_embedding) {
            part("temb_proj.w", u.temb_off[p] * T, p + ".time_emb_proj.weight", co * T, pack_rows(co, T, T));
            part("temb_proj.b", u.temb_off[p], p + ".time_emb_proj.bias", co, pack_flat(co));
        }
        norm(p + ".norm2", co);
        const bool sc = ci != co;
        const size_t tail = sc && u.fuse_sc ? ci : 0;
        conv(p + ".conv2.w", p + ".conv2.weight", co, co, co, co, tail);
        vec(p + ".conv2.b", p + ".conv2.bias", co);
        if (!sc) return;
        if (u.fuse_sc) part(p + ".conv2.w", 9 * co, p + ".conv_shortcut.weight", co * ci, pack_rows(co, ci, 9 * co + ci));
        else mat(p + ".sc.w", p + ".conv_shortcut.weight", co, ci);
        vec(p + ".sc.b", p + ".conv_shortcut.bias", co);
    }
    // diffusers Transformer2DModel; attn2's to_k / to_v of every layer are row blocks of ONE matrix over the context (ctx_kv.w, and ip_kv.w for
    // the IP-Adapter's optional to_k_ip / to_v_ip; reserved by the caller, offsets in kv_off)
    void transformer(const XfDesc& x) {
        const size_t C = x.c, X = c.ctx_dim;
        norm(x.name + ".norm", C);
        linear(x.name + ".proj_in", C, C);          // [C, C] or [C, C, 1, 1]
        linear(x.name + ".proj_out", C, C);
        for (int k = 0; k < x.layers; ++k) {
            const std::string b = x.name + ".transformer_blocks." + std::to_string(k);
            for (const char* nn : {".norm1", ".norm2", ".norm3"}) norm(b + nn, C);
            const float qf = 1.4426950408889634f / sqrtf((float)(C / x.heads));
            add(b + ".qkv.w", 3 * C * C, false, qf);
            part(b + ".qkv.w", 0, b + ".attn1.to_q.weight", C * C, pack_rows(C, C, C, qf));
            part(b + ".qkv.w", C * C, b + ".attn1.to_k.weight", C * C, pack_rows(C, C, C));
            part(b + ".qkv.w", 2 * C * C, b + ".attn1.to_v.weight", C * C, pack_rows(C, C, C));
            linear(b + ".o1", C, C, b + ".attn1.to_out.0");
            mat(b + ".q2.w", b + ".attn2.to_q.weight", C, C, qf);
            const size_t kv = u.kv_off[b];
            part("ctx_kv.w", kv * X, b + ".attn2.to_k.weight", C * X, pack_rows(C, X, X));
            part("ctx_kv.w", (kv + C) * X, b + ".attn2.to_v.weight", C * X, pack_rows(C, X, X));
            part("ip_kv.w", kv * X, b + ".attn2.processor.to_k_ip.weight", C * X, pack_rows(C, X, X), false);
            part("ip_kv.w", (kv + C) * X, b + ".attn2.processor.to_v_ip.weight", C * X, pack_rows(C, X, X), false);
            linear(b + ".o2", C, C, b + ".attn2.to_out.0");
            // GEGLU: rows [0, 4C) = value, [4C, 8C) = gate  ->  interleaved (value_i, gate_i)
            const long long h = 4 * C, K = C;
            add(b + ".ff1.w", 8 * C * C, false);
            part(b + ".ff1.w", 0, b + ".ff.net.0.proj.weight", 8 * C * C, PackDims{{1, 2, h, K}, {0, h * K, K, 1}, {0, K, 2 * K, 1}, K});
            add(b + ".ff1.b", 8 * C, true);
            part(b + ".ff1.b", 0, b + ".ff.net.0.proj.bias", 8 * C, PackDims{{1, 1, 2, h}, {0, 0, h, 1}, {0, 0, 1, 2}, h});
            linear(b + ".ff2", C, 4 * C, b + ".ff.net.2");
        }
    }
    // Downsample2D / Upsample2D conv; phases: also the summed taps of the four 2 x 2 phase convs (mve_upsample_conv_phases)
    void resample(const std::string& p, size_t C, bool phases) {
        Source& s = conv(p + ".w", p + ".weight", C, C);
        if (phases) {
            add(p + ".w4", C * 16 * C, false);
            PackStep w4{p + ".w4"};
            w4.phase4 = true;
            s.steps.push_back(w4);
        }
        vec(p + ".b", p + ".bias", C);
    }
};

void layout_params(Unet& u) {
    const Config& c = u.cfg;
    SlabBuilder sb{u};
    std::vector<ResnetDesc> rs;
    std::vector<XfDesc> xs;
    enumerate(c, rs, xs);
    u.fuse_sc = g_fuse_shortcut != 0;
    for (int i = 0; i < c.n_levels; ++i) u.fuse_sc = u.fuse_sc && (c.ch[i] % 64 == 0);
    const auto num = [](int k) { return std::to_string(k); };
    switch (c.kind) {
    case Kind::Lpips: {
        // every VGG conv twice: forward packing and the transposed / flipped packing that turns the same kernel into its dgrad.  The dgrad weight
        // as a conv weight: W'[o' = ci][i' = co][ky][kx] = W[co][ci][2-ky][2-kx]; co is always a multiple of 64, so the slab-major layout
        // [O'][I'/64][9][64]; source offset of (o', slab, tap, c) = (slab*64 + c)*ci*9 + o'*9 + (8 - tap): the 8 is the step's source offset, the
        // tap stride is -1.  conv1_1: 3 real input channels / dgrad rows, padded to 8 (the rest stay zero).
        for (int i = 0; i < 13; ++i) {
            const std::string n = vgg_name(i), e = "vgg." + num(i);
            const long long ci = VGG_CIN[i], co = VGG_COUT[i], cp = i == 0 ? 8 : ci;
            Source& s = sb.conv(e + ".w", n + ".weight", co, ci, co, cp);
            sb.add(e + ".wt", cp * 9 * co, false);
            s.steps.push_back({e + ".wt", 0, 8, PackDims{{ci, co / 64, 9, 64}, {9, 64 * ci * 9, -1, ci * 9}, {9 * co, 9 * 64, 64, 1}, 64}});
            sb.vec(e + ".b", n + ".bias", co);
        }
        for (int k = 0; k < 5; ++k) sb.vec("lin." + num(k), "lin" + num(k) + ".model.1.weight", VGG_COUT[VGG_BLK_FIRST[k + 1] - 1]);
        sb.vec("shift", "scaling_layer.shift", 3, true, 8);
        sb.vec("scale", "scaling_layer.scale", 3, true, 8);
        sb.add("zeros", 512, true);          // ReLU = PReLU with zero slopes (the slab is zero-filled when it is allocated)
        break;
    }
    case Kind::ClipText: {
        const size_t C = c.ch[0];
        const std::string em = "text_model.embeddings.";
        sb.mat(em + "token_embedding.w", em + "token_embedding.weight", c.clip_vocab, C);
        sb.mat(em + "position_embedding.w", em + "position_embedding.weight", c.clip_max_pos, C);
        sb.clip_layers("text_model");
        sb.norm("text_model.final_layer_norm", C);
        if (c.clip_proj) sb.mat("text_projection.w", "text_projection.weight", c.clip_proj, C);
        break;
    }
    case Kind::ClipVision: {
        // the patch convolution's weight [C, 3, P, P] becomes [C][Kp]: (channel, ky, kx) columns, zero-padded from 3 * P * P to a multiple of 8
        // by the packing kernel itself (mve_clip_patchify lays out the matching operand rows)
        const size_t C = c.ch[0], PP3 = 3 * (size_t)c.cv_patch * c.cv_patch, Kp = (PP3 + 7) / 8 * 8, G = c.cv_image / c.cv_patch;
        const std::string em = "vision_model.embeddings.";
        sb.vec(em + "class_embedding", em + "class_embedding", C, false);
        sb.add(em + "patch_embedding.w", C * Kp, false);
        sb.part(em + "patch_embedding.w", 0, em + "patch_embedding.weight", C * PP3, PackDims{{1, 1, (long long)C, (long long)Kp}, {0, 0, (long long)PP3, 1}, {0, 0, (long long)Kp, 1}, (long long)PP3});
        sb.mat(em + "position_embedding.w", em + "position_embedding.weight", G * G + 1, C);
        sb.norm("vision_model.pre_layrnorm", C);
        sb.clip_layers("vision_model");
        sb.norm("vision_model.post_layernorm", C);
        if (c.clip_proj) sb.mat("visual_projection.w", "visual_projection.weight", c.clip_proj, C);
        break;
    }
    case Kind::Sam: {
        // transformers' SamVisionEncoder names (mvedit_amd/sam.py renames segment_anything's keys onto them).  The patch convolution's weight
        // [C, 3, P, P] becomes [C][Kp] as for the CLIP tower; pos_embed and the relative-position tables stay in the engine dtype ([G*G][C],
        // [2n-1][head_dim] with n = window_size, or the grid in a global block: a table of another length would need the reference's linear
        // interpolation and fails the loader's element count); the neck's 3 x 3 weight in the conv's K order.
        const size_t C = c.ch[0], I = c.clip_inter, O = c.sm_out, PP3 = 3 * (size_t)c.sm_patch * c.sm_patch, Kp = (PP3 + 7) / 8 * 8, G = c.sm_image / c.sm_patch;
        const size_t hd = C / c.heads[0];
        sb.add("patch_embed.projection.w", C * Kp, false);
        sb.part("patch_embed.projection.w", 0, "patch_embed.projection.weight", C * PP3,
                PackDims{{1, 1, (long long)C, (long long)Kp}, {0, 0, (long long)PP3, 1}, {0, 0, (long long)Kp, 1}, (long long)PP3});
        sb.vec("patch_embed.projection.b", "patch_embed.projection.bias", C);
        sb.vec("pos_embed", "pos_embed", G * G * C, false);
        for (int k = 0; k < c.layers_per_block; ++k) {
            const std::string b = "layers." + num(k);
            const size_t n = (c.sm_global >> k) & 1ull ? G : (size_t)c.sm_window;
            sb.norm(b + ".layer_norm1", C);
            sb.linear(b + ".attn.qkv", 3 * C, C);
            sb.vec(b + ".attn.rel_pos_h", b + ".attn.rel_pos_h", (2 * n - 1) * hd, false);
            sb.vec(b + ".attn.rel_pos_w", b + ".attn.rel_pos_w", (2 * n - 1) * hd, false);
            sb.linear(b + ".attn.proj", C, C);
            sb.norm(b + ".layer_norm2", C);
            sb.linear(b + ".mlp.lin1", I, C);
            sb.linear(b + ".mlp.lin2", C, I);
        }
        sb.mat("neck.conv1.w", "neck.conv1.weight", O, C);
        sb.norm("neck.layer_norm1", O);
        sb.conv("neck.conv2.w", "neck.conv2.weight", O, O);
        sb.norm("neck.layer_norm2", O);
        break;
    }
    case Kind::SamDecoder: {
        // the names `SamModel.state_dict()` prints (mvedit_amd/sam.py renames segment_anything's keys onto them).  EVERY slot is fp32 (vec()'s
        // default): the slab carries fp32 slots next to 16-bit ones for every kind, so nothing changes for the others.  Linear weights stay [out][in].
        // A ConvTranspose2d weight [Cin][Cout][2][2] becomes the GEMM operand [(2 ky + kx) Cout + co][Cin] of mve_sam_upscale.  The Mt hypernetwork
        // MLPs and the iou head are stacked, the iou head last, in the three slots mve_sam_token_mlps reads (`mlps.w0 / w1 / w2` and biases; the iou
        // head's proj_out fills the first Mt of its C / 8 rows, the rest stay zero).  `dense_pe` has no state-dict tensor: mve_sam_decoder_finalize
        // computes it from the gaussian matrix.
        const size_t C = c.ch[0], I = c.clip_inter, Mt = c.sd_masks, G = c.sd_grid, C4 = C / 4, C8 = C / 8, Ci = C / 2;
        const std::string pe = "prompt_encoder.", md = "mask_decoder.", tf = md + "transformer.";
        auto lin = [&](const std::string& p, size_t rows, size_t cols) { sb.vec(p + ".w", p + ".weight", rows * cols); sb.vec(p + ".b", p + ".bias", rows); };
        auto attention = [&](const std::string& p, size_t inner) {
            for (const char* pj : {".q_proj", ".k_proj", ".v_proj"}) lin(p + pj, inner, C);
            lin(p + ".out_proj", C, inner);
        };
        sb.vec("gaussian", "shared_image_embedding.positional_embedding", C);
        sb.add("dense_pe", G * G * C, true);
        sb.add("point_embed", 4 * C, true);
        for (int k = 0; k < 4; ++k) sb.part("point_embed", k * C, pe + "point_embed." + num(k) + ".weight", C, pack_flat(C));
        sb.vec("not_a_point", pe + "not_a_point_embed.weight", C);
        sb.vec("no_mask", pe + "no_mask_embed.weight", C);
        sb.vec("iou_token", md + "iou_token.weight", C);
        sb.vec("mask_tokens", md + "mask_tokens.weight", Mt * C);
        for (int k = 0; k < c.layers_per_block; ++k) {
            const std::string b = tf + "layers." + num(k);
            attention(b + ".self_attn", C);
            sb.norm(b + ".layer_norm1", C);
            attention(b + ".cross_attn_token_to_image", Ci);
            sb.norm(b + ".layer_norm2", C);
            lin(b + ".mlp.lin1", I, C);
            lin(b + ".mlp.lin2", C, I);
            sb.norm(b + ".layer_norm3", C);
            attention(b + ".cross_attn_image_to_token", Ci);
            sb.norm(b + ".layer_norm4", C);
        }
        attention(tf + "final_attn_token_to_image", Ci);
        sb.norm(tf + "layer_norm_final_attn", C);
        const size_t cin[2] = {C, C4}, cout[2] = {C4, C8};
        for (int k = 0; k < 2; ++k) {
            const std::string u2 = md + "upscale_conv" + num(k + 1);
            const long long ci = (long long)cin[k], co = (long long)cout[k];
            sb.add(u2 + ".w", 4 * co * ci, true);
            sb.part(u2 + ".w", 0, u2 + ".weight", 4 * co * ci, PackDims{{1, 4, co, ci}, {0, 1, 4, co * 4}, {0, co * ci, ci, 1}, ci});
            sb.vec(u2 + ".b", u2 + ".bias", co);
        }
        sb.norm(md + "upscale_layer_norm", C4);
        sb.add("mlps.w0", (Mt + 1) * C * C, true); sb.add("mlps.b0", (Mt + 1) * C, true);
        sb.add("mlps.w1", (Mt + 1) * C * C, true); sb.add("mlps.b1", (Mt + 1) * C, true);
        sb.add("mlps.w2", (Mt + 1) * C8 * C, true); sb.add("mlps.b2", (Mt + 1) * C8, true);
        for (size_t j = 0; j <= Mt; ++j) {
            const std::string m = j < Mt ? md + "output_hypernetworks_mlps." + num((int)j) : md + "iou_prediction_head";
            const size_t no = j < Mt ? C8 : Mt;
            sb.part("mlps.w0", j * C * C, m + ".proj_in.weight", C * C, pack_flat(C * C)); sb.part("mlps.b0", j * C, m + ".proj_in.bias", C, pack_flat(C));
            sb.part("mlps.w1", j * C * C, m + ".layers.0.weight", C * C, pack_flat(C * C)); sb.part("mlps.b1", j * C, m + ".layers.0.bias", C, pack_flat(C));
            sb.part("mlps.w2", j * C8 * C, m + ".proj_out.weight", no * C, pack_flat(no * C)); sb.part("mlps.b2", j * C8, m + ".proj_out.bias", no, pack_flat(no));
        }
        break;
    }
    case Kind::Loftr: {
        // Engine-side slot names (mvedit_amd/matcher.py maps the checkpoint's keys onto them: BatchNorm folded into the convolution in front of it,
        // the 196-wide stage padded to 200 channels with zeros, k | v concatenated, conv K order): the loader converts a tensor of the slot's size.
        const size_t Wd[3] = {128, 200, 256};
        sb.w16("stem.w", 128 * 56); sb.f32("stem.b", 128);
        size_t cin = 128;
        for (int s = 0; s < 3; ++s) {
            const size_t co = Wd[s];
            for (int m = 0; m < 2; ++m) {
                const std::string b = "l" + num(s + 1) + ".b" + num(m);
                sb.w16(b + ".c1.w", co * 9 * (m == 0 ? cin : co)); sb.f32(b + ".c1.b", co);
                sb.w16(b + ".c2.w", co * 9 * co); sb.f32(b + ".c2.b", co);
                if (m == 0 && s > 0) { sb.w16(b + ".ds.w", co * cin); sb.f32(b + ".ds.b", co); }
            }
            cin = co;
        }
        sb.w16("l3oc.w", 256 * 256); sb.w16("l2oc.w", 256 * 200); sb.w16("l1oc.w", 200 * 128);
        sb.w16("l2oc2.0.w", 256 * 9 * 256); sb.f32("l2oc2.0.b", 256); sb.w16("l2oc2.3.w", 200 * 9 * 256);
        sb.w16("l1oc2.0.w", 200 * 9 * 200); sb.f32("l1oc2.0.b", 200); sb.w16("l1oc2.3.w", 128 * 9 * 200);
        for (int t = 0; t < 2; ++t) {
            const size_t C = t == 0 ? 256 : 128;
            for (int k = 0; k < (t == 0 ? 8 : 2); ++k) {
                const std::string b = (t == 0 ? "c" : "f") + num(k);
                sb.w16(b + ".q.w", C * C); sb.w16(b + ".kv.w", 2 * C * C); sb.w16(b + ".merge.w", C * C);
                sb.w16(b + ".mlp0.w", 4 * C * C); sb.w16(b + ".mlp2.w", 2 * C * C);
                sb.f32(b + ".n1.g", C); sb.f32(b + ".n1.b", C); sb.f32(b + ".n2.g", C); sb.f32(b + ".n2.b", C);
            }
        }
        sb.w16("dp.w", 128 * 256); sb.f32("dp.b", 128); sb.w16("mf.w", 128 * 256); sb.f32("mf.b", 128);
        break;
    }
    case Kind::Dpt: {
        // Engine-side slot names: the Python side (mvedit_amd/normal_model.py) maps the checkpoint's keys onto them and does every transformation
        // that is more than a copy -- weight standardisation, q|k|v concatenation, the readout's token / class halves, the conv K order, padding --
        // so the loader only converts a tensor of the slot's size (16-bit slots in the engine dtype, fp32 slots as they are).
        auto gnorm = [&](const std::string& n, size_t C) { sb.f32(n + ".g", C); sb.f32(n + ".b", C); };
        const size_t C = c.ch[0], I = c.dp_inter, F = c.dp_features, Gd = c.dp_image / 16, Cs = c.dp_stem;
        sb.w16("stem.w", Cs * 152); gnorm("stem", Cs);
        size_t cin = Cs;
        for (int s = 0; s < 3; ++s) {
            const size_t cout = c.dp_stage[s], mid = cout / 4;
            for (int m = 0; m < c.dp_depth[s]; ++m) {
                const std::string b = "s" + num(s) + ".b" + num(m);
                sb.w16(b + ".c1.w", mid * cin); gnorm(b + ".n1", mid);
                sb.w16(b + ".c2.w", mid * 9 * mid); gnorm(b + ".n2", mid);
                sb.w16(b + ".c3.w", cout * mid); gnorm(b + ".n3", cout);
                if (m == 0) { sb.w16(b + ".ds.w", cout * cin); gnorm(b + ".dn", cout); }
                cin = cout;
            }
        }
        sb.w16("proj.w", C * cin); sb.f32("proj.b", C);
        sb.w16("cls", C); sb.w16("pos", (Gd * Gd + 1) * C);
        for (int k = 0; k <= c.dp_tap[1]; ++k) {
            const std::string b = "l" + num(k);
            gnorm(b + ".n1", C);
            sb.w16(b + ".qkv.w", 3 * C * C); sb.f32(b + ".qkv.b", 3 * C);
            sb.w16(b + ".o.w", C * C); sb.f32(b + ".o.b", C);
            gnorm(b + ".n2", C);
            sb.w16(b + ".fc1.w", I * C); sb.f32(b + ".fc1.b", I);
            sb.w16(b + ".fc2.w", C * I); sb.f32(b + ".fc2.b", C);
        }
        for (int k = 0; k < 2; ++k) {
            const std::string r = k == 0 ? "r3" : "r4";
            const size_t N = c.dp_neck[k];
            sb.w16(r + ".wt", C * C); sb.w16(r + ".wc", C * C); sb.f32(r + ".b", C);
            sb.w16(r + ".p.w", N * C); sb.f32(r + ".p.b", N);
            if (k == 1) { sb.w16("r4.z.w", N * 9 * N); sb.f32("r4.z.b", N); }
        }
        sb.w16("rn1.w", F * 9 * c.dp_stage[0]); sb.w16("rn2.w", F * 9 * c.dp_stage[1]); sb.w16("rn3.w", F * 9 * c.dp_neck[0]); sb.w16("rn4.w", F * 9 * c.dp_neck[1]);
        for (int k = 1; k <= 4; ++k) {
            const std::string f = "f" + num(k);
            for (const char* un : {".u1", ".u2"}) {
                if (k == 4 && std::string(un) == ".u1") continue;       // refinenet4 has one input: its resConfUnit1 never runs
                sb.w16(f + un + ".c1.w", F * 9 * F); sb.f32(f + un + ".c1.b", F);
                sb.w16(f + un + ".c2.w", F * 9 * F); sb.f32(f + un + ".c2.b", F);
            }
            sb.w16(f + ".out.w", F * F); sb.f32(f + ".out.b", F);
        }
        sb.w16("h0.w", (F / 2) * 9 * F); sb.f32("h0.b", F / 2);
        sb.w16("h2.w", 32 * 9 * (F / 2)); sb.f32("h2.b", 32);
        sb.w16("h4.w", 8 * 32); sb.f32("h4.b", 8);          // num_channels rows, zero-padded to the GEMM's 8
        break;
    }
    case Kind::Resampler: {
        // the reference's state_dict() names; Linear weights as they come ([out][in]), LayerNorm affine parameters and biases in fp32
        const size_t D = c.ch[0], inner = (size_t)c.heads[0] * 64, F = c.rs_inner, E = c.rs_embed, O = c.rs_out, Q = c.rs_queries;
        sb.mat("latents", "latents", Q, D);
        sb.linear("proj_in", D, E);
        for (int k = 0; k < c.layers_per_block; ++k) {
            const std::string a = "layers." + num(k) + ".0", f = "layers." + num(k) + ".1";
            sb.norm(a + ".norm1", D);
            sb.norm(a + ".norm2", D);
            sb.mat(a + ".to_q.w", a + ".to_q.weight", inner, D);
            sb.mat(a + ".to_kv.w", a + ".to_kv.weight", 2 * inner, D);
            sb.mat(a + ".to_out.w", a + ".to_out.weight", D, inner);
            sb.norm(f + ".0", D);
            sb.mat(f + ".1.w", f + ".1.weight", F, D);
            sb.mat(f + ".3.w", f + ".3.weight", D, F);
        }
        sb.linear("proj_out", O, D);
        sb.norm("norm_out", O);
        break;
    }
    case Kind::Srvgg: {
        // body.0: conv in_ch -> F; body.(2k), k = 1..num_conv: conv F -> F; body.(2k+1): PReLU slopes; last: conv F -> out_ch * r * r, its rows
        // padded to a multiple of 8
        const size_t F = c.ch[0], nout = (size_t)c.out_ch * c.sr_scale * c.sr_scale, opad = (nout + 7) & ~(size_t)7;
        const int last = 2 * (c.layers_per_block + 1);
        for (int k = 0; k <= c.layers_per_block + 1; ++k) {
            const std::string b = "body." + num(2 * k);
            const bool end = 2 * k == last;
            sb.conv(b + ".w", b + ".weight", end ? nout : F, k == 0 ? c.in_ch : F, end ? opad : F, k == 0 ? 8 : F);
            sb.vec(b + ".b", b + ".bias", end ? nout : F, true, end ? opad : F);
            if (!end) sb.vec("body." + num(2 * k + 1) + ".a", "body." + num(2 * k + 1) + ".weight", F);
        }
        break;
    }
    case Kind::VaeDecoder: case Kind::VaeEncoder: {
        // names are the half's own (mve_unet_load_param strips `decoder.` / `encoder.`; (post_)quant_conv is `pq_conv`: 1x1 over <= 8 channels,
        // zero-padded to 8 x 8)
        const bool dec = c.kind == Kind::VaeDecoder;
        const int n = c.n_levels;
        const size_t C = c.ch[n - 1], Cin0 = dec ? C : c.ch[0], Cout0 = dec ? c.ch[0] : C, nq = dec ? c.in_ch : c.out_ch;
        sb.add("pq_conv.w", 8 * 8, false);
        sb.part("pq_conv.w", 0, "pq_conv.weight", nq * nq, pack_rows(nq, nq, 8)).zero = true;
        sb.vec("pq_conv.b", "pq_conv.bias", nq, true, 8);
        sb.conv("conv_in.w", "conv_in.weight", Cin0, c.in_ch, Cin0, 8);
        sb.vec("conv_in.b", "conv_in.bias", Cin0);
        for (auto& r : rs) sb.resnet(r, false);
        // the mid block's single-head attention: to_q | to_k share one [2C, C] matrix
        const std::string a = "mid_block.attentions.0";
        sb.norm(a + ".group_norm", C);
        sb.add(a + ".qk.w", 2 * C * C, false);
        sb.part(a + ".qk.w", 0, a + ".to_q.weight", C * C, pack_rows(C, C, C));
        sb.part(a + ".qk.w", C * C, a + ".to_k.weight", C * C, pack_rows(C, C, C));
        sb.add(a + ".qk.b", 2 * C, true);
        sb.part(a + ".qk.b", 0, a + ".to_q.bias", C, pack_flat(C));
        sb.part(a + ".qk.b", C, a + ".to_k.bias", C, pack_flat(C));
        sb.linear(a + ".v", C, C, a + ".to_v");
        sb.linear(a + ".o", C, C, a + ".to_out.0");
        for (int i = 0; i + 1 < n; ++i) {
            const size_t Cs = dec ? c.ch[n - 1 - i] : c.ch[i];
            sb.resample((dec ? "up_blocks." + num(i) + ".upsamplers" : "down_blocks." + num(i) + ".downsamplers") + ".0.conv", Cs, dec && Cs % 64 == 0);
        }
        sb.norm("norm_out", Cout0, "conv_norm_out");
        sb.conv("conv_out.w", "conv_out.weight", c.out_ch, Cout0, 8, Cout0);
        sb.vec("conv_out.b", "conv_out.bias", c.out_ch, true, 8);
        break;
    }
    case Kind::UNet: case Kind::ControlNet: {
        const bool controlnet = c.kind == Kind::ControlNet;
        const size_t T = c.temb_dim(), C0 = c.ch[0];
        sb.conv("conv_in.w", "conv_in.weight", C0, c.in_ch, C0, 8);
        sb.vec("conv_in.b", "conv_in.bias", C0);
        sb.mat("time.w1", "time_embedding.linear_1.weight", T, C0);
        sb.vec("time.b1", "time_embedding.linear_1.bias", T);
        sb.mat("time.w2", "time_embedding.linear_2.weight", T, T);
        sb.vec("time.b2", "time_embedding.linear_2.bias", T);
        u.sum_temb = 0;
        for (auto& r : rs) { u.temb_off[r.name] = u.sum_temb; u.sum_temb += r.cout; }
        sb.add("temb_proj.w", (size_t)u.sum_temb * T, false);
        sb.add("temb_proj.b", u.sum_temb, true);
        for (auto& r : rs) sb.resnet(r, true);
        u.sum_kv = 0;
        for (auto& x : xs)
            for (int k = 0; k < x.layers; ++k) {
                u.kv_off[x.name + ".transformer_blocks." + num(k)] = u.sum_kv;
                u.sum_kv += 2 * x.c;
            }
        sb.add("ctx_kv.w", (size_t)u.sum_kv * c.ctx_dim, false);
        sb.add("ip_kv.w", (size_t)u.sum_kv * c.ctx_dim, false);      // IP-Adapter to_k_ip / to_v_ip, same column layout (optional weights)
        u.n_xf_layers = (int)u.kv_off.size();
        for (auto& x : xs) sb.transformer(x);
        for (int i = 0; i + 1 < c.n_levels; ++i) {
            sb.resample("down_blocks." + num(i) + ".downsamplers.0.conv", c.ch[i], false);
            if (controlnet) continue;
            const size_t Cu = c.ch[c.n_levels - 1 - i];
            sb.resample("up_blocks." + num(i) + ".upsamplers.0.conv", Cu, Cu % 64 == 0);
        }
        if (!controlnet) {
            sb.norm("norm_out", C0, "conv_norm_out");
            sb.conv("conv_out.w", "conv_out.weight", c.out_ch, C0, 8, C0);
            sb.vec("conv_out.b", "conv_out.bias", c.out_ch, true, 8);
            break;
        }
        // controlnet_cond_embedding: conv_in (cond_ch -> 16), blocks (16->16, 16->32 s2, 32->32, 32->96 s2, 96->96, 96->256 s2),
        // conv_out (256 -> ch[0]); controlnet_down_blocks.k / controlnet_mid_block: 1x1 "zero" convolutions
        const std::string e = "controlnet_cond_embedding.";
        sb.conv(e + "conv_in.w", e + "conv_in.weight", CN_EMB[0], c.cond_ch, CN_EMB[0], 8);
        sb.vec(e + "conv_in.b", e + "conv_in.bias", CN_EMB[0]);
        for (int k = 0; k < 6; ++k) sb.conv_bias(e + "blocks." + num(k), CN_EMB[(k + 1) / 2], CN_EMB[k / 2]);
        sb.conv_bias(e + "conv_out", C0, CN_EMB[3]);
        int k = 0;
        sb.linear("controlnet_down_blocks." + num(k++), C0, C0);
        for (int i = 0; i < c.n_levels; ++i) {
            for (int j = 0; j < c.layers_per_block; ++j) sb.linear("controlnet_down_blocks." + num(k++), c.ch[i], c.ch[i]);
            if (i + 1 < c.n_levels) sb.linear("controlnet_down_blocks." + num(k++), c.ch[i], c.ch[i]);
        }
        const size_t Cm = c.ch[c.n_levels - 1];
        sb.linear("controlnet_mid_block", Cm, Cm);
        break;
    }
    }
    u.slab_bytes = sb.top;
}

// add_embedding (TimestepEmbedding(add_P, temb_dim)) of a 'text_time' handle: appended behind the existing slots, before the slab is allocated
// (mve_unet_set_addition_embed)
void layout_addition_embed(Unet& u) {
    SlabBuilder sb{u, u.slab_bytes};
    const size_t T = u.cfg.temb_dim(), P = u.cfg.add_P;
    sb.mat("add.w1", "add_embedding.linear_1.weight", T, P);
    sb.vec("add.b1", "add_embedding.linear_1.bias", T);
    sb.mat("add.w2", "add_embedding.linear_2.weight", T, T);
    sb.vec("add.b2", "add_embedding.linear_2.bias", T);
    u.slab_bytes = sb.top;
}

// ---------------------------------------------------------------------------------------------------
// load one state-dict tensor into its packed place: look the name up, check the tensor against its entry, then -- and only then -- touch the
// device: the slab on the first load (zero-filled: padding rows / optional weights start as zeros), the entry's steps
// ---------------------------------------------------------------------------------------------------
int load_param(Unet& u, const std::string& name, const void* src, int src_dtype, int ndim, const long long* shape, hipStream_t s) {
    const Config& c = u.cfg;
    const auto it = u.sources.find(name);
    MVE_CHECK(it != u.sources.end(), MVE_ERR_ARG, "load_param: %s is not a parameter of %s of this configuration", name.c_str(), kind_name(c.kind));
    const Source& e = it->second;
    MVE_CHECK(src_dtype == MVE_F32 || src_dtype == MVE_F16 || src_dtype == MVE_BF16, MVE_ERR_ARG, "load_param(%s): bad src dtype %d", name.c_str(), src_dtype);
    long long numel = 1;
    for (int i = 0; i < ndim; ++i) numel = shape[i] > 0 && numel > 0 ? numel * shape[i] : -1;
    if (e.conv[0])
        MVE_CHECK(ndim == 4 && shape[0] == e.conv[0] && shape[1] == e.conv[1] && shape[2] == 3 && shape[3] == 3, MVE_ERR_ARG,
                  "load_param(%s): expected [%lld,%lld,3,3]", name.c_str(), e.conv[0], e.conv[1]);
    MVE_CHECK(numel == e.numel, MVE_ERR_ARG, "load_param(%s): expected %lld elements, got %lld", name.c_str(), e.numel, numel);
    for (const PackStep& st : e.steps) {       // the table against the slots it names: no step writes past its slot
        const auto p = u.params.find(st.slot);
        long long end = st.phase4 ? 16 * e.conv[0] * e.conv[1] : 1;
        for (int i = 0; i < 4 && !st.phase4; ++i) end += (st.d.D[i] - 1) * st.d.t[i];
        MVE_CHECK(p != u.params.end() && (st.off + (size_t)end) * (p->second.f32 ? 4 : 2) <= p->second.bytes, MVE_ERR_STATE,
                  "load_param(%s): the layout's entry does not fit slot %s", name.c_str(), st.slot.c_str());
    }
    if (!u.slab) {
        hipError_t err = hipMalloc((void**)&u.slab, u.slab_bytes);
        if (err != hipSuccess) {
            u.slab = nullptr;
            mve_set_error("unet_load_param: hipMalloc(%zu) failed: %s", u.slab_bytes, hipGetErrorString(err));
            return MVE_ERR_HIP;
        }
        MVE_HIP(hipMemsetAsync(u.slab, 0, u.slab_bytes, s));
    }
    for (const PackStep& st : e.steps) {
        const Param& p = u.params[st.slot];
        void* dst = u.slab + p.off + st.off * (p.f32 ? 4 : 2);
        if (e.zero) MVE_HIP(hipMemsetAsync(u.slab + p.off, 0, p.bytes, s));
        const void* from = (const unsigned char*)src + st.src_off * esz(src_dtype);
        const int rc = st.phase4 ? mve_pack_upsample_phase_weights(src_dtype, c.dtype, from, (int)e.conv[0], (int)e.conv[1], dst, s)
                                 : pack(src_dtype, p.f32 ? MVE_F32 : c.dtype, from, dst, st.d, s);
        if (rc != MVE_OK) return rc;
    }
    if (e.optional && !u.loaded.count(name)) ++u.n_ip_loaded;
    u.loaded[name] = true;
    u.sd_pe_ready = false;      // the SAM decoder's dense positional encoding follows its gaussian matrix (mve_sam_decoder_finalize)
    return MVE_OK;
}

}  // namespace
