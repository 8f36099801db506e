// Fragment of the executor's single translation unit (csrc/unet.hip includes it; not a stand-alone header): the LoFTR matcher plans -- the
// reference's `matcher` (loftr/loftr.py with default_cfg, loaded at lib/apis/adapter3d.py:411-415).
#pragma once
#include "executor_builder.h"

namespace {

// LoFTR.forward in two plans with one host read (the match count) between them.
//   phase 1 (coarse): ResNetFPN_8_2 over image0 | image1 as one batch of 2N (backbone/resnet_fpn.py; every BatchNorm folded into the convolution in
//     front of it when the weights were packed, the 196-wide stage carried as 200 channels whose last 4 are zero), the position add, the 8 coarse
//     encoder layers (loftr_module/transformer.py) on mve_linattn_kv / _apply, the similarity GEMM, dual softmax and mutual-nearest selection.
//   phase 2 (fine): FinePreprocess (window gather, down_proj, merge_feat as a GEMM over the fine half with the coarse half as the epilogue's
//     per-window row vector), the 2 fine encoder layers, FineMatching.  Planned for the capacity N * L; every op takes the match count of the call
//     (Run::loftr_M) at run time.
// The token stream of a transformer lives in the left half of a [rows][2C] buffer whose right half receives norm1(message): `mlp(cat[x, message])`
// is then ONE GEMM over K = 2C with lda = 2C -- the concatenation is never formed and nothing is rounded that the reference does not round.
// Run::cn_out carries the LOFTR_IO call tensors (include/mvedit_amd.h: mve_loftr_forward_coarse) followed by the optional taps.
constexpr int LOFTR_IO = 13, LOFTR_TAPS_COARSE = 14, LOFTR_TAPS_FINE = 3;

int Builder::build_loftr(int N_, int H, int W, int phase) {
    begin(N_, H, W, phase, c.dtype);
    const int e = 2, d = dt, N = N_, Bn = 2 * N_, Hc = H / 8, Wc = W / 8, L = Hc * Wc, Sp = (L + 7) / 8 * 8, H2 = H / 2, W2 = W / 2, heads = 8;
    const long long cap = (long long)N * L;
    MVE_CHECK((long long)Bn * H2 * W2 * 256 < (1ll << 31) && cap * 25 * 2 * 256 < (1ll << 31) && (long long)L * Sp < (1ll << 31), MVE_ERR_ARG,
              "loftr: %d pairs of %d x %d overflow 32-bit activation indexing", N, H, W);
    const float ln_eps = 1e-5f, la_eps = 1e-6f;
    // copy `rows` rows of `width` bytes out of a pitched workspace tensor into call tensor / tap k (skipped when the caller gave no pointer)
    auto copy_out = [&](Ref x, size_t spitch, size_t width, int k, std::function<size_t(const Run&)> rows, const char* what) {
        live(x, what);
        op(OC_OTHER, 0, what, [=](const Run& r) {
            void* dst = r.cn_out[k];
            if (!dst) return (int)MVE_OK;
            return hipMemcpy2DAsync(dst, width, r.p(x), spitch, width, rows(r), hipMemcpyDeviceToDevice, r.stream) == hipSuccess ? (int)MVE_OK : (int)MVE_ERR_HIP;
        });
    };
    auto fixed = [](size_t n) { return [n](const Run&) { return n; }; };

    // One encoder layer call: the rows `xsel` of X (0 = first half, 1 = second half, 2 = all) attend their source (the other half; themselves for 2).
    // T tokens per batch item, `nh` batch items per half (the match count in the fine plan).  Q / KV / MS are scratch for the capacity.
    struct LayerBufs { Ref Q, KV, MS, kvf, law; size_t law_bytes; };
    auto layer = [&](const std::string& p, Ref X, const LayerBufs& bf, int C, int T, int nh_cap, bool fine, int xsel) {
        const int D = C / heads, C2 = 2 * C;
        const Ref Wq = wt(p + ".q.w"), Wkv = wt(p + ".kv.w"), Wm = wt(p + ".merge.w"), W0 = wt(p + ".mlp0.w"), W2 = wt(p + ".mlp2.w");
        const Ref g1 = wt(p + ".n1.g"), b1 = wt(p + ".n1.b"), g2 = wt(p + ".n2.g"), b2 = wt(p + ".n2.b");
        const Ref Q = bf.Q, KV = bf.KV, MS = bf.MS, kvf = bf.kvf, law = bf.law;
        const size_t law_bytes = bf.law_bytes;
        for (const Ref& t : {X, Q, KV, MS, kvf}) live(t, "encoder layer");
        struct Sz { int nb, rows; size_t xo, so; };
        auto sz = [=](const Run& r) {
            const int nh = fine ? r.loftr_M : nh_cap;
            Sz s;
            s.nb = xsel == 2 ? 2 * nh : nh; s.rows = s.nb * T;
            s.xo = xsel == 1 ? (size_t)nh * T * C2 * e : 0;
            s.so = xsel == 0 ? (size_t)nh * T * C2 * e : 0;
            return s;
        };
        const double rows_cap = (double)(xsel == 2 ? 2 : 1) * nh_cap * T;
        auto mm = [=](const Run& r, const void* A, int lda, const Ref& Wt, int ldw, void* out, int ldc, int rows, int Nn, int K) {
            return mve_gemm_pair(d, A, lda, r.p(Wt), ldw, out, ldc, rows, Nn, K, nullptr, nullptr, 0, 0, nullptr, 0, 0, 1.0f, nullptr, 0, 0, nullptr, nullptr, r.stream);
        };
        op(OC_LINEAR, 2.0 * rows_cap * C * C, "attn.q_proj", [=](const Run& r) { const Sz s = sz(r); return mm(r, (char*)r.p(X) + s.xo, C2, Wq, C, r.p(Q), C, s.rows, C, C); });
        op(OC_LINEAR, 4.0 * rows_cap * C * C, "attn.k_proj | v_proj", [=](const Run& r) { const Sz s = sz(r); return mm(r, (char*)r.p(X) + s.so, C2, Wkv, C, r.p(KV), C2, s.rows, C2, C); });
        op(OC_ATTN, 2.0 * rows_cap * C * D, "linear attention K^T V", [=](const Run& r) {
            const Sz s = sz(r);
            return mve_linattn_kv(d, r.p(KV), C2, (char*)r.p(KV) + (size_t)C * e, C2, s.nb, T, heads, D, (float*)r.p(kvf), r.p(law), law_bytes, r.stream);
        });
        op(OC_ATTN, 2.0 * rows_cap * C * D, "linear attention apply", [=](const Run& r) {
            const Sz s = sz(r);
            return mve_linattn_apply(d, r.p(Q), C, (const float*)r.p(kvf), r.p(MS), C, s.nb, T, heads, D, la_eps, r.stream);
        });
        op(OC_LINEAR, 2.0 * rows_cap * C * C, "attn.merge", [=](const Run& r) { const Sz s = sz(r); return mm(r, r.p(MS), C, Wm, C, r.p(Q), C, s.rows, C, C); });
        op(OC_NORM, 0, "norm1 -> message half", [=](const Run& r) {
            const Sz s = sz(r);
            return mve_layernorm(d, r.p(Q), C, (char*)r.p(X) + s.xo + (size_t)C * e, C2, s.rows, C, (const float*)r.p(g1), (const float*)r.p(b1), ln_eps, r.stream);
        });
        op(OC_LINEAR, 2.0 * rows_cap * C2 * C2, "mlp.0 over x | message", [=](const Run& r) { const Sz s = sz(r); return mm(r, (char*)r.p(X) + s.xo, C2, W0, C2, r.p(KV), C2, s.rows, C2, C2); });
        op(OC_OTHER, 0, "relu", [=](const Run& r) { const Sz s = sz(r); return mve_dpt_add_relu(d, r.p(KV), nullptr, r.p(KV), (size_t)s.rows * C2, r.stream); });
        op(OC_LINEAR, 2.0 * rows_cap * C * C2, "mlp.2", [=](const Run& r) { const Sz s = sz(r); return mm(r, r.p(KV), C2, W2, C2, r.p(MS), C, s.rows, C, C2); });
        op(OC_NORM, 0, "x + norm2", [=](const Run& r) {
            const Sz s = sz(r);
            char* x = (char*)r.p(X) + s.xo;
            return mve_loftr_ln_add(d, r.p(MS), C, x, C2, x, C2, s.rows, C, (const float*)r.p(g2), (const float*)r.p(b2), ln_eps, r.stream);
        });
    };
    auto layer_bufs = [&](int C, int T, long long nh_cap) {
        const size_t rows = (size_t)2 * nh_cap * T;
        LayerBufs bf;
        bf.Q = ws(rows * C * e); bf.KV = ws(rows * 2 * C * e); bf.MS = ws(rows * C * e);
        bf.kvf = ws((size_t)2 * nh_cap * heads * ((size_t)(C / heads) * (C / heads) + C / heads) * 4);
        bf.law_bytes = mve_linattn_workspace_bytes((int)(2 * nh_cap), T, heads, C / heads);
        bf.law = bf.law_bytes ? ws(bf.law_bytes) : Ref();
        return bf;
    };
    auto rel_bufs = [&](const LayerBufs& bf) { rel(bf.Q); rel(bf.KV); rel(bf.MS); rel(bf.kvf); rel(bf.law); };

    if (phase == 1) {
        const Ref px = arg(Ref::SAMPLE), pos = arg(Ref::CTX);
        auto tap = [&](Ref x, size_t bytes, int k, const char* what) { copy_out(x, bytes, bytes, LOFTR_IO + k, fixed(1), what); };
        auto leaky = [&](Ref x, size_t nel) {
            live(x, "leaky relu");
            op(OC_OTHER, 0, "leaky relu", [=](const Run& r) { return mve_loftr_leaky_relu(d, r.p(x), r.p(x), nel, 0.01f, r.stream); });
        };
        // BasicBlock: relu(bn1(conv1)), bn2(conv2) + shortcut in the second convolution's epilogue, relu
        auto block = [&](Ref x, int cin, int co, int Hh, int Ww, int stride, const std::string& b) {
            const int Ho = Hh / stride, Wo = Ww / stride;
            Ref y1 = conv3x3(x, cin, Bn, Hh, Ww, stride, b + ".c1.w", wt(b + ".c1.b"), co, Ref(), 0, "block.conv1+bn1");
            relu(y1, (size_t)Bn * Ho * Wo * co, "relu");
            Ref sc = x;
            if (stride == 2) {
                Ref xs = gather_s2(x, Bn, Hh, Ww, cin);
                sc = conv1x1(xs, Bn * Ho * Wo, cin, b + ".ds.w", wt(b + ".ds.b"), co, "block.downsample+bn");
                rel(xs);
            }
            Ref y = conv3x3(y1, co, Bn, Ho, Wo, 1, b + ".c2.w", wt(b + ".c2.b"), co, sc, 0, "block.conv2+bn2+shortcut");
            relu(y, (size_t)Bn * Ho * Wo * co, "relu");
            rel(y1);
            if (stride == 2) rel(sc);
            return y;
        };

        // ---- backbone -------------------------------------------------------------------------------------------------------------------------
        Ref x0;
        {
            Ref rows = ws((size_t)Bn * H2 * W2 * 56 * e);
            op(OC_OTHER, 0, "stem window rows", [=](const Run& r) { return mve_loftr_stem_rows(d, r.p(px), Bn, H, W, r.p(rows), 56, r.stream); });
            x0 = conv1x1(rows, Bn * H2 * W2, 56, "stem.w", wt("stem.b"), 128, "stem.conv 7x7/2+bn");
            rel(rows);
            relu(x0, (size_t)Bn * H2 * W2 * 128, "relu");
            tap(x0, (size_t)Bn * H2 * W2 * 128 * e, 0, "stem -> tap");
        }
        const int Wd[3] = {128, 200, 256};
        Ref xs[3];
        Ref x = x0;
        int cin = 128, Hh = H2, Ww = W2;
        for (int s = 0; s < 3; ++s) {
            const std::string b = "l" + std::to_string(s + 1);
            const int stride = s == 0 ? 1 : 2;
            Ref a = block(x, cin, Wd[s], Hh, Ww, stride, b + ".b0");
            if (s == 0) rel(x);      // the stem output; the stage outputs stay for the FPN
            Hh /= stride; Ww /= stride;
            Ref y = block(a, Wd[s], Wd[s], Hh, Ww, 1, b + ".b1");
            rel(a);
            xs[s] = y; x = y; cin = Wd[s];
            tap(y, (size_t)Bn * Hh * Ww * Wd[s] * e, 1 + s, "stage -> tap");
        }
        const int H4 = H / 4, W4 = W / 4;
        Ref x3o = conv1x1(xs[2], Bn * L, 256, "l3oc.w", Ref(), 256, "layer3_outconv");
        rel(xs[2]);
        tap(x3o, (size_t)Bn * L * 256 * e, 4, "coarse feature -> tap");
        Ref u3 = upsample2x(x3o, Bn, Hc, Wc, 256, "upsample x2 (align_corners)");
        Ref s2 = ws((size_t)Bn * H4 * W4 * 256 * e);
        dense(xs[1], wt("l2oc.w"), Ref(), s2, Bn * H4 * W4, 256, 200, u3, "layer2_outconv + upsampled");
        rel(u3); rel(xs[1]);
        Ref t2 = conv3x3(s2, 256, Bn, H4, W4, 1, "l2oc2.0.w", wt("l2oc2.0.b"), 256, Ref(), 0, "layer2_outconv2.conv+bn");
        rel(s2);
        leaky(t2, (size_t)Bn * H4 * W4 * 256);
        Ref x2o = conv3x3(t2, 256, Bn, H4, W4, 1, "l2oc2.3.w", Ref(), 200, Ref(), 0, "layer2_outconv2.conv");
        rel(t2);
        Ref u2 = upsample2x(x2o, Bn, H4, W4, 200, "upsample x2 (align_corners)");
        rel(x2o);
        Ref s1 = ws((size_t)Bn * H2 * W2 * 200 * e);
        dense(xs[0], wt("l1oc.w"), Ref(), s1, Bn * H2 * W2, 200, 128, u2, "layer1_outconv + upsampled");
        rel(u2); rel(xs[0]);
        Ref t1 = conv3x3(s1, 200, Bn, H2, W2, 1, "l1oc2.0.w", wt("l1oc2.0.b"), 200, Ref(), 0, "layer1_outconv2.conv+bn");
        rel(s1);
        leaky(t1, (size_t)Bn * H2 * W2 * 200);
        conv(t1, 200, Bn, H2, W2, 1, 0, wt("l1oc2.3.w"), 128, cn_out(0), Ref(), Ref(), 0, Ref(), 0, "layer1_outconv2.conv -> feat_f");
        rel(t1);

        // ---- tokens: position add, 8 encoder layers ----------------------------------------------------------------------------------------------
        const size_t rows = (size_t)Bn * L;
        Ref X = ws((rows + 8) * 512 * e);      // + 8 rows of zeros: the similarity GEMM reads Sp >= S rows of feat1
        {
            Ref tok = ws(rows * 256 * e);
            live(x3o, "position add");
            op(OC_OTHER, 0, "position add", [=](const Run& r) { return mve_loftr_pos_add(d, r.p(x3o), (const float*)r.p(pos), r.p(tok), Bn, L, 256, r.stream); });
            rel(x3o);
            tap(tok, rows * 256 * e, 5, "tokens -> tap");
            op(OC_OTHER, 0, "zero the padding rows", [=](const Run& r) {
                return hipMemsetAsync((char*)r.p(X) + rows * 512 * e, 0, (size_t)8 * 512 * e, r.stream) == hipSuccess ? (int)MVE_OK : (int)MVE_ERR_HIP;
            });
            copy2d(X, 512 * e, tok, 256 * e, 256 * e, rows, "tokens -> stream");
            rel(tok);
        }
        {
            const LayerBufs bf = layer_bufs(256, L, N);
            for (int k = 0; k < 8; ++k) {
                const std::string p = "c" + std::to_string(k);
                if (k % 2 == 0) layer(p, X, bf, 256, L, N, false, 2);      // 'self': feat0 | feat1 as one batch of 2N
                else { layer(p, X, bf, 256, L, N, false, 0); layer(p, X, bf, 256, L, N, false, 1); }      // 'cross': feat1 attends the UPDATED feat0
                copy_out(X, 512 * e, 256 * e, LOFTR_IO + 6 + k, fixed(rows), "encoder layer -> tap");
            }
            rel_bufs(bf);
        }
        copy_out(X, 512 * e, 256 * e, 1, fixed(rows), "tokens -> feat_c");

        // ---- coarse matching ---------------------------------------------------------------------------------------------------------------------
        {
            const float scale = 1.0f / (256.0f * 0.1f);      // (f0 / sqrt(C)) . (f1 / sqrt(C)) / temperature
            live(X, "similarity");
            op(OC_LINEAR, 2.0 * N * (double)L * Sp * 256, "similarity", [=](const Run& r) {
                for (int n = 0; n < N; ++n) {
                    const char* f0 = (const char*)r.p(X) + (size_t)n * L * 512 * e;
                    const char* f1 = (const char*)r.p(X) + (size_t)(N + n) * L * 512 * e;
                    float* out = (float*)r.cn_out[2] + (size_t)n * L * Sp;
                    const int rc = mve_gemm_pair(d, f0, 512, f1, 512, out, Sp, L, Sp, 256, nullptr, nullptr, 0, 0, nullptr, 0, MVE_GEMM_OUT_F32, scale, nullptr, 0, 0, nullptr, nullptr,
                                                 r.stream);
                    if (rc) return rc;
                }
                return (int)MVE_OK;
            });
            rel(X);
            Ref rs = ws((size_t)N * L * 2 * 4), cs = ws((size_t)N * L * 2 * 4);
            op(OC_OTHER, 0, "dual softmax statistics", [=](const Run& r) {
                return mve_dsmax_stats((const float*)r.cn_out[2], N, L, L, Sp, (float*)r.p(rs), (float*)r.p(cs), r.stream);
            });
            op(OC_OTHER, 0, "dual softmax confidence", [=](const Run& r) {
                return mve_dsmax_conf((const float*)r.cn_out[2], N, L, L, Sp, (const float*)r.p(rs), (const float*)r.p(cs), (float*)r.cn_out[3], r.stream);
            });
            rel(rs); rel(cs);
            const size_t sb = mve_dsmax_select_workspace_bytes(N, L, L);
            Ref sw = ws(sb);
            op(OC_OTHER, 0, "mutual-nearest selection", [=](const Run& r) {
                return mve_dsmax_select((const float*)r.cn_out[3], N, Hc, Wc, Hc, Wc, r.loftr_thr, r.loftr_border, 8.0f, (int64_t*)r.cn_out[4], (int64_t*)r.cn_out[5],
                                        (int64_t*)r.cn_out[6], (float*)r.cn_out[7], (float*)r.cn_out[8], (float*)r.cn_out[9], (int*)r.cn_out[10], r.p(sw), sb, r.stream);
            });
            rel(sw);
        }
    } else {
        // ---- fine stage, for M = Run::loftr_M matches (capacity N * L) ---------------------------------------------------------------------------------
        const long long Mc = cap;
        const size_t fmap = (size_t)N * H2 * W2 * 128 * e, cmap = (size_t)N * L * 256 * e;
        Ref U = ws((size_t)2 * Mc * 25 * 128 * e);
        op(OC_OTHER, 0, "fine window gather", [=](const Run& r) {
            const int M = r.loftr_M;
            const char* ff = (const char*)r.cn_out[0];
            int rc = mve_loftr_unfold(d, ff, N, H2, W2, 128, (const int64_t*)r.cn_out[4], (const int64_t*)r.cn_out[5], M, r.p(U), r.stream);
            if (rc) return rc;
            return mve_loftr_unfold(d, ff + fmap, N, H2, W2, 128, (const int64_t*)r.cn_out[4], (const int64_t*)r.cn_out[6], M, (char*)r.p(U) + (size_t)M * 25 * 128 * e, r.stream);
        });
        copy_out(U, 128 * e, 128 * e, LOFTR_IO + 0, [](const Run& r) { return (size_t)2 * r.loftr_M * 25; }, "windows -> tap");
        Ref G = ws((size_t)2 * Mc * 256 * e), CW = ws((size_t)2 * Mc * 128 * e), RV = ws((size_t)2 * Mc * 128 * 4);
        op(OC_OTHER, 0, "coarse feature gather", [=](const Run& r) {
            const int M = r.loftr_M;
            const char* fc = (const char*)r.cn_out[1];
            int rc = mve_loftr_gather_rows(d, fc, N, L, 256, (const int64_t*)r.cn_out[4], (const int64_t*)r.cn_out[5], M, r.p(G), r.stream);
            if (rc) return rc;
            return mve_loftr_gather_rows(d, fc + cmap, N, L, 256, (const int64_t*)r.cn_out[4], (const int64_t*)r.cn_out[6], M, (char*)r.p(G) + (size_t)M * 256 * e, r.stream);
        });
        const Ref Wdp = wt("dp.w"), bdp = wt("dp.b"), Wmf = wt("mf.w"), Wmc = wt("mf.w", 128), bmf = wt("mf.b");
        op(OC_LINEAR, 2.0 * 2 * Mc * 128 * 256, "down_proj", [=](const Run& r) {
            return mve_gemm_pair(d, r.p(G), 256, r.p(Wdp), 256, r.p(CW), 128, 2 * r.loftr_M, 128, 256, (const float*)r.p(bdp), nullptr, 0, 0, nullptr, 0, 0, 1.0f, nullptr, 0, 0, nullptr,
                                 nullptr, r.stream);
        });
        op(OC_LINEAR, 2.0 * 2 * Mc * 128 * 128, "merge_feat (coarse half + bias)", [=](const Run& r) {
            return mve_gemm_pair(d, r.p(CW), 128, r.p(Wmc), 256, r.p(RV), 128, 2 * r.loftr_M, 128, 128, (const float*)r.p(bmf), nullptr, 0, 0, nullptr, 0, MVE_GEMM_OUT_F32, 1.0f, nullptr,
                                 0, 0, nullptr, nullptr, r.stream);
        });
        Ref X = ws((size_t)2 * Mc * 25 * 256 * e);
        op(OC_LINEAR, 2.0 * 2 * Mc * 25 * 128 * 128, "merge_feat (fine half + window row)", [=](const Run& r) {
            return mve_gemm_pair(d, r.p(U), 128, r.p(Wmf), 256, r.p(X), 256, 2 * r.loftr_M * 25, 128, 128, nullptr, (const float*)r.p(RV), 128, 25, nullptr, 0, 0, 1.0f, nullptr, 0, 0,
                                 nullptr, nullptr, r.stream);
        });
        rel(U); rel(G); rel(CW); rel(RV);
        auto rows2 = [](const Run& r) { return (size_t)2 * r.loftr_M * 25; };
        copy_out(X, 256 * e, 128 * e, LOFTR_IO + 1, rows2, "merged windows -> tap");
        {
            const LayerBufs bf = layer_bufs(128, 25, Mc);
            layer("f0", X, bf, 128, 25, (int)Mc, true, 2);
            layer("f1", X, bf, 128, 25, (int)Mc, true, 0);
            layer("f1", X, bf, 128, 25, (int)Mc, true, 1);
            rel_bufs(bf);
        }
        Ref FY = ws((size_t)2 * Mc * 25 * 128 * e);
        live(X, "fine windows"); live(FY, "fine windows");
        op(OC_OTHER, 0, "fine windows -> dense", [=](const Run& r) {
            return hipMemcpy2DAsync(r.p(FY), 128 * e, r.p(X), 256 * e, 128 * e, rows2(r), hipMemcpyDeviceToDevice, r.stream) == hipSuccess ? (int)MVE_OK : (int)MVE_ERR_HIP;
        });
        rel(X);
        copy_out(FY, 128 * e, 128 * e, LOFTR_IO + 2, rows2, "fine windows -> tap");
        const float radius = 2.0f * ((float)H / (float)H2);      // (window // 2) * image / fine map
        op(OC_OTHER, 0, "fine matching", [=](const Run& r) {
            const int M = r.loftr_M;
            return mve_loftr_fine_match(d, r.p(FY), (char*)r.p(FY) + (size_t)M * 25 * 128 * e, M, 128, (const float*)r.cn_out[9], radius, (float*)r.cn_out[11], (float*)r.cn_out[12],
                                        r.stream);
        });
        rel(FY);
    }
    return finish("loftr");
}

}  // namespace
