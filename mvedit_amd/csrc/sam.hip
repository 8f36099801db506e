// Segment Anything image encoder primitives (include/mvedit_amd.h section 2g): self-attention with MViTv2's decomposed relative-position bias,
// the zero-padded window partition around it, and the absolute position add.  They replace the arithmetic of segment_anything's
// `ImageEncoderViT` (the same as transformers' SamVisionEncoder, models/sam/modeling_sam.py) that the reference reaches through
// `SamPredictor.set_image` (lib/apis/adapter3d.py:363-372, :723-734; lib/pipelines/utils.py:114-131).  Everything else of the encoder is the
// executor's GEMMs, mve_layernorm, mve_act and mve_conv3x3 (csrc/builder_sam.h).  One timing exists (profiles/sam_encoder.txt); nothing here is tuned.
#include "common.h"

#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------------
// attention with decomposed relative-position bias: one block of four waves per (sequence, head, tile of 64 queries)
//
//   logit(q, k) = scale * Q[q].K[k] + Q[q].Rh[qh - kh + gh - 1] + Q[q].Rw[qw - kw + gw - 1],  (qh, qw) = (q / gw, q % gw), same for k
//
//   The bias needs, per query, only Q.Rh^T [2gh-1] and Q.Rw^T [2gw-1].  A wave owns 16 queries; in the prologue it forms both products with
//   the 16x16x32 MFMA -- A = its Q fragments (kept in registers for the key loop), B = table rows read from global memory (the tables are at
//   most 127 x 80 elements and every block reads the same ones: they stay in L2) -- and leaves them in LDS as fp32, sT [64][TLD].  The bias is
//   never rounded to 16 bit.  The key loop walks tiles of 64 keys: K [64][HDP] and V transposed [HD][64] staged in LDS by the whole block, S =
//   Q K^T by MFMA, the two bias terms fetched from sT by (qh - kh, qw - kw), an online softmax in fp32 (base 2), P through LDS (C/D layout -> A
//   operand layout) rounded to the storage type, O += P V by MFMA.  The padded tail of the last key tile is masked by a select: a masked key
//   takes no part in the maximum and has probability exactly 0; key 0 is always visible, so the maximum is finite after the first tile.
//   The sum is taken over the unrounded fp32 probabilities; O = acc / sum is rounded once.  head_dim 80 runs as 96 with zero columns.
//   No atomics; a block reads nothing but its own sequence: two runs give the same bits and a sequence's result does not depend on NS.
// ---------------------------------------------------------------------------------------------------
constexpr int RP_WAVES = 4, RP_QT = 64, RP_KT = 64;
constexpr int RP_VLD = RP_KT + 8;         // V^T and P row pitch (elements): 144 B

template <int HD> struct RpDims {
    static constexpr int HDP = (HD + 31) / 32 * 32;      // K extent of the QK^T MFMA steps
    static constexpr int KS = HDP / 32;
    static constexpr int NT = HD / 16;                    // 16-column output tiles
    static constexpr int KLD = HDP + 8;                   // K row pitch
};

inline int rp_tld(int gh, int gw) { return (2 * gh - 1 + 2 * gw - 1) | 1; }      // odd: the 16 rows of a wave start on different banks
template <int HD>
inline size_t rp_lds_bytes(int gh, int gw) {
    return (size_t)RP_QT * rp_tld(gh, gw) * 4 + ((size_t)RP_KT * RpDims<HD>::KLD + (size_t)HD * RP_VLD + (size_t)RP_WAVES * 16 * RP_VLD) * 2 + 16;
}

template <class Tag, int HD>
__global__ __launch_bounds__(RP_WAVES * 64) void k_attention_relpos(const typename Tag::T* __restrict__ Q, int ldq, const typename Tag::T* __restrict__ K, int ldk,
                                                                    const typename Tag::T* __restrict__ V, int ldv, const typename Tag::T* __restrict__ Rh,
                                                                    const typename Tag::T* __restrict__ Rw, typename Tag::T* __restrict__ O, int ldo, int gh, int gw,
                                                                    int heads, int nqt, float scale_log2e) {
    typedef typename Tag::T T;
    typedef typename Tag::V8 V8;
    typedef RpDims<HD> D;
    extern __shared__ __attribute__((aligned(16))) unsigned char rp_lds[];
    const int L = gh * gw, nh = 2 * gh - 1, nw = 2 * gw - 1, TLD = (nh + nw) | 1;
    float* sT = reinterpret_cast<float*>(rp_lds);
    T* sK = reinterpret_cast<T*>(rp_lds + (((size_t)RP_QT * TLD * 4 + 15) & ~(size_t)15));
    T* sVt = sK + RP_KT * D::KLD;
    T* sP = sVt + HD * RP_VLD;

    const int qt = blockIdx.x % nqt, sh = blockIdx.x / nqt, h = sh % heads, seq = sh / heads;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const size_t row0 = (size_t)seq * L;
    const T* Qh = Q + h * HD;
    const T* Kh = K + h * HD;
    const T* Vh = V + h * HD;
    T* Oh = O + h * HD;
    const int q0 = qt * RP_QT + w * 16;      // this wave's 16 queries (rows >= L: computed on zeros, never stored)

    // Q fragments (A operand): row q0 + lr, k = 32 ks + 8 lg + j; columns >= HD and rows >= L are zeros
    V8 qa[D::KS];
#pragma unroll
    for (int ks = 0; ks < D::KS; ++ks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) qa[ks][e] = (T)0.f;
        if (q0 + lr < L && ks * 32 + lg * 8 < HD) qa[ks] = *reinterpret_cast<const V8*>(Qh + (row0 + q0 + lr) * (size_t)ldq + ks * 32 + lg * 8);
    }
    // bias tables of this wave's queries: sT[q][j] = Q[q] . Rh[j] (j < nh), sT[q][nh + j] = Q[q] . Rw[j] (j < nw)
    float* myT = sT + (size_t)w * 16 * TLD;
    for (int part = 0; part < 2; ++part) {
        const T* R = part ? Rw : Rh;
        const int n = part ? nw : nh, base = part ? nh : 0;
        for (int t = 0; t < (n + 15) / 16; ++t) {
            const int j = t * 16 + lr;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < D::KS; ++ks) {
                V8 rb;
#pragma unroll
                for (int e = 0; e < 8; ++e) rb[e] = (T)0.f;
                if (j < n && ks * 32 + lg * 8 < HD) rb = *reinterpret_cast<const V8*>(R + (size_t)j * HD + ks * 32 + lg * 8);      // B operand: table row j
                acc = Tag::mfma16(qa[ks], rb, acc);
            }
            // C/D layout: acc[r] is (query q0 + 4 lg + r, table row 16 t + lr)
            if (j < n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) myT[(lg * 4 + r) * TLD + base + j] = acc[r];
            }
        }
    }
    // per accumulator row r (query q0 + 4 lg + r): the index of its height / width term for key (0, 0); key (kh, kw) subtracts kh / kw
    int tqh[4], tqw[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int q = q0 + lg * 4 + r;
        q = q < L ? q : L - 1;
        const int qh = q / gw, qw = q - qh * gw;
        tqh[r] = (lg * 4 + r) * TLD + (qh + gh - 1);
        tqw[r] = (lg * 4 + r) * TLD + nh + (qw + gw - 1);
    }

    f32x4 acc[D::NT];
#pragma unroll
    for (int nt = 0; nt < D::NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m[4] = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f}, sum[4] = {0.f, 0.f, 0.f, 0.f};
    T* myP = sP + w * 16 * RP_VLD;

    for (int k0 = 0; k0 < L; k0 += RP_KT) {
        __syncthreads();          // the previous tile's K / V^T / P are consumed (first pass: the bias tables are written)
        for (int i = tid; i < RP_KT * (D::HDP / 8); i += RP_WAVES * 64) {
            const int r = i / (D::HDP / 8), c8 = (i - r * (D::HDP / 8)) * 8;
            V8 kv, vv;
#pragma unroll
            for (int e = 0; e < 8; ++e) { kv[e] = (T)0.f; vv[e] = (T)0.f; }
            const bool in = k0 + r < L && c8 < HD;
            if (in) {
                kv = *reinterpret_cast<const V8*>(Kh + (row0 + k0 + r) * (size_t)ldk + c8);
                vv = *reinterpret_cast<const V8*>(Vh + (row0 + k0 + r) * (size_t)ldv + c8);
            }
            *reinterpret_cast<V8*>(&sK[r * D::KLD + c8]) = kv;
            if (c8 < HD) {
#pragma unroll
                for (int e = 0; e < 8; ++e) sVt[(c8 + e) * RP_VLD + r] = vv[e];
            }
        }
        __syncthreads();
        f32x4 s[RP_KT / 16];
#pragma unroll
        for (int kt = 0; kt < RP_KT / 16; ++kt) {
            s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < D::KS; ++ks) {
                const V8 kb = *reinterpret_cast<const V8*>(&sK[(kt * 16 + lr) * D::KLD + ks * 32 + lg * 8]);      // B operand: key k0 + 16 kt + lr
                s[kt] = Tag::mfma16(qa[ks], kb, s[kt]);
            }
        }
        // C/D layout: s[kt][r] is (query q0 + 4 lg + r, key k0 + 16 kt + lr)
        float tm[4] = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
#pragma unroll
        for (int kt = 0; kt < RP_KT / 16; ++kt) {
            const int key = k0 + kt * 16 + lr;
            const bool vis = key < L;
            const int kc = vis ? key : L - 1, kh = kc / gw, kw = kc - kh * gw;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float bias = myT[tqh[r] - kh] + myT[tqw[r] - kw];
                s[kt][r] = s[kt][r] * scale_log2e + bias * 1.4426950408889634f;
                tm[r] = vis ? fmaxf(tm[r], s[kt][r]) : tm[r];
            }
        }
        float alpha[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) tm[r] = fmaxf(tm[r], __shfl_xor(tm[r], o, 64));
            const float mn = fmaxf(m[r], tm[r]);
            alpha[r] = exp2f(m[r] - mn);
            m[r] = mn;
            sum[r] *= alpha[r];
        }
#pragma unroll
        for (int kt = 0; kt < RP_KT / 16; ++kt) {
            const int kl = kt * 16 + lr;
            const bool vis = k0 + kl < L;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = vis ? exp2f(s[kt][r] - m[r]) : 0.f;
                sum[r] += p;
                myP[(lg * 4 + r) * RP_VLD + kl] = Tag::from_f32(p);
            }
        }
#pragma unroll
        for (int nt = 0; nt < D::NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[nt][r] *= alpha[r];
        __syncthreads();          // P of this wave is in LDS
#pragma unroll
        for (int kk = 0; kk < RP_KT / 32; ++kk) {
            const V8 pa = *reinterpret_cast<const V8*>(&myP[lr * RP_VLD + kk * 32 + lg * 8]);                      // A operand: query q0 + lr
#pragma unroll
            for (int nt = 0; nt < D::NT; ++nt) {
                const V8 vb = *reinterpret_cast<const V8*>(&sVt[(nt * 16 + lr) * RP_VLD + kk * 32 + lg * 8]);      // B operand: column 16 nt + lr
                acc[nt] = Tag::mfma16(pa, vb, acc[nt]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sum[r] += __shfl_xor(sum[r], o, 64);
        const int q = q0 + lg * 4 + r;
        if (q < L) {
#pragma unroll
            for (int nt = 0; nt < D::NT; ++nt) Oh[(row0 + q) * (size_t)ldo + nt * 16 + lr] = Tag::from_f32(acc[nt][r] / sum[r]);
        }
    }
}

template <class Tag, int HD>
int launch_attention_relpos_hd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* Rh, const void* Rw, void* O, int ldo, int NS,
                               int gh, int gw, int heads, float scale, hipStream_t s) {
    typedef typename Tag::T T;
    const int nqt = (gh * gw + RP_QT - 1) / RP_QT;
    // the kernel is allowed the LDS of the largest grid (gh + gw = 128, the table pitch of 64 x 64: ~100 KB) once per device; a launch asks for what
    // its own grid needs, so the 14 x 14 windows (~48 KB) keep three blocks on a CU
    static bool configured[64] = {};
    int dev = 0;
    MVE_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !configured[dev]) {
        MVE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attention_relpos<Tag, HD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rp_lds_bytes<HD>(64, 64)));
        if (dev >= 0 && dev < 64) configured[dev] = true;
    }
    k_attention_relpos<Tag, HD><<<dim3((unsigned)((size_t)NS * heads * nqt)), dim3(RP_WAVES * 64), rp_lds_bytes<HD>(gh, gw), s>>>(
        (const T*)Q, ldq, (const T*)K, ldk, (const T*)V, ldv, (const T*)Rh, (const T*)Rw, (T*)O, ldo, gh, gw, heads, nqt, scale * 1.4426950408889634f);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

template <class Tag>
int launch_attention_relpos(int hd, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* Rh, const void* Rw, void* O, int ldo, int NS,
                            int gh, int gw, int heads, float scale, hipStream_t s) {
    if (hd == 64) return launch_attention_relpos_hd<Tag, 64>(Q, ldq, K, ldk, V, ldv, Rh, Rw, O, ldo, NS, gh, gw, heads, scale, s);
    return launch_attention_relpos_hd<Tag, 80>(Q, ldq, K, ldk, V, ldv, Rh, Rw, O, ldo, NS, gh, gw, heads, scale, s);
}

// ---------------------------------------------------------------------------------------------------
// window partition / un-partition: x [B][G][G][C] <-> win [B * nw * nw][w * w][C], nw = ceil(G / w); one thread per 8 channels of a WINDOW
// row.  Partition writes zeros where the padded map has no source; un-partition never reads those rows.  16-byte vectors, no arithmetic.
// ---------------------------------------------------------------------------------------------------
template <bool UN>
__global__ __launch_bounds__(256) void k_sam_window(const u32x4* __restrict__ src, u32x4* __restrict__ dst, int G, int w, int nw, int C8, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / C8;                     // row of the windowed tensor
    const int c8 = (int)(i - row * C8), ww = w * w;
    const long long win = row / ww;
    const int t = (int)(row - win * ww), ty = t / w, tx = t - ty * w;
    const long long b = win / ((long long)nw * nw);
    const int wi = (int)(win - b * nw * nw), wy = wi / nw, wx = wi - wy * nw;
    const int y = wy * w + ty, x = wx * w + tx;
    const bool in = y < G && x < G;
    const long long xi = ((b * G + y) * G + x) * C8 + c8;
    if (UN) {
        if (in) dst[xi] = src[i];
    } else {
        dst[i] = in ? src[xi] : u32x4{0u, 0u, 0u, 0u};
    }
}

// position add: y[b, p, :] = round_once(float(x[b, p, :]) + float(pos[p, :])); one thread per 8 channels
template <class Tag>
__global__ __launch_bounds__(256) void k_sam_pos_add(const typename Tag::T* __restrict__ x, const typename Tag::T* __restrict__ pos, typename Tag::T* __restrict__ y,
                                                     long long per_image8, long long total) {
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const V8 a = reinterpret_cast<const V8*>(x)[i], e = reinterpret_cast<const V8*>(pos)[i % per_image8];
    V8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = Tag::from_f32(Tag::to_f32(a[k]) + Tag::to_f32(e[k]));
    reinterpret_cast<V8*>(y)[i] = o;
}

template <class Tag>
int launch_sam_pos_add(const void* x, const void* pos, void* y, int B, int HW, int C, hipStream_t s) {
    typedef typename Tag::T T;
    const long long per = (long long)HW * (C / 8), total = (long long)B * per;
    k_sam_pos_add<Tag><<<mve_cdiv(total, 256), 256, 0, s>>>((const T*)x, (const T*)pos, (T*)y, per, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_window(const char* who, int dtype, const void* a, const void* b, int B, int G, int C, int w) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "%s: dtype %d must be f16 or bf16", who, dtype);
    MVE_CHECK(a && b, MVE_ERR_ARG, "%s: null pointer (d_x / d_win)", who);
    MVE_CHECK(B >= 1 && G >= 1 && w >= 1 && w <= G, MVE_ERR_ARG, "%s: bad B %d / G %d / window %d (1 <= window <= G)", who, B, G, w);
    MVE_CHECK(C >= 8 && C % 8 == 0, MVE_ERR_ARG, "%s: C %d must be a multiple of 8", who, C);
    const long long gp = (long long)(G + w - 1) / w * w;
    MVE_CHECK((long long)B * gp * gp * C < (1ll << 31), MVE_ERR_ARG, "%s: batch B %d overflows 32-bit indexing", who, B);
    MVE_CHECK(aligned16(a) && aligned16(b), MVE_ERR_ARG, "%s: d_x / d_win must be 16-byte aligned", who);
    return MVE_OK;
}

template <bool UN>
int launch_sam_window(const void* src, void* dst, int B, int G, int C, int w, hipStream_t s) {
    const int nw = (G + w - 1) / w;
    const long long total = (long long)B * nw * nw * w * w * (C / 8);
    k_sam_window<UN><<<mve_cdiv(total, 256), 256, 0, s>>>((const u32x4*)src, (u32x4*)dst, G, w, nw, C / 8, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // namespace

extern "C" int mve_attention_relpos(int dtype, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* rel_h, const void* rel_w, void* O,
                                    int ldo, int NS, int gh, int gw, int heads, int head_dim, float scale, void* stream) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "attention_relpos: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(Q && K && V && O && rel_h && rel_w, MVE_ERR_ARG, "attention_relpos: null pointer (d_Q / d_K / d_V / d_rel_h / d_rel_w / d_O)");
    MVE_CHECK(head_dim == 64 || head_dim == 80, MVE_ERR_ARG, "attention_relpos: head_dim %d must be 64 or 80", head_dim);
    MVE_CHECK(gh >= 1 && gw >= 1 && (long long)gh + gw <= 128, MVE_ERR_ARG,
              "attention_relpos: gh %d / gw %d must be >= 1 with gh + gw <= 128 (the per-query bias tables live in LDS)", gh, gw);
    MVE_CHECK(NS >= 1 && heads >= 1, MVE_ERR_ARG, "attention_relpos: bad NS %d / heads %d", NS, heads);
    const long long L = (long long)gh * gw, width = (long long)heads * head_dim;
    MVE_CHECK((long long)NS * heads * ((L + RP_QT - 1) / RP_QT) < (1ll << 31), MVE_ERR_ARG, "attention_relpos: NS %d x heads %d overflows the grid", NS, heads);
    MVE_CHECK(ldq >= width && ldq % 8 == 0, MVE_ERR_ARG, "attention_relpos: ldq %d must be a multiple of 8 and >= heads * head_dim", ldq);
    MVE_CHECK(ldk >= width && ldk % 8 == 0, MVE_ERR_ARG, "attention_relpos: ldk %d must be a multiple of 8 and >= heads * head_dim", ldk);
    MVE_CHECK(ldv >= width && ldv % 8 == 0, MVE_ERR_ARG, "attention_relpos: ldv %d must be a multiple of 8 and >= heads * head_dim", ldv);
    MVE_CHECK(ldo >= width, MVE_ERR_ARG, "attention_relpos: ldo %d must be >= heads * head_dim", ldo);
    const long long ldmax = ldq > ldk ? (ldq > ldv ? ldq : ldv) : (ldk > ldv ? ldk : ldv);
    MVE_CHECK((long long)NS * L * (ldmax > ldo ? ldmax : ldo) < (1ll << 40), MVE_ERR_ARG, "attention_relpos: NS %d is out of range", NS);
    MVE_CHECK(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(rel_h) && aligned16(rel_w), MVE_ERR_ARG,
              "attention_relpos: d_Q / d_K / d_V / d_rel_h / d_rel_w must be 16-byte aligned");
    MVE_CHECK(scale == scale && scale > 0.f, MVE_ERR_ARG, "attention_relpos: scale must be positive");
    return MVE_DISPATCH_16(dtype, launch_attention_relpos, head_dim, Q, ldq, K, ldk, V, ldv, rel_h, rel_w, O, ldo, NS, gh, gw, heads, scale, (hipStream_t)stream);
}

extern "C" int mve_sam_window_partition(int dtype, const void* x, int B, int G, int C, int window, void* win, void* stream) {
    const int rc = check_window("sam_window_partition", dtype, x, win, B, G, C, window);
    if (rc) return rc;
    return launch_sam_window<false>(x, win, B, G, C, window, (hipStream_t)stream);
}

extern "C" int mve_sam_window_unpartition(int dtype, const void* win, int B, int G, int C, int window, void* x, void* stream) {
    const int rc = check_window("sam_window_unpartition", dtype, x, win, B, G, C, window);
    if (rc) return rc;
    return launch_sam_window<true>(win, x, B, G, C, window, (hipStream_t)stream);
}

extern "C" int mve_sam_pos_add(int dtype, const void* x, const void* pos, void* y, int B, int HW, int C, void* stream) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "sam_pos_add: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(x && pos && y, MVE_ERR_ARG, "sam_pos_add: null pointer (d_x / d_pos / d_y)");
    MVE_CHECK(B >= 1 && HW >= 1, MVE_ERR_ARG, "sam_pos_add: bad B %d / HW %d", B, HW);
    MVE_CHECK(C >= 8 && C % 8 == 0, MVE_ERR_ARG, "sam_pos_add: C %d must be a multiple of 8", C);
    MVE_CHECK((long long)B * HW * C < (1ll << 31), MVE_ERR_ARG, "sam_pos_add: batch B %d overflows 32-bit indexing", B);
    MVE_CHECK(aligned16(x) && aligned16(pos) && aligned16(y), MVE_ERR_ARG, "sam_pos_add: d_x / d_pos / d_y must be 16-byte aligned");
    return MVE_DISPATCH_16(dtype, launch_sam_pos_add, x, pos, y, B, HW, C, (hipStream_t)stream);
}
