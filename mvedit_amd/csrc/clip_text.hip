// CLIP text tower primitives (include/mvedit_amd.h section 2c): causal self-attention, token + position embedding, quick-GELU / GELU, and the
// end-of-text pooling gather.  They replace the arithmetic of transformers' CLIPTextModel / CLIPTextModelWithProjection
// (models/clip/modeling_clip.py) that the reference's pipelines reach through `self.text_encoder` (lib/pipelines/utils.py:244-283,
// lib/pipelines/mvedit_3d_pipeline.py:368).  The text tower is not the hot loop: the kernels are written to be read, not tuned.
#include "common.h"

#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------------
// causal attention, head_dim 64, L <= 128: one block of four waves per (batch item, head)
//
//   LDS: K [128][64] row-major and V transposed [64][128] of the head (rows >= L are zeros), plus one P tile [16][128] per wave.
//   A wave owns query tiles of 16 rows (tile w and tile w + 4).  For query tile t only the key tiles 0..t can be visible, so
//   S = Q K^T is at most 8 accumulator tiles of the 16x16x32 MFMA, all of them held in registers: the softmax is the plain two-pass
//   one (row maximum, then exp and sum), not an online one.  The mask is a select on (key <= query && key < L): a masked logit takes
//   no part in the maximum and its probability is the constant 0, so no infinity is ever formed.  Every row sees key 0, so the maximum
//   is finite and the sum is at least 1.  P goes through LDS (C/D layout -> A operand layout) rounded to the storage type, the sum is
//   taken over the unrounded fp32 values, O = (P V) / sum is rounded once.
// ---------------------------------------------------------------------------------------------------
constexpr int CA_D = 64, CA_LMAX = 128, CA_WAVES = 4;
constexpr int CA_KLD = CA_D + 8;          // K row pitch (elements): 144 B, 16-byte aligned, rows land on different banks
constexpr int CA_VLD = CA_LMAX + 8;       // V^T and P row pitch: 272 B

template <class Tag>
__global__ __launch_bounds__(CA_WAVES * 64) void k_attention_causal(const typename Tag::T* __restrict__ Q, int ldq, const typename Tag::T* __restrict__ K, int ldk,
                                                                    const typename Tag::T* __restrict__ V, int ldv, typename Tag::T* __restrict__ O, int ldo,
                                                                    int L, int heads, float scale_log2e) {
    typedef typename Tag::T T;
    typedef typename Tag::V8 V8;
    __shared__ __attribute__((aligned(16))) T sK[CA_LMAX * CA_KLD];
    __shared__ __attribute__((aligned(16))) T sVt[CA_D * CA_VLD];
    __shared__ __attribute__((aligned(16))) T sP[CA_WAVES * 16 * CA_VLD];

    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t row0 = (size_t)b * L;
    const T* Kh = K + h * CA_D;
    const T* Vh = V + h * CA_D;
    const T* Qh = Q + h * CA_D;
    T* Oh = O + h * CA_D;

    // stage K and V^T of this head; rows >= L are zeros
    for (int i = tid; i < CA_LMAX * (CA_D / 8); i += CA_WAVES * 64) {
        const int r = i >> 3, c8 = (i & 7) * 8;
        V8 kv, vv;
#pragma unroll
        for (int e = 0; e < 8; ++e) { kv[e] = (T)0.f; vv[e] = (T)0.f; }
        if (r < L) {
            kv = *reinterpret_cast<const V8*>(Kh + (row0 + r) * (size_t)ldk + c8);
            vv = *reinterpret_cast<const V8*>(Vh + (row0 + r) * (size_t)ldv + c8);
        }
        *reinterpret_cast<V8*>(&sK[r * CA_KLD + c8]) = kv;
#pragma unroll
        for (int e = 0; e < 8; ++e) sVt[(c8 + e) * CA_VLD + r] = vv[e];
    }
    __syncthreads();

    const int nqt = (L + 15) >> 4;
    const int lr = lane & 15, lg = lane >> 4;
    T* myP = sP + w * 16 * CA_VLD;

    for (int it = 0; it < CA_LMAX / 16 / CA_WAVES; ++it) {
        const int qt = w + it * CA_WAVES;           // wave-uniform
        const bool active = qt < nqt;
        const int q0 = qt * 16;
        f32x4 s[8];
        float rsum[4] = {1.f, 1.f, 1.f, 1.f};
        if (active) {
            // Q fragments (A operand): row q0 + lr, k = 32 ks + 8 lg + j
            V8 qa[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int e = 0; e < 8; ++e) qa[ks][e] = (T)0.f;
                if (q0 + lr < L) qa[ks] = *reinterpret_cast<const V8*>(Qh + (row0 + q0 + lr) * (size_t)ldq + ks * 32 + lg * 8);
            }
#pragma unroll
            for (int kt = 0; kt < 8; ++kt) {
                s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (kt <= qt) {
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const V8 kb = *reinterpret_cast<const V8*>(&sK[(kt * 16 + lr) * CA_KLD + ks * 32 + lg * 8]);      // B operand: key kt*16 + lr
                        s[kt] = Tag::mfma16(qa[ks], kb, s[kt]);
                    }
                }
            }
            // C/D layout: s[kt][r] is (query q0 + 4 lg + r, key 16 kt + lr)
            float m[4] = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
#pragma unroll
            for (int kt = 0; kt < 8; ++kt) {
                if (kt <= qt) {
                    const int key = kt * 16 + lr;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool vis = key <= q0 + lg * 4 + r && key < L;
                        s[kt][r] *= scale_log2e;
                        m[r] = vis ? fmaxf(m[r], s[kt][r]) : m[r];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) m[r] = fmaxf(m[r], __shfl_xor(m[r], o, 64));
            float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kt = 0; kt < 8; ++kt) {
                if (kt <= (qt | 1)) {                // the PV step covers 32 keys: the odd partner tile of an even qt holds zeros
                    const int key = kt * 16 + lr;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool vis = kt <= qt && key <= q0 + lg * 4 + r && key < L;
                        const float p = vis ? exp2f(s[kt][r] - m[r]) : 0.f;
                        sum[r] += p;
                        myP[(lg * 4 + r) * CA_VLD + key] = Tag::from_f32(p);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) sum[r] += __shfl_xor(sum[r], o, 64);
                rsum[r] = sum[r];
            }
        }
        __syncthreads();          // P of this wave is in LDS (block barrier: every wave runs the same number of iterations)
        if (active) {
            f32x4 acc[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int nks = (qt >> 1) + 1;          // 32-key steps that cover key tiles 0..qt
            for (int kk = 0; kk < nks; ++kk) {
                const V8 pa = *reinterpret_cast<const V8*>(&myP[lr * CA_VLD + kk * 32 + lg * 8]);                   // A operand: query q0 + lr
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const V8 vb = *reinterpret_cast<const V8*>(&sVt[(nt * 16 + lr) * CA_VLD + kk * 32 + lg * 8]);      // B operand: column nt*16 + lr
                    acc[nt] = Tag::mfma16(pa, vb, acc[nt]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + lg * 4 + r;
                if (q < L) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) Oh[(row0 + q) * (size_t)ldo + nt * 16 + lr] = Tag::from_f32(acc[nt][r] / rsum[r]);
                }
            }
        }
        __syncthreads();          // the P tile is free for the next iteration
    }
}

template <class Tag>
int launch_attention_causal(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int L, int heads, float scale,
                            hipStream_t s) {
    typedef typename Tag::T T;
    k_attention_causal<Tag><<<(unsigned)(B * heads), CA_WAVES * 64, 0, s>>>((const T*)Q, ldq, (const T*)K, ldk, (const T*)V, ldv, (T*)O, ldo, L, heads,
                                                                         scale * 1.4426950408889634f);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// embedding: out[b, i, :] = tok[ids[b, i]] + pos[i]; one thread per 8 channels
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_clip_embed(const int* __restrict__ ids, const typename Tag::T* __restrict__ tok, const typename Tag::T* __restrict__ pos,
                                                    typename Tag::T* __restrict__ out, int L, int C8, int vocab, long long total) {
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / C8;
    const int c8 = (int)(i - row * C8), p = (int)(row % L);
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);      // callers validate the ids; a bad one must still not read outside the table
    const V8 a = reinterpret_cast<const V8*>(tok)[(size_t)id * C8 + c8], e = reinterpret_cast<const V8*>(pos)[(size_t)p * C8 + c8];
    V8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = Tag::from_f32(Tag::to_f32(a[k]) + Tag::to_f32(e[k]));
    reinterpret_cast<V8*>(out)[i] = o;
}

template <class Tag>
int launch_clip_embed(const int* ids, const void* tok, const void* pos, void* out, int B, int L, int C, int vocab, hipStream_t s) {
    typedef typename Tag::T T;
    const long long total = (long long)B * L * (C / 8);
    k_clip_embed<Tag><<<mve_cdiv(total, 256), 256, 0, s>>>(ids, (const T*)tok, (const T*)pos, (T*)out, L, C / 8, vocab, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// activation: quick_gelu x * sigmoid(1.702 x) (transformers QuickGELUActivation), gelu 0.5 x (1 + erf(x / sqrt 2)) (nn.GELU())
// ---------------------------------------------------------------------------------------------------
template <class Tag, int KIND>
__global__ __launch_bounds__(256) void k_act(const typename Tag::T* __restrict__ x, typename Tag::T* __restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = Tag::to_f32(x[i]);
        float r;
        if (KIND == MVE_ACT_QUICK_GELU) r = v / (1.f + expf(-1.702f * v));
        else r = 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
        y[i] = Tag::from_f32(r);
    }
}

template <class Tag>
int launch_act(int kind, const void* x, void* y, size_t n, hipStream_t s) {
    typedef typename Tag::T T;
    const unsigned grid = (n + 255) / 256 > 65535 ? 65535u : (unsigned)((n + 255) / 256);
    if (kind == MVE_ACT_QUICK_GELU) k_act<Tag, MVE_ACT_QUICK_GELU><<<grid, 256, 0, s>>>((const T*)x, (T*)y, n);
    else k_act<Tag, MVE_ACT_GELU><<<grid, 256, 0, s>>>((const T*)x, (T*)y, n);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// pooling: out[b, :] = x[b, pos(b), :], pos chosen on the device by transformers' two rules; one block per batch item, every thread scans
// the item's L ids (L is a text length)
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_clip_pool(const typename Tag::T* __restrict__ x, const int* __restrict__ ids, typename Tag::T* __restrict__ out, int L, int C,
                                                   int eos) {
    const int b = blockIdx.x;
    const int* row = ids + (size_t)b * L;
    int pos = 0;
    if (eos == 2) {               // legacy: ids.argmax(-1), the first position of the maximum
        int best = row[0];
        for (int i = 1; i < L; ++i) { const int v = row[i]; if (v > best) { best = v; pos = i; } }
    } else {                      // (ids == eos).int().argmax(-1): the first match, 0 without one
        for (int i = 0; i < L; ++i) if (row[i] == eos) { pos = i; break; }
    }
    const typename Tag::T* src = x + ((size_t)b * L + pos) * C;
    for (int c = threadIdx.x; c < C; c += 256) out[(size_t)b * C + c] = src[c];
}

template <class Tag>
int launch_clip_pool(const void* x, const int* ids, void* out, int B, int L, int C, int eos, hipStream_t s) {
    typedef typename Tag::T T;
    k_clip_pool<Tag><<<(unsigned)B, 256, 0, s>>>((const T*)x, ids, (T*)out, L, C, eos);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mve_attention_causal(int dtype, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int L, int heads,
                                    int head_dim, float scale, void* stream) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "attention_causal: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(Q && K && V && O, MVE_ERR_ARG, "attention_causal: null pointer (d_Q / d_K / d_V / d_O)");
    MVE_CHECK(head_dim == CA_D, MVE_ERR_ARG, "attention_causal: head_dim %d must be 64", head_dim);
    MVE_CHECK(L >= 1 && L <= CA_LMAX, MVE_ERR_ARG, "attention_causal: L %d must be in [1, 128]", L);
    MVE_CHECK(B >= 1 && heads >= 1 && (long long)B * heads < (1ll << 31), MVE_ERR_ARG, "attention_causal: bad B %d / heads %d", B, heads);
    const int width = heads * CA_D;
    MVE_CHECK(ldq >= width && ldq % 8 == 0, MVE_ERR_ARG, "attention_causal: ldq %d must be a multiple of 8 and >= heads * 64", ldq);
    MVE_CHECK(ldk >= width && ldk % 8 == 0, MVE_ERR_ARG, "attention_causal: ldk %d must be a multiple of 8 and >= heads * 64", ldk);
    MVE_CHECK(ldv >= width && ldv % 8 == 0, MVE_ERR_ARG, "attention_causal: ldv %d must be a multiple of 8 and >= heads * 64", ldv);
    MVE_CHECK(ldo >= width, MVE_ERR_ARG, "attention_causal: ldo %d must be >= heads * 64", ldo);
    MVE_CHECK(aligned16(Q) && aligned16(K) && aligned16(V), MVE_ERR_ARG, "attention_causal: d_Q / d_K / d_V must be 16-byte aligned");
    MVE_CHECK(scale == scale && scale > 0.f, MVE_ERR_ARG, "attention_causal: scale must be positive");
    return MVE_DISPATCH_16(dtype, launch_attention_causal, Q, ldq, K, ldk, V, ldv, O, ldo, B, L, heads, scale, (hipStream_t)stream);
}

extern "C" int mve_clip_embed(int dtype, const int32_t* ids, const void* tok, const void* pos, void* out, int B, int L, int C, int vocab, int max_pos, void* stream) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "clip_embed: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(ids && tok && pos && out, MVE_ERR_ARG, "clip_embed: null pointer (d_ids / d_tok / d_pos / d_out)");
    MVE_CHECK(B >= 1 && L >= 1, MVE_ERR_ARG, "clip_embed: bad B %d / L %d", B, L);
    MVE_CHECK(vocab >= 1 && max_pos >= 1, MVE_ERR_ARG, "clip_embed: bad vocab %d / max_pos %d", vocab, max_pos);
    MVE_CHECK(L <= max_pos, MVE_ERR_ARG, "clip_embed: L %d exceeds max_pos %d (max_position_embeddings)", L, max_pos);
    MVE_CHECK(C >= 8 && C % 8 == 0, MVE_ERR_ARG, "clip_embed: C %d must be a multiple of 8", C);
    MVE_CHECK(aligned16(tok) && aligned16(pos) && aligned16(out), MVE_ERR_ARG, "clip_embed: d_tok / d_pos / d_out must be 16-byte aligned");
    return MVE_DISPATCH_16(dtype, launch_clip_embed, (const int*)ids, tok, pos, out, B, L, C, vocab, (hipStream_t)stream);
}

extern "C" int mve_act(int dtype, int kind, const void* x, void* y, size_t n, void* stream) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "act: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(kind == MVE_ACT_QUICK_GELU || kind == MVE_ACT_GELU, MVE_ERR_ARG, "act: kind %d (0 = quick_gelu, 1 = gelu)", kind);
    MVE_CHECK(x && y, MVE_ERR_ARG, "act: null pointer (d_x / d_y)");
    if (n == 0) return MVE_OK;
    return MVE_DISPATCH_16(dtype, launch_act, kind, x, y, n, (hipStream_t)stream);
}

extern "C" int mve_clip_pool(int dtype, const void* x, const int32_t* ids, void* out, int B, int L, int C, int eos_token_id, void* stream) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "clip_pool: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(x && ids && out, MVE_ERR_ARG, "clip_pool: null pointer (d_x / d_ids / d_out)");
    MVE_CHECK(B >= 1 && L >= 1 && C >= 1, MVE_ERR_ARG, "clip_pool: bad B %d / L %d / C %d", B, L, C);
    return MVE_DISPATCH_16(dtype, launch_clip_pool, x, (const int*)ids, out, B, L, C, eos_token_id, (hipStream_t)stream);
}
