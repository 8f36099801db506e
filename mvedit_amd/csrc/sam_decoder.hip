// Segment Anything prompt encoder, two-way mask decoder and mask post-processing primitives (include/mvedit_amd.h section 2h): what
// `SamPredictor.predict` runs behind the image encoder (lib/apis/adapter3d.py:721-735, lib/pipelines/utils.py:108-146).  The arithmetic is
// transformers' SamPromptEncoder / SamMaskDecoder / SamPositionalEmbedding (models/sam/modeling_sam.py), the same as segment_anything's; the plan
// that strings the kernels together is csrc/builder_sam_decoder.h.
//
// EVERYTHING here is fp32: fp32 parameters, fp32 activations, fp32 accumulation (a 16-bit decoder sits 1e-1 .. 6e-1 from float64 on
// the masks).  The only 16-bit tensor read is the image encoder's embedding (mve_sam_src), the only one written the encoder's input pixels
// (mve_sam_preprocess).  No atomics and no split-K: every output element is one fixed chain of operations, two runs give the same bits, and an
// item's result does not depend on how many items share the launch.  The GEMM is plain VALU FMA on LDS tiles: gfx950's fp32 MFMA runs at the
// vector rate, and at 1.3 GFLOP per prompt neither is a bottleneck.  One timing exists (profiles/sam_decoder.txt); nothing here is tuned.
#include "common.h"

#include <math.h>

namespace {

constexpr float SD_NEG = -3.0e38f;      // the running maximum before the first key: finite, so no infinity is ever formed

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------------------
// out [M, N] = A [M, K] . W [N, K]^T (+ bias[N]) (+ res [M, N]) (ReLU): 64 x 64 output tile per block of 256 threads, 4 x 4 per thread, K in steps
// of 16 through LDS.  Each step's 16 products are summed into a fresh partial that is then added to the running sum: a two-level sum in a fixed
// order (k ascending inside a step, steps ascending), whose rounding error grows with sqrt(16) + sqrt(K / 16) instead of sqrt(K).  An element's
// chain does not depend on M, on the tile it falls in or on its neighbours.
// ---------------------------------------------------------------------------------------------------
constexpr int GT = 64, GK = 16;

template <bool RELU>
__global__ __launch_bounds__(256) void k_gemm_f32(const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw, const float* __restrict__ bias,
                                                  const float* __restrict__ res, int ldr, float* __restrict__ out, int ldc, int M, int N, int K) {
    __shared__ float sA[GK][GT + 4], sW[GK][GT + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
    const int lr = tid >> 2, lk = (tid & 3) * 4;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < K; k0 += GK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + lk + e;
            sA[lk + e][lr] = (m0 + lr < M && k < K) ? A[(size_t)(m0 + lr) * lda + k] : 0.f;
            sW[lk + e][lr] = (n0 + lr < N && k < K) ? W[(size_t)(n0 + lr) * ldw + k] : 0.f;
        }
        __syncthreads();
        float part[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[i][j] = 0.f;
#pragma unroll
        for (int k = 0; k < GK; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = sA[k][ty * 4 + i]; b[i] = sW[k][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[i][j] = fmaf(a[i], b[j], part[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += part[i][j];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n >= N) continue;
            float v = acc[i][j];
            if (bias) v += bias[n];
            if (res) v += res[(size_t)m * ldr + n];
            if (RELU) v = fmaxf(v, 0.f);
            out[(size_t)m * ldc + n] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// attention, fp32.  Two kernels, chosen by Lk alone:
//   Lk <= 16 (keys are the prompt tokens): one thread per (item, query, head) walks the keys with an online softmax;
//   Lk  > 16 (keys are the image): one block of 256 threads per (item, query, head); thread t walks keys t, t + 256, ... with an online softmax and
//            the 256 partial (max, sum, acc) triples are merged by a tree over LDS in a fixed order.
// A thread without a key holds (SD_NEG, 0, 0) and merges as nothing.  The tail is a guard on the key index, never a value: no infinity is formed.
// ---------------------------------------------------------------------------------------------------
template <int HD>
__device__ __forceinline__ void attn_step(const float (&q)[HD], const float* __restrict__ kr, const float* __restrict__ vr, float scale, float& m, float& sum,
                                          float (&acc)[HD]) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
        const float4 k4 = *reinterpret_cast<const float4*>(kr + c);
        s = fmaf(q[c], k4.x, s); s = fmaf(q[c + 1], k4.y, s); s = fmaf(q[c + 2], k4.z, s); s = fmaf(q[c + 3], k4.w, s);
    }
    s *= scale;
    const float mn = fmaxf(m, s), corr = expf(m - mn), p = expf(s - mn);
    sum = sum * corr + p;
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
        const float4 v4 = *reinterpret_cast<const float4*>(vr + c);
        acc[c] = acc[c] * corr + p * v4.x; acc[c + 1] = acc[c + 1] * corr + p * v4.y;
        acc[c + 2] = acc[c + 2] * corr + p * v4.z; acc[c + 3] = acc[c + 3] * corr + p * v4.w;
    }
    m = mn;
}

template <int HD>
__global__ __launch_bounds__(256) void k_attn_f32_short(const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk, const float* __restrict__ V, int ldv,
                                                        float* __restrict__ O, int ldo, long long total, int Lq, int Lk, int heads, float scale) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int h = (int)(i % heads);
    const long long row = i / heads, n = row / Lq;      // row = n * Lq + query
    float q[HD], acc[HD], m = SD_NEG, sum = 0.f;
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
        const float4 q4 = *reinterpret_cast<const float4*>(Q + row * ldq + h * HD + c);
        q[c] = q4.x; q[c + 1] = q4.y; q[c + 2] = q4.z; q[c + 3] = q4.w;
        acc[c] = acc[c + 1] = acc[c + 2] = acc[c + 3] = 0.f;
    }
    for (int k = 0; k < Lk; ++k) attn_step<HD>(q, K + (n * Lk + k) * ldk + h * HD, V + (n * Lk + k) * ldv + h * HD, scale, m, sum, acc);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int c = 0; c < HD; c += 4)
        *reinterpret_cast<float4*>(O + row * ldo + h * HD + c) = make_float4(acc[c] * inv, acc[c + 1] * inv, acc[c + 2] * inv, acc[c + 3] * inv);
}

template <int HD>
__global__ __launch_bounds__(256) void k_attn_f32_long(const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk, const float* __restrict__ V, int ldv,
                                                       float* __restrict__ O, int ldo, int Lq, int Lk, int heads, float scale) {
    __shared__ float sm[256], ss[256], sa[256][HD + 1];
    const int tid = threadIdx.x;
    const int h = blockIdx.x % heads;
    const long long row = blockIdx.x / heads, n = row / Lq;
    float q[HD], acc[HD], m = SD_NEG, sum = 0.f;
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
        const float4 q4 = *reinterpret_cast<const float4*>(Q + row * ldq + h * HD + c);
        q[c] = q4.x; q[c + 1] = q4.y; q[c + 2] = q4.z; q[c + 3] = q4.w;
        acc[c] = acc[c + 1] = acc[c + 2] = acc[c + 3] = 0.f;
    }
    for (int k = tid; k < Lk; k += 256) attn_step<HD>(q, K + (n * Lk + k) * ldk + h * HD, V + (n * Lk + k) * ldv + h * HD, scale, m, sum, acc);
    sm[tid] = m; ss[tid] = sum;
#pragma unroll
    for (int c = 0; c < HD; ++c) sa[tid][c] = acc[c];
    for (int st = 128; st >= 1; st >>= 1) {
        __syncthreads();
        if (tid < st) {
            const float m1 = sm[tid], m2 = sm[tid + st], mn = fmaxf(m1, m2), c1 = expf(m1 - mn), c2 = expf(m2 - mn);
            sm[tid] = mn;
            ss[tid] = ss[tid] * c1 + ss[tid + st] * c2;
#pragma unroll
            for (int c = 0; c < HD; ++c) sa[tid][c] = sa[tid][c] * c1 + sa[tid + st][c] * c2;
        }
    }
    __syncthreads();
    if (tid < HD) O[row * ldo + h * HD + tid] = sa[0][tid] / ss[0];
}

template <int HD>
int launch_attn(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int NB, int Lq, int Lk, int heads, float scale, hipStream_t s) {
    const long long total = (long long)NB * Lq * heads;
    if (Lk <= 16) k_attn_f32_short<HD><<<mve_cdiv(total, 256), 256, 0, s>>>(Q, ldq, K, ldk, V, ldv, O, ldo, total, Lq, Lk, heads, scale);
    else k_attn_f32_long<HD><<<(unsigned)total, 256, 0, s>>>(Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, heads, scale);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// row-wise helpers: LayerNorm over the last dimension (one wave per row, torch's two-pass mean / variance), y = x + pe[row mod period]
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_layernorm_f32(const float* __restrict__ x, float* __restrict__ y, long long rows, int C, const float* __restrict__ g,
                                                       const float* __restrict__ b, float eps) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + row * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xr[c];
    const float mean = wave_sum(s) / (float)C;
    float v = 0.f;
    for (int c = lane; c < C; c += 64) { const float d = xr[c] - mean; v = fmaf(d, d, v); }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)C + eps);
    for (int c = lane; c < C; c += 64) y[row * C + c] = (xr[c] - mean) * rstd * g[c] + b[c];
}

__global__ __launch_bounds__(256) void k_add_rows_f32(const float* __restrict__ x, const float* __restrict__ pe, float* __restrict__ y, long long total, long long period) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) y[i] = x[i] + pe[i % period];
}

// ---------------------------------------------------------------------------------------------------
// prompt encoder
// ---------------------------------------------------------------------------------------------------
// SamPositionalEmbedding.forward on one normalised coordinate pair: c = 2 c - 1, c @ gaussian [2, C/2], times 2 pi, [sin | cos]
__device__ __forceinline__ void pos_enc(float cx, float cy, const float* __restrict__ gauss, int half, int j, float& sn, float& cs) {
    cx = 2.0f * cx - 1.0f; cy = 2.0f * cy - 1.0f;
    const float v = 6.283185307179586f * (cx * gauss[j] + cy * gauss[half + j]);
    sn = sinf(v); cs = cosf(v);
}

__global__ __launch_bounds__(256) void k_sam_dense_pe(const float* __restrict__ gauss, float* __restrict__ out, int G, int C) {
    const int half = C / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)G * G * half) return;
    const int j = (int)(i % half), cell = (int)(i / half), cy = cell / G, cx = cell - cy * G;
    float sn, cs;
    pos_enc(((float)cx + 0.5f) / (float)G, ((float)cy + 0.5f) / (float)G, gauss, half, j, sn, cs);
    out[(size_t)cell * C + j] = sn;
    out[(size_t)cell * C + half + j] = cs;
}

// one block per (item, token): iou token, mask tokens, points (+ the padding point), box corners
__global__ __launch_bounds__(128) void k_sam_prompt_tokens(const float* __restrict__ boxes, const float* __restrict__ points, const int* __restrict__ labels, int Np, int pad,
                                                           const float* __restrict__ gauss, const float* __restrict__ point_embed, const float* __restrict__ not_a_point,
                                                           const float* __restrict__ iou_token, const float* __restrict__ mask_tokens, float* __restrict__ out, int T, int Mt,
                                                           int C, float S) {
    const int t = blockIdx.x % T, n = blockIdx.x / T, half = C / 2;
    float* o = out + (size_t)blockIdx.x * C;
    if (t < 1 + Mt) {
        const float* src = t == 0 ? iou_token : mask_tokens + (size_t)(t - 1) * C;
        for (int c = threadIdx.x; c < C; c += blockDim.x) o[c] = src[c];
        return;
    }
    const int s = t - 1 - Mt, npt = Np + pad;
    float x, y;
    int label;          // -1 / 0 / 1: a point; 2 / 3: a box corner (the index of its point_embed row)
    if (s < npt) {
        if (s < Np) { x = points[((size_t)n * Np + s) * 2]; y = points[((size_t)n * Np + s) * 2 + 1]; label = labels[(size_t)n * Np + s]; }
        else { x = 0.f; y = 0.f; label = -1; }
    } else {
        const int k = s - npt;
        x = boxes[(size_t)n * 4 + 2 * k]; y = boxes[(size_t)n * 4 + 2 * k + 1]; label = 2 + k;
    }
    if (label == -1) {
        for (int c = threadIdx.x; c < C; c += blockDim.x) o[c] = not_a_point[c];
        return;
    }
    const float* add = label >= 0 && label <= 3 ? point_embed + (size_t)label * C : nullptr;      // any other label: the bare encoding, as the reference's `where` chain
    for (int j = threadIdx.x; j < half; j += blockDim.x) {
        float sn, cs;
        pos_enc((x + 0.5f) / S, (y + 0.5f) / S, gauss, half, j, sn, cs);
        o[j] = sn + (add ? add[j] : 0.f);
        o[half + j] = cs + (add ? add[half + j] : 0.f);
    }
}

// embedding [B, C, G2] (16 bit, NCHW) -> rows [N, G2, C] fp32 of image n / P, plus no_mask_embed[C]: a 32 x 32 transpose through LDS
template <class Tag>
__global__ __launch_bounds__(256) void k_sam_src(const typename Tag::T* __restrict__ emb, const float* __restrict__ no_mask, float* __restrict__ out, int P, int C, int G2) {
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32, n = blockIdx.z, b = n / P;
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, p = p0 + tx;
        if (c < C && p < G2) t[i][tx] = Tag::to_f32(emb[((size_t)b * C + c) * G2 + p]);
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + i, c = c0 + tx;
        if (p < G2 && c < C) out[((size_t)n * G2 + p) * C + c] = t[tx][i] + no_mask[c];
    }
}

// ---------------------------------------------------------------------------------------------------
// ConvTranspose2d(k = 2, s = 2) behind its GEMM: y4 [N Gi Gi, 4 Co] with column (2 ky + kx) Co + co -> out [N, 2 Gi, 2 Gi, Co] rows, + bias, then
// mode 1: LayerNorm2d over the channels of the pixel (affine) and erf GELU; mode 2: erf GELU.  One wave per output pixel.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sam_upscale_shuffle(const float* __restrict__ y4, const float* __restrict__ bias, const float* __restrict__ g,
                                                             const float* __restrict__ b, float eps, float* __restrict__ out, long long pixels, int Gi, int Co, int mode) {
    const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pix >= pixels) return;
    const int Go = 2 * Gi;
    const int X = (int)(pix % Go), Y = (int)((pix / Go) % Go);
    const long long n = pix / ((long long)Go * Go);
    const float* src = y4 + ((n * Gi + (Y >> 1)) * Gi + (X >> 1)) * 4 * Co + ((Y & 1) * 2 + (X & 1)) * Co;
    float mean = 0.f, rstd = 1.f;
    if (mode == 1) {
        float s = 0.f;
        for (int c = lane; c < Co; c += 64) s += src[c] + bias[c];
        mean = wave_sum(s) / (float)Co;
        float v = 0.f;
        for (int c = lane; c < Co; c += 64) { const float d = (src[c] + bias[c]) - mean; v = fmaf(d, d, v); }
        rstd = 1.0f / sqrtf(wave_sum(v) / (float)Co + eps);
    }
    for (int c = lane; c < Co; c += 64) {
        float v = src[c] + bias[c];
        if (mode == 1) v = (v - mean) * rstd * g[c] + b[c];
        out[pix * Co + c] = gelu_erf(v);
    }
}

// ---------------------------------------------------------------------------------------------------
// the Mt hypernetwork MLPs and the iou head: one block per (item, MLP j); j < Mt reads token 1 + j and writes hyper[n, j, :O3], j == Mt reads
// token 0 and writes iou[n, :Mt].  Stacked weights: w0 [Mt+1][Hd][C], w1 [Mt+1][Hd][Hd], w2 [Mt+1][O3][Hd] (the iou head's rows first).  One wave
// per output, lanes over the inputs, a butterfly sum: a fixed order.
// ---------------------------------------------------------------------------------------------------
constexpr int SD_MLP_MAX = 512;

__device__ __forceinline__ void mlp_layer(const float* __restrict__ w, const float* __restrict__ bias, const float* in, float* outv, int nin, int nout, bool relu) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int o = wave; o < nout; o += 4) {
        float s = 0.f;
        for (int k = lane; k < nin; k += 64) s = fmaf(w[(size_t)o * nin + k], in[k], s);
        s = wave_sum(s) + bias[o];
        if (lane == 0) outv[o] = relu ? fmaxf(s, 0.f) : s;
    }
}

__global__ __launch_bounds__(256) void k_sam_token_mlps(const float* __restrict__ queries, int T, int C, int Hd, int O3, int Mt, const float* __restrict__ w0,
                                                        const float* __restrict__ b0, const float* __restrict__ w1, const float* __restrict__ b1,
                                                        const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ hyper, float* __restrict__ iou) {
    __shared__ float s0[SD_MLP_MAX], s1[SD_MLP_MAX];
    const int j = blockIdx.x % (Mt + 1), n = blockIdx.x / (Mt + 1);
    const float* in = queries + ((size_t)n * T + (j < Mt ? 1 + j : 0)) * C;
    for (int c = threadIdx.x; c < C; c += 256) s0[c] = in[c];
    __syncthreads();
    mlp_layer(w0 + (size_t)j * Hd * C, b0 + (size_t)j * Hd, s0, s1, C, Hd, true);
    __syncthreads();
    mlp_layer(w1 + (size_t)j * Hd * Hd, b1 + (size_t)j * Hd, s1, s0, Hd, Hd, true);
    __syncthreads();
    float* dst = j < Mt ? hyper + ((size_t)n * Mt + j) * O3 : iou + (size_t)n * Mt;
    mlp_layer(w2 + (size_t)j * O3 * Hd, b2 + (size_t)j * O3, s0, dst, Hd, j < Mt ? O3 : Mt, false);
}

// low_res[n, m, p] = sum_c hyper[n, m, c] up[n, p, c]: one thread per (item, pixel), c ascending
constexpr int SD_MP_MAX = 512;
__global__ __launch_bounds__(256) void k_sam_mask_product(const float* __restrict__ hyper, const float* __restrict__ up, float* __restrict__ low, int Mt, int Cu, int P2) {
    __shared__ float sh[SD_MP_MAX];
    const int n = blockIdx.y;
    for (int i = threadIdx.x; i < Mt * Cu; i += 256) sh[i] = hyper[(size_t)n * Mt * Cu + i];
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P2) return;
    const float* u = up + ((size_t)n * P2 + p) * Cu;
    for (int m = 0; m < Mt; ++m) {
        float s = 0.f;
        for (int c = 0; c < Cu; ++c) s = fmaf(sh[m * Cu + c], u[c], s);
        low[((size_t)n * Mt + m) * P2 + p] = s;
    }
}

// ---------------------------------------------------------------------------------------------------
// image pre- and mask post-processing
// ---------------------------------------------------------------------------------------------------
struct Norm3 { float mean[3], std[3]; };

template <class Tag>
__global__ __launch_bounds__(256) void k_sam_preprocess(const uint8_t* __restrict__ img, int h, int w, int S, Norm3 nm, typename Tag::T* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 3ll * S * S) return;
    const int x = (int)(i % S), y = (int)((i / S) % S), c = (int)(i / ((long long)S * S));
    float v = 0.f;
    if (y < h && x < w) v = ((float)img[((size_t)y * w + x) * 3 + c] - nm.mean[c]) / nm.std[c];
    out[i] = Tag::from_f32(v);
}

// ATen's upsample_bilinear2d source index (align_corners = False): src = max((dst + 0.5) scale - 0.5, 0), i0 = floor, i1 = min(i0 + 1, in - 1)
__device__ __forceinline__ void bilinear_src(int dst, float scale, int in, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
    const float src = fmaxf(((float)dst + 0.5f) * scale - 0.5f, 0.f);
    i0 = (int)src;
    i0 = i0 < in - 1 ? i0 : in - 1;
    i1 = i0 < in - 1 ? i0 + 1 : i0;
    l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}
__device__ __forceinline__ float bilinear_at(const float* __restrict__ p, int ld, int y0, int y1, float ly, int x0, int x1, float lx) {
    return (1.0f - ly) * ((1.0f - lx) * p[(size_t)y0 * ld + x0] + lx * p[(size_t)y0 * ld + x1]) + ly * ((1.0f - lx) * p[(size_t)y1 * ld + x0] + lx * p[(size_t)y1 * ld + x1]);
}

// low [NP, L, L] -> bilinear to S x S -> crop [:h_in, :w_in] -> bilinear to (H, W), composed: the four taps of the second resize are each a
// bilinear sample of the low-res map (16 reads per output pixel, no S x S buffer); mask = value > thr (the value that is written as the logit)
__global__ __launch_bounds__(256) void k_sam_postprocess(const float* __restrict__ low, int L, int S, int h_in, int w_in, int H, int W, float thr,
                                                         uint8_t* __restrict__ masks, float* __restrict__ logits, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int X = (int)(i % W), Y = (int)((i / W) % H);
    const float* p = low + (i / ((long long)W * H)) * L * L;
    const float s1 = (float)L / (float)S, sy2 = (float)h_in / (float)H, sx2 = (float)w_in / (float)W;
    int ys[2], xs[2];
    float ly, lx;
    bilinear_src(Y, sy2, h_in, ys[0], ys[1], ly);
    bilinear_src(X, sx2, w_in, xs[0], xs[1], lx);
    float tap[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        int y0, y1; float wy;
        bilinear_src(ys[a], s1, L, y0, y1, wy);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            int x0, x1; float wx;
            bilinear_src(xs[b], s1, L, x0, x1, wx);
            tap[a][b] = bilinear_at(p, L, y0, y1, wy, x0, x1, wx);
        }
    }
    const float v = (1.0f - ly) * ((1.0f - lx) * tap[0][0] + lx * tap[0][1]) + ly * ((1.0f - lx) * tap[1][0] + lx * tap[1][1]);
    masks[i] = v > thr ? 1 : 0;
    if (logits) logits[i] = v;
}

template <class Tag>
int launch_src(const void* emb, const float* no_mask, float* out, int N, int P, int C, int G2, hipStream_t s) {
    k_sam_src<Tag><<<dim3(mve_cdiv(G2, 32), mve_cdiv(C, 32), N), 256, 0, s>>>((const typename Tag::T*)emb, no_mask, out, P, C, G2);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}
template <class Tag>
int launch_preprocess(const uint8_t* img, int h, int w, int S, const Norm3& nm, void* out, hipStream_t s) {
    k_sam_preprocess<Tag><<<mve_cdiv(3ull * S * S, 256), 256, 0, s>>>(img, h, w, S, nm, (typename Tag::T*)out);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // namespace

extern "C" {

int mve_gemm_f32(const float* d_A, int lda, const float* d_W, int ldw, const float* d_bias, const float* d_res, int ldr, float* d_out, int ldc, int M, int N, int K,
                 int relu, void* stream) {
    MVE_CHECK(d_A && d_W && d_out, MVE_ERR_ARG, "gemm_f32: null pointer");
    MVE_CHECK(M >= 1 && N >= 1 && K >= 1, MVE_ERR_ARG, "gemm_f32: bad shape M %d N %d K %d", M, N, K);
    MVE_CHECK(lda >= K && ldw >= K && ldc >= N && (!d_res || ldr >= N), MVE_ERR_ARG, "gemm_f32: a leading dimension is shorter than its row");
    MVE_CHECK((M + GT - 1) / GT <= 65535, MVE_ERR_ARG, "gemm_f32: M %d exceeds 65535 row tiles", M);
    const dim3 grid(mve_cdiv(N, GT), mve_cdiv(M, GT));
    if (relu) k_gemm_f32<true><<<grid, 256, 0, (hipStream_t)stream>>>(d_A, lda, d_W, ldw, d_bias, d_res, ldr, d_out, ldc, M, N, K);
    else k_gemm_f32<false><<<grid, 256, 0, (hipStream_t)stream>>>(d_A, lda, d_W, ldw, d_bias, d_res, ldr, d_out, ldc, M, N, K);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_attention_f32(const float* d_Q, int ldq, const float* d_K, int ldk, const float* d_V, int ldv, float* d_O, int ldo, int NB, int Lq, int Lk, int heads,
                      int head_dim, float scale, void* stream) {
    MVE_CHECK(d_Q && d_K && d_V && d_O, MVE_ERR_ARG, "attention_f32: null pointer");
    MVE_CHECK(head_dim == 16 || head_dim == 32, MVE_ERR_ARG, "attention_f32: head_dim %d must be 16 or 32", head_dim);
    MVE_CHECK(NB >= 1 && Lq >= 1 && Lk >= 1 && heads >= 1, MVE_ERR_ARG, "attention_f32: bad shape NB %d Lq %d Lk %d heads %d", NB, Lq, Lk, heads);
    const int C = heads * head_dim;
    MVE_CHECK(ldq >= C && ldk >= C && ldv >= C && ldo >= C && ((ldq | ldk | ldv | ldo) & 3) == 0, MVE_ERR_ARG,
              "attention_f32: row strides must be multiples of 4 and at least heads * head_dim = %d", C);
    MVE_CHECK(aligned16(d_Q) && aligned16(d_K) && aligned16(d_V) && aligned16(d_O), MVE_ERR_ARG, "attention_f32: pointers must be 16-byte aligned");
    MVE_CHECK((long long)NB * Lq * heads < (1ll << 31), MVE_ERR_ARG, "attention_f32: NB Lq heads overflows the grid");
    if (head_dim == 16) return launch_attn<16>(d_Q, ldq, d_K, ldk, d_V, ldv, d_O, ldo, NB, Lq, Lk, heads, scale, (hipStream_t)stream);
    return launch_attn<32>(d_Q, ldq, d_K, ldk, d_V, ldv, d_O, ldo, NB, Lq, Lk, heads, scale, (hipStream_t)stream);
}

int mve_layernorm_f32(const float* d_x, float* d_y, int rows, int C, const float* d_gamma, const float* d_beta, float eps, void* stream) {
    MVE_CHECK(d_x && d_y && d_gamma && d_beta && rows >= 1 && C >= 1, MVE_ERR_ARG, "layernorm_f32: bad arguments");
    k_layernorm_f32<<<mve_cdiv(rows, 4), 256, 0, (hipStream_t)stream>>>(d_x, d_y, rows, C, d_gamma, d_beta, eps);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_add_rows_f32(const float* d_x, const float* d_pe, float* d_y, int rows, int C, int period_rows, void* stream) {
    MVE_CHECK(d_x && d_pe && d_y && rows >= 1 && C >= 1 && period_rows >= 1, MVE_ERR_ARG, "add_rows_f32: bad arguments");
    const long long total = (long long)rows * C;
    MVE_CHECK((total + 255) / 256 < (1ll << 31), MVE_ERR_ARG, "add_rows_f32: too many elements");
    k_add_rows_f32<<<mve_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(d_x, d_pe, d_y, total, (long long)period_rows * C);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_sam_dense_pe(const float* d_gaussian, float* d_out, int G, int C, void* stream) {
    MVE_CHECK(d_gaussian && d_out && G >= 1 && G <= 1024 && C >= 2 && C % 2 == 0, MVE_ERR_ARG, "sam_dense_pe: bad arguments (G %d, C %d)", G, C);
    k_sam_dense_pe<<<mve_cdiv((unsigned long long)G * G * (C / 2), 256), 256, 0, (hipStream_t)stream>>>(d_gaussian, d_out, G, C);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_sam_prompt_tokens(const float* d_boxes, const float* d_points, const int32_t* d_labels, int N, int n_points, const float* d_gaussian, const float* d_point_embed,
                          const float* d_not_a_point, const float* d_iou_token, const float* d_mask_tokens, int num_mask_tokens, int C, float image_size, float* d_out,
                          int T, void* stream) {
    MVE_CHECK(d_gaussian && d_point_embed && d_not_a_point && d_iou_token && d_mask_tokens && d_out, MVE_ERR_ARG, "sam_prompt_tokens: null pointer");
    MVE_CHECK(N >= 1 && n_points >= 0 && num_mask_tokens >= 1 && C >= 2 && C % 2 == 0 && image_size > 0.f, MVE_ERR_ARG, "sam_prompt_tokens: bad arguments");
    MVE_CHECK(d_boxes || n_points > 0, MVE_ERR_ARG, "sam_prompt_tokens: no prompt (neither a box nor points)");
    MVE_CHECK(n_points == 0 || (d_points && d_labels), MVE_ERR_ARG, "sam_prompt_tokens: %d points without coordinates / labels", n_points);
    const int pad = n_points > 0 && !d_boxes ? 1 : 0;
    const int want = 1 + num_mask_tokens + n_points + pad + (d_boxes ? 2 : 0);
    MVE_CHECK(T == want, MVE_ERR_ARG, "sam_prompt_tokens: T %d, the prompt has %d tokens", T, want);
    MVE_CHECK(T <= 16, MVE_ERR_ARG, "sam_prompt_tokens: %d tokens exceed 16", T);
    MVE_CHECK((long long)N * T < (1ll << 31), MVE_ERR_ARG, "sam_prompt_tokens: N T overflows the grid");
    k_sam_prompt_tokens<<<(unsigned)(N * T), 128, 0, (hipStream_t)stream>>>(d_boxes, d_points, d_labels, n_points, pad, d_gaussian, d_point_embed, d_not_a_point, d_iou_token,
                                                                             d_mask_tokens, d_out, T, num_mask_tokens, C, image_size);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_sam_src(int dtype, const void* d_embedding, const float* d_no_mask_embed, float* d_out, int N, int P, int C, int G, void* stream) {
    MVE_CHECK(d_embedding && d_no_mask_embed && d_out, MVE_ERR_ARG, "sam_src: null pointer");
    MVE_CHECK(N >= 1 && N <= 65535 && P >= 1 && N % P == 0 && C >= 1 && G >= 1 && G <= 1024, MVE_ERR_ARG, "sam_src: bad arguments (N %d, P %d, C %d, G %d)", N, P, C, G);
    return MVE_DISPATCH_16(dtype, launch_src, d_embedding, d_no_mask_embed, d_out, N, P, C, G * G, (hipStream_t)stream);
}

int mve_sam_upscale(const float* d_x, const float* d_W4, const float* d_bias, const float* d_ln_gamma, const float* d_ln_beta, float eps, float* d_tmp, float* d_out, int N,
                    int Gi, int Cin, int Cout, int mode, void* stream) {
    MVE_CHECK(d_x && d_W4 && d_bias && d_tmp && d_out, MVE_ERR_ARG, "sam_upscale: null pointer");
    MVE_CHECK(mode == 1 || mode == 2, MVE_ERR_ARG, "sam_upscale: mode %d (1 = LayerNorm2d + GELU, 2 = GELU)", mode);
    MVE_CHECK(mode == 2 || (d_ln_gamma && d_ln_beta), MVE_ERR_ARG, "sam_upscale: mode 1 needs the LayerNorm2d parameters");
    MVE_CHECK(N >= 1 && Gi >= 1 && Gi <= 2048 && Cin >= 1 && Cout >= 1 && (long long)N * Gi * Gi < (1ll << 22), MVE_ERR_ARG, "sam_upscale: bad shape");
    const int rc = mve_gemm_f32(d_x, Cin, d_W4, Cin, nullptr, nullptr, 0, d_tmp, 4 * Cout, N * Gi * Gi, 4 * Cout, Cin, 0, stream);
    if (rc) return rc;
    const long long pixels = 4ll * N * Gi * Gi;
    k_sam_upscale_shuffle<<<mve_cdiv(pixels, 4), 256, 0, (hipStream_t)stream>>>(d_tmp, d_bias, d_ln_gamma, d_ln_beta, eps, d_out, pixels, Gi, Cout, mode);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_sam_token_mlps(const float* d_queries, int N, int T, int C, int hidden, int out_dim, int num_mask_tokens, const float* d_w0, const float* d_b0, const float* d_w1,
                       const float* d_b1, const float* d_w2, const float* d_b2, float* d_hyper, float* d_iou, void* stream) {
    MVE_CHECK(d_queries && d_w0 && d_b0 && d_w1 && d_b1 && d_w2 && d_b2 && d_hyper && d_iou, MVE_ERR_ARG, "sam_token_mlps: null pointer");
    MVE_CHECK(N >= 1 && num_mask_tokens >= 1 && T >= 1 + num_mask_tokens, MVE_ERR_ARG, "sam_token_mlps: bad N %d / T %d / num_mask_tokens %d", N, T, num_mask_tokens);
    MVE_CHECK(C >= 1 && C <= SD_MLP_MAX && hidden >= 1 && hidden <= SD_MLP_MAX && out_dim >= num_mask_tokens && out_dim <= SD_MLP_MAX, MVE_ERR_ARG,
              "sam_token_mlps: widths C %d / hidden %d / out_dim %d must be at most %d, out_dim at least num_mask_tokens", C, hidden, out_dim, SD_MLP_MAX);
    MVE_CHECK((long long)N * (num_mask_tokens + 1) < (1ll << 31), MVE_ERR_ARG, "sam_token_mlps: N overflows the grid");
    k_sam_token_mlps<<<(unsigned)(N * (num_mask_tokens + 1)), 256, 0, (hipStream_t)stream>>>(d_queries, T, C, hidden, out_dim, num_mask_tokens, d_w0, d_b0, d_w1, d_b1, d_w2,
                                                                                               d_b2, d_hyper, d_iou);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_sam_mask_product(const float* d_hyper, const float* d_up, float* d_low_res, int N, int num_mask_tokens, int Cu, int pixels, void* stream) {
    MVE_CHECK(d_hyper && d_up && d_low_res, MVE_ERR_ARG, "sam_mask_product: null pointer");
    MVE_CHECK(N >= 1 && N <= 65535 && num_mask_tokens >= 1 && Cu >= 1 && pixels >= 1 && num_mask_tokens * Cu <= SD_MP_MAX, MVE_ERR_ARG,
              "sam_mask_product: bad shape (N %d, masks %d, channels %d, pixels %d; masks x channels at most %d)", N, num_mask_tokens, Cu, pixels, SD_MP_MAX);
    k_sam_mask_product<<<dim3(mve_cdiv(pixels, 256), N), 256, 0, (hipStream_t)stream>>>(d_hyper, d_up, d_low_res, num_mask_tokens, Cu, pixels);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_sam_preprocess(int dtype, const uint8_t* d_image, int h, int w, int S, const float* pixel_mean, const float* pixel_std, void* d_out, void* stream) {
    MVE_CHECK(d_image && d_out, MVE_ERR_ARG, "sam_preprocess: null pointer");
    MVE_CHECK(S >= 1 && S <= 8192 && h >= 1 && w >= 1 && h <= S && w <= S, MVE_ERR_ARG, "sam_preprocess: image %d x %d does not fit the %d x %d input", h, w, S, S);
    Norm3 nm{{123.675f, 116.28f, 103.53f}, {58.395f, 57.12f, 57.375f}};      // segment_anything's Sam.pixel_mean / pixel_std
    for (int c = 0; c < 3; ++c) {
        if (pixel_mean) nm.mean[c] = pixel_mean[c];
        if (pixel_std) nm.std[c] = pixel_std[c];
        MVE_CHECK(nm.std[c] > 0.f, MVE_ERR_ARG, "sam_preprocess: pixel_std[%d] must be positive", c);
    }
    return MVE_DISPATCH_16(dtype, launch_preprocess, d_image, h, w, S, nm, d_out, (hipStream_t)stream);
}

int mve_sam_postprocess(const float* d_low_res, int planes, int L, int S, int h_in, int w_in, int H, int W, float mask_threshold, uint8_t* d_masks, float* d_logits,
                        void* stream) {
    MVE_CHECK(d_low_res && d_masks, MVE_ERR_ARG, "sam_postprocess: null pointer");
    MVE_CHECK(planes >= 1 && L >= 1 && S >= 1 && h_in >= 1 && w_in >= 1 && h_in <= S && w_in <= S && H >= 1 && W >= 1, MVE_ERR_ARG,
              "sam_postprocess: bad shape (planes %d, low-res %d, input %d, crop %d x %d, output %d x %d)", planes, L, S, h_in, w_in, H, W);
    const long long total = (long long)planes * H * W;
    MVE_CHECK((total + 255) / 256 < (1ll << 31), MVE_ERR_ARG, "sam_postprocess: output too large");
    k_sam_postprocess<<<mve_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(d_low_res, L, S, h_in, w_in, H, W, mask_threshold, d_masks, d_logits, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // extern "C"
