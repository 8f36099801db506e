// LoFTR matcher primitives (include/mvedit_amd.h section 2f): the kernels of the reference's detector-free matcher (loftr/, loaded at
// lib/apis/adapter3d.py:411-415, run per Zero123++ view by lib/core/utils/pose_estimation.py) that the GEMM / conv / norm primitives do not give:
// the operand rows of the single-channel 7 x 7 / 2 stem, LeakyReLU, the sinusoidal position add, linear attention (loftr_module/
// linear_attention.py) as a K^T V reduction and a per-row apply, dual-softmax confidence with mutual-nearest selection (utils/coarse_matching.py),
// the 5 x 5 fine-window gather (loftr_module/fine_preprocess.py) and the fine-window expectation (utils/fine_matching.py).
// Every reduction runs in fp32 in a fixed order -- no float atomics -- so two runs give the same bits.  All of them are bandwidth- or
// launch-bound (head dims 32 / 16, 25-row windows); written to be read, not tuned.
#include "common.h"
#include "scan.h"

namespace {

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool is16(int dtype) { return dtype == MVE_F16 || dtype == MVE_BF16; }

// phi(x) = elu(x) + 1 = x + 1 (x > 0), exp(x) (x <= 0)
__device__ __forceinline__ float la_phi(float x) { return x > 0.f ? x + 1.f : expf(x); }

// ---------------------------------------------------------------------------------------------------
// stem rows: Conv2d(1, C, 7, stride 2, padding 3) of an even-sized single-channel image as a GEMM.
// rows[(b*Ho + oy)*Wo + ox][ky*7 + kx] = pixels[b][0][2*oy - 3 + ky][2*ox - 3 + kx] (0 outside), columns [49, 56) zero.
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_loftr_stem_rows(const typename Tag::T* __restrict__ px, typename Tag::T* __restrict__ rows, int H, int W, long long total) {
    typedef typename Tag::T T;
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Ho = H / 2, Wo = W / 2;
    const long long row = i / 7;
    const int k0 = (int)(i - row * 7) * 8;
    const int b = (int)(row / ((long long)Ho * Wo)), g = (int)(row - (long long)b * Ho * Wo), oy = g / Wo, ox = g - oy * Wo;
    const T* img = px + (size_t)b * H * W;
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        T v = (T)0.f;
        if (k < 49) {
            const int ky = k / 7, kx = k - ky * 7;
            const int y = 2 * oy - 3 + ky, x = 2 * ox - 3 + kx;
            if (y >= 0 && y < H && x >= 0 && x < W) v = img[(size_t)y * W + x];
        }
        o[e] = v;
    }
    reinterpret_cast<V8*>(rows)[i] = o;
}

template <class Tag>
int launch_stem_rows(const void* px, void* rows, int B, int H, int W, hipStream_t s) {
    typedef typename Tag::T T;
    const long long total = (long long)B * (H / 2) * (W / 2) * 7;
    k_loftr_stem_rows<Tag><<<mve_cdiv(total, 256), 256, 0, s>>>((const T*)px, (T*)rows, H, W, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// y = x (x >= 0), slope * x (x < 0): the product in fp32, one rounding
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_loftr_leaky_relu(const typename Tag::V8* __restrict__ x, typename Tag::V8* __restrict__ y, float slope, long long n8) {
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const V8 v = x[i];
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float f = Tag::to_f32(v[e]);
        o[e] = f >= 0.f ? v[e] : Tag::from_f32(f * slope);
    }
    y[i] = o;
}

template <class Tag>
int launch_leaky_relu(const void* x, void* y, size_t n, float slope, hipStream_t s) {
    typedef typename Tag::V8 V8;
    k_loftr_leaky_relu<Tag><<<mve_cdiv(n / 8, 256), 256, 0, s>>>((const V8*)x, (V8*)y, slope, (long long)(n / 8));
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// position add: y[b, p, :] = round_once(float(x[b, p, :]) + pos[p, :]), pos fp32 [HW][C]
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_loftr_pos_add(const typename Tag::V8* __restrict__ x, const float* __restrict__ pos, typename Tag::V8* __restrict__ y, long long per_image8,
                                                       long long total8) {
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total8) return;
    const float* p = pos + (i % per_image8) * 8;
    const V8 v = x[i];
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = Tag::from_f32(Tag::to_f32(v[e]) + p[e]);
    y[i] = o;
}

template <class Tag>
int launch_pos_add(const void* x, const float* pos, void* y, int B, int HW, int C, hipStream_t s) {
    typedef typename Tag::V8 V8;
    const long long per = (long long)HW * C / 8, total = per * B;
    k_loftr_pos_add<Tag><<<mve_cdiv(total, 256), 256, 0, s>>>((const V8*)x, pos, (V8*)y, per, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// linear attention, K^T V: per (batch, head) KV[d][v] = sum_s phi(K[s][d]) V[s][v], Ksum[d] = sum_s phi(K[s][d]).
// Block (bh, split) reduces LA_CHUNK rows of S in 64-row LDS tiles; thread t owns the D*D/256 outputs t, t + 256, ... (row d = idx / D, column
// v = idx % D: a wave reads one or two phi(K) values broadcast and consecutive V values -- conflict free) and sums its rows in ascending order.
// out[(bh * nsplit + split)][D*D + D]: KV row-major, then Ksum.
// ---------------------------------------------------------------------------------------------------
constexpr int LA_CHUNK = 128;
constexpr int LA_TILE = 64;

template <class Tag, int D>
__global__ __launch_bounds__(256) void k_linattn_kv(const typename Tag::T* __restrict__ K, int ldk, const typename Tag::T* __restrict__ V, int ldv, int S, int H,
                                                    float* __restrict__ out, int nsplit) {
    typedef typename Tag::V8 V8;
    constexpr int D8 = D / 8, NPT = D * D / 256, E = D * D + D;
    __shared__ float sk[LA_TILE][D];
    __shared__ float sv[LA_TILE][D];
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H, split = blockIdx.y, tid = threadIdx.x;
    const int s0 = split * LA_CHUNK, s1 = min(S, s0 + LA_CHUNK);
    float acc[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) acc[j] = 0.f;
    float ks = 0.f;
    for (int t0 = s0; t0 < s1; t0 += LA_TILE) {
        const int rows = min(LA_TILE, s1 - t0);
        for (int i = tid; i < rows * D8; i += 256) {
            const int r = i / D8, c8 = i - r * D8;
            const size_t row = (size_t)b * S + t0 + r;
            const V8 kv = *reinterpret_cast<const V8*>(K + row * ldk + h * D + c8 * 8);
            const V8 vv = *reinterpret_cast<const V8*>(V + row * ldv + h * D + c8 * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                sk[r][c8 * 8 + e] = la_phi(Tag::to_f32(kv[e]));
                sv[r][c8 * 8 + e] = Tag::to_f32(vv[e]);
            }
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const int idx = tid + 256 * j;
                acc[j] += sk[r][idx / D] * sv[r][idx % D];
            }
            if (tid < D) ks += sk[r][tid];
        }
        __syncthreads();
    }
    float* o = out + ((size_t)bh * nsplit + split) * E;
#pragma unroll
    for (int j = 0; j < NPT; ++j) o[tid + 256 * j] = acc[j];
    if (tid < D) o[D * D + tid] = ks;
}

// the partial sums of one (batch, head) in ascending split order
__global__ __launch_bounds__(256) void k_linattn_kv_reduce(const float* __restrict__ part, float* __restrict__ out, int nsplit, int E, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long bh = i / E;
    const int e = (int)(i - bh * E);
    float a = 0.f;
    for (int k = 0; k < nsplit; ++k) a += part[((size_t)bh * nsplit + k) * E + e];
    out[i] = a;
}

template <class Tag>
int launch_linattn_kv(const void* K, int ldk, const void* V, int ldv, int B, int S, int H, int D, float* kv, float* ws, hipStream_t s) {
    typedef typename Tag::T T;
    const int nsplit = (S + LA_CHUNK - 1) / LA_CHUNK, E = D * D + D;
    float* dst = nsplit == 1 ? kv : ws;
    const dim3 grid((unsigned)(B * H), (unsigned)nsplit);
    if (D == 32) k_linattn_kv<Tag, 32><<<grid, 256, 0, s>>>((const T*)K, ldk, (const T*)V, ldv, S, H, dst, nsplit);
    else k_linattn_kv<Tag, 16><<<grid, 256, 0, s>>>((const T*)K, ldk, (const T*)V, ldv, S, H, dst, nsplit);
    MVE_LAUNCH_CHECK();
    if (nsplit > 1) {
        const long long total = (long long)B * H * E;
        k_linattn_kv_reduce<<<mve_cdiv(total, 256), 256, 0, s>>>(ws, kv, nsplit, E, total);
        MVE_LAUNCH_CHECK();
    }
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// linear attention, apply: out[l][v] = sum_d phi(Q[l][d]) KV[d][v] / (sum_d phi(Q[l][d]) Ksum[d] + eps), rounded once.
// One thread per 8 output columns of one row; KV + Ksum of the (batch, head) sit in LDS.
// ---------------------------------------------------------------------------------------------------
template <class Tag, int D>
__global__ __launch_bounds__(256) void k_linattn_apply(const typename Tag::T* __restrict__ Q, int ldq, const float* __restrict__ kv, typename Tag::T* __restrict__ out, int ldo,
                                                       int L, int H, float eps) {
    typedef typename Tag::V8 V8;
    constexpr int D8 = D / 8, RPB = 256 / D8, E = D * D + D;
    __shared__ float skv[E];
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H, tid = threadIdx.x;
    for (int i = tid; i < E; i += 256) skv[i] = kv[(size_t)bh * E + i];
    __syncthreads();
    const int l = blockIdx.y * RPB + tid / D8, v0 = (tid % D8) * 8;
    if (l >= L) return;
    const size_t row = (size_t)b * L + l;
    float fq[D];
#pragma unroll
    for (int c8 = 0; c8 < D8; ++c8) {
        const V8 q = *reinterpret_cast<const V8*>(Q + row * ldq + h * D + c8 * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) fq[c8 * 8 + e] = la_phi(Tag::to_f32(q[e]));
    }
    float den = 0.f, o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        den += fq[d] * skv[D * D + d];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += fq[d] * skv[d * D + v0 + e];
    }
    den += eps;
    V8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = Tag::from_f32(o[e] / den);
    *reinterpret_cast<V8*>(out + row * ldo + h * D + v0) = r;
}

template <class Tag>
int launch_linattn_apply(const void* Q, int ldq, const float* kv, void* out, int ldo, int B, int L, int H, int D, float eps, hipStream_t s) {
    typedef typename Tag::T T;
    const int rpb = 256 / (D / 8);
    const dim3 grid((unsigned)(B * H), (unsigned)((L + rpb - 1) / rpb));
    if (D == 32) k_linattn_apply<Tag, 32><<<grid, 256, 0, s>>>((const T*)Q, ldq, kv, (T*)out, ldo, L, H, eps);
    else k_linattn_apply<Tag, 16><<<grid, 256, 0, s>>>((const T*)Q, ldq, kv, (T*)out, ldo, L, H, eps);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// dual softmax.  sim fp32 [N][L][ld], only columns [0, S) are ever read.
// row statistics (softmax over S): one wave per row -- max, then sum exp(x - max); lanes combine by xor butterflies (a fixed order).
// column statistics (softmax over L): a block is 32 columns x 8 row groups (group g takes rows g, g + 8, ...); the 8 partial maxima, then the 8
// partial sums against the common maximum, are combined through LDS in group order.
// stat[..][2] = (max, sum exp).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void k_dsmax_row_stats(const float* __restrict__ sim, long long rows, int S, int ld, float* __restrict__ stat) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;      // wave-uniform
    const int lane = threadIdx.x & 63;
    const float* x = sim + (size_t)row * ld;
    float m = -INFINITY;
    for (int j = lane; j < S; j += 64) m = fmaxf(m, x[j]);
    m = wave_max(m);
    float a = 0.f;
    for (int j = lane; j < S; j += 64) a += expf(x[j] - m);
    a = wave_sum(a);
    if (lane == 0) { stat[2 * row] = m; stat[2 * row + 1] = a; }
}

// SUM = true: (max, sum exp) per column; SUM = false: the maximum alone (stat[n*S + j])
template <bool SUM>
__global__ __launch_bounds__(256) void k_dsmax_col_stats(const float* __restrict__ x, int L, int S, int ld, float* __restrict__ stat) {
    __shared__ float red[8][32];
    const int n = blockIdx.y, c = threadIdx.x & 31, g = threadIdx.x >> 5, j = blockIdx.x * 32 + c;
    const bool ok = j < S;
    const float* col = x + (size_t)n * L * ld + (ok ? j : 0);
    float m = -INFINITY;
    if (ok)
        for (int i = g; i < L; i += 8) m = fmaxf(m, col[(size_t)i * ld]);
    red[g][c] = m;
    __syncthreads();
    m = red[0][c];
#pragma unroll
    for (int k = 1; k < 8; ++k) m = fmaxf(m, red[k][c]);
    if (!SUM) {
        if (ok && g == 0) stat[(size_t)n * S + j] = m;
        return;
    }
    __syncthreads();
    float a = 0.f;
    if (ok)
        for (int i = g; i < L; i += 8) a += expf(col[(size_t)i * ld] - m);
    red[g][c] = a;
    __syncthreads();
    if (ok && g == 0) {
        a = red[0][c];
#pragma unroll
        for (int k = 1; k < 8; ++k) a += red[k][c];
        stat[2 * ((size_t)n * S + j)] = m;
        stat[2 * ((size_t)n * S + j) + 1] = a;
    }
}

// conf[n][i][j] = exp(x - rowmax) / rowsum * exp(x - colmax) / colsum, fp32, compact [N][L][S]
__global__ __launch_bounds__(256) void k_dsmax_conf(const float* __restrict__ sim, int L, int S, int ld, const float* __restrict__ rstat, const float* __restrict__ cstat,
                                                    float* __restrict__ conf, long long total) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long row = e / S;      // n * L + i
    const int j = (int)(e - row * S);
    const long long n = row / L;
    const float x = sim[(size_t)row * ld + j];
    const float rm = rstat[2 * row], rs = rstat[2 * row + 1];
    const float cm = cstat[2 * (n * S + j)], cs = cstat[2 * (n * S + j) + 1];
    conf[e] = (expf(x - cm) / cs) * (expf(x - rm) / rs);
}

// ---------------------------------------------------------------------------------------------------
// mutual-nearest selection (get_coarse_match): row i of pair n matches column j when conf > thr, neither cell lies within `border` cells of its
// grid's edge, and conf equals both its row's and its column's maximum; among several such j (exactly equal floats) the lowest.
// One wave per row: the row maximum, then every lane's lowest passing j, then the minimum over lanes.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dsmax_select_rows(const float* __restrict__ conf, const float* __restrict__ colmax, long long rows, int L, int S, int W0, int H1, int W1,
                                                           int H0, float thr, int border, int* __restrict__ flag, int* __restrict__ jbest) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;      // wave-uniform
    const int lane = threadIdx.x & 63;
    const long long n = row / L;
    const int i = (int)(row - n * L), y0 = i / W0, x0 = i - y0 * W0;
    const float* x = conf + (size_t)row * S;
    const float* cm = colmax + (size_t)n * S;
    float m = -INFINITY;
    for (int j = lane; j < S; j += 64) m = fmaxf(m, x[j]);
    m = wave_max(m);
    int best = 0x7fffffff;
    const bool row_in = border <= 0 || (y0 >= border && y0 < H0 - border && x0 >= border && x0 < W0 - border);
    if (row_in && m > thr) {
        for (int j = lane; j < S; j += 64) {
            const float v = x[j];
            if (v != m || v != cm[j]) continue;
            const int y1 = j / W1, x1 = j - y1 * W1;
            if (border > 0 && !(y1 >= border && y1 < H1 - border && x1 >= border && x1 < W1 - border)) continue;
            best = j;
            break;
        }
    }
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    if (lane == 0) { flag[row] = best != 0x7fffffff; jbest[row] = best; }
}

__global__ __launch_bounds__(256) void k_dsmax_compact(const float* __restrict__ conf, const int* __restrict__ flag, const int* __restrict__ jbest, const int* __restrict__ offs,
                                                       long long rows, int L, int S, int W0, int W1, float scale, long long* __restrict__ b_ids, long long* __restrict__ i_ids,
                                                       long long* __restrict__ j_ids, float* __restrict__ mconf, float* __restrict__ mk0, float* __restrict__ mk1) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows || !flag[row]) return;
    const int o = offs[row], j = jbest[row];      // o < rows: at most one match per row
    const long long n = row / L;
    const int i = (int)(row - n * L);
    b_ids[o] = n; i_ids[o] = i; j_ids[o] = j;
    mconf[o] = conf[(size_t)row * S + j];
    if (mk0) { mk0[2 * o] = (float)(i % W0) * scale; mk0[2 * o + 1] = (float)(i / W0) * scale; }
    if (mk1) { mk1[2 * o] = (float)(j % W1) * scale; mk1[2 * o + 1] = (float)(j / W1) * scale; }
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------------
// fine windows: F.unfold(feat, 5, stride 4, padding 2) at the matched coarse cells only.
// rows[(m*25 + ky*5 + kx)][:] = feat[b_ids[m]][4*cy - 2 + ky][4*cx - 2 + kx][:] (zero outside the map, and for an id outside its range),
// (cy, cx) = (id / Wc, id % Wc), Wc = Wf / 4.  feat NHWC.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_loftr_unfold(const u32x4* __restrict__ feat, int N, int Hf, int Wf, int C8, const long long* __restrict__ b_ids,
                                                      const long long* __restrict__ ids, u32x4* __restrict__ rows, long long total) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long r = t / C8;      // m * 25 + ww
    const int c8 = (int)(t - r * C8);
    const long long m = r / 25;
    const int ww = (int)(r - m * 25), ky = ww / 5, kx = ww - ky * 5;
    const int Hc = Hf / 4, Wc = Wf / 4;
    const long long b = b_ids[m], id = ids[m];
    u32x4 v = {0u, 0u, 0u, 0u};
    if (b >= 0 && b < N && id >= 0 && id < (long long)Hc * Wc) {
        const int cy = (int)id / Wc, cx = (int)id - cy * Wc, y = 4 * cy - 2 + ky, x = 4 * cx - 2 + kx;
        if (y >= 0 && y < Hf && x >= 0 && x < Wf) v = feat[(((size_t)b * Hf + y) * Wf + x) * C8 + c8];
    }
    rows[t] = v;
}

// ---------------------------------------------------------------------------------------------------
// fine matching: one wave per match.  Lane r < 25 takes the dot product of window 0's centre row (12) with row r of window 1 over C in fp32,
// the softmax at 1/sqrt(C) and the moments over the normalised 5 x 5 grid {-1, -1/2, 0, 1/2, 1}^2 (x fastest) are xor butterflies.
// expec[m] = (E[x], E[y], sqrt(max(Var x, 1e-10)) + sqrt(max(Var y, 1e-10))); mk1_f[m] = mk1_c[m] + (E[x], E[y]) * radius.
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_loftr_fine_match(const typename Tag::T* __restrict__ f0, const typename Tag::T* __restrict__ f1, long long M, int C, float temp,
                                                          const float* __restrict__ mk1_c, float radius, float* __restrict__ expec, float* __restrict__ mk1_f) {
    typedef typename Tag::V8 V8;
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;      // wave-uniform
    const int lane = threadIdx.x & 63;
    const bool on = lane < 25;
    // The logits reach ~100, where one fp32 rounding of the dot product already moves exp() by 1e-5: the products of two 16-bit values are
    // exact in fp32 and the sum is compensated (Kahan), so the dot product carries one rounding instead of one per term.
    float dot = 0.f;
    if (on) {
#pragma clang fp contract(off)
        const V8* a = reinterpret_cast<const V8*>(f0 + ((size_t)m * 25 + 12) * C);
        const V8* b = reinterpret_cast<const V8*>(f1 + ((size_t)m * 25 + lane) * C);
        float comp = 0.f;
        for (int c8 = 0; c8 < C / 8; ++c8) {
            const V8 va = a[c8], vb = b[c8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float y = Tag::to_f32(va[e]) * Tag::to_f32(vb[e]) - comp;
                const float t = dot + y;
                comp = (t - dot) - y;
                dot = t;
            }
        }
    }
    const float z = on ? dot * temp : -INFINITY;
    const float mx = wave_max(z);
    const float p = on ? expf(z - mx) : 0.f;
    const float den = wave_sum(p);
    const float gx = on ? (float)(lane % 5) * 0.5f - 1.f : 0.f, gy = on ? (float)(lane / 5) * 0.5f - 1.f : 0.f;
    const float h = p / den;
    const float ex = wave_sum(h * gx), ey = wave_sum(h * gy), exx = wave_sum(h * gx * gx), eyy = wave_sum(h * gy * gy);
    if (lane == 0) {
        const float vx = exx - ex * ex, vy = eyy - ey * ey;
        expec[3 * m] = ex; expec[3 * m + 1] = ey;
        expec[3 * m + 2] = sqrtf(fmaxf(vx, 1e-10f)) + sqrtf(fmaxf(vy, 1e-10f));
        mk1_f[2 * m] = mk1_c[2 * m] + ex * radius;
        mk1_f[2 * m + 1] = mk1_c[2 * m + 1] + ey * radius;
    }
}

// ---------------------------------------------------------------------------------------------------
// y[m, :] = x[m, :] + LayerNorm(o[m, :]) (LoFTREncoderLayer's `x + norm2(message)`): one wave per row, the row in registers (C <= 512), mean and
// biased variance by xor butterflies, everything in fp32, one rounding.  y may alias x.
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_loftr_ln_add(const typename Tag::T* __restrict__ o, int ldo, const typename Tag::T* x, int ldx, typename Tag::T* y, int ldy, long long M,
                                                      int C, const float* __restrict__ gamma, const float* __restrict__ beta, float eps) {
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;      // wave-uniform
    const int lane = threadIdx.x & 63, per = C / 64;
    float v[8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < per) { v[k] = Tag::to_f32(o[(size_t)m * ldo + lane + 64 * k]); s += v[k]; }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < per) { const float d = v[k] - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < per) {
            const int c = lane + 64 * k;
            y[(size_t)m * ldy + c] = Tag::from_f32(Tag::to_f32(x[(size_t)m * ldx + c]) + ((v[k] - mean) * rstd * gamma[c] + beta[c]));
        }
}

template <class Tag>
int launch_ln_add(const void* o, int ldo, const void* x, int ldx, void* y, int ldy, int M, int C, const float* gamma, const float* beta, float eps, hipStream_t s) {
    typedef typename Tag::T T;
    k_loftr_ln_add<Tag><<<mve_cdiv((unsigned long long)M, 4), 256, 0, s>>>((const T*)o, ldo, (const T*)x, ldx, (T*)y, ldy, (long long)M, C, gamma, beta, eps);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// rows[m, :] = feat[b_ids[m]][ids[m]][:] (zero for an id outside its range): the coarse features at the matched cells.  feat [N][L][C].
__global__ __launch_bounds__(256) void k_loftr_gather_rows(const u32x4* __restrict__ feat, int N, int L, int C8, const long long* __restrict__ b_ids,
                                                           const long long* __restrict__ ids, u32x4* __restrict__ rows, long long total) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long m = t / C8;
    const int c8 = (int)(t - m * C8);
    const long long b = b_ids[m], id = ids[m];
    u32x4 v = {0u, 0u, 0u, 0u};
    if (b >= 0 && b < N && id >= 0 && id < L) v = feat[((size_t)b * L + id) * C8 + c8];
    rows[t] = v;
}

template <class Tag>
int launch_fine_match(const void* f0, const void* f1, int M, int C, float temp, const float* mk1_c, float radius, float* expec, float* mk1_f, hipStream_t s) {
    typedef typename Tag::T T;
    k_loftr_fine_match<Tag><<<mve_cdiv((unsigned long long)M, 4), 256, 0, s>>>((const T*)f0, (const T*)f1, (long long)M, C, temp, mk1_c, radius, expec, mk1_f);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int check_linattn(const char* who, int dtype, const void* a, int lda, const void* b, int ldb, int B, int S, int H, int D) {
    MVE_CHECK(is16(dtype), MVE_ERR_ARG, "%s: dtype %d must be f16 or bf16", who, dtype);
    MVE_CHECK(a && b, MVE_ERR_ARG, "%s: null pointer", who);
    MVE_CHECK(D == 32 || D == 16, MVE_ERR_ARG, "%s: head dim %d must be 32 or 16", who, D);
    MVE_CHECK(B >= 1 && S >= 1 && H >= 1, MVE_ERR_ARG, "%s: bad B %d / length %d / heads %d", who, B, S, H);
    MVE_CHECK(lda >= H * D && ldb >= H * D && lda % 8 == 0 && ldb % 8 == 0, MVE_ERR_ARG, "%s: leading dimensions %d / %d must be multiples of 8 and >= heads * D = %d", who, lda, ldb,
              H * D);
    MVE_CHECK(aligned16(a) && aligned16(b), MVE_ERR_ARG, "%s: pointers must be 16-byte aligned", who);
    MVE_CHECK((long long)B * H < (1ll << 31) && (long long)B * S * (long long)(lda > ldb ? lda : ldb) < (1ll << 40), MVE_ERR_ARG, "%s: B %d x heads %d overflows the grid", who, B, H);
    return MVE_OK;
}

int check_sim(const char* who, const void* sim, int N, int L, int S, int ld) {
    MVE_CHECK(sim, MVE_ERR_ARG, "%s: null pointer (d_sim)", who);
    MVE_CHECK(N >= 1 && N <= 65535 && L >= 1 && S >= 1, MVE_ERR_ARG, "%s: bad N %d / L %d / S %d", who, N, L, S);
    MVE_CHECK(ld >= S, MVE_ERR_ARG, "%s: ld %d < S %d", who, ld, S);
    MVE_CHECK((long long)N * L < (1ll << 31) && (long long)N * S < (1ll << 31), MVE_ERR_ARG, "%s: N %d overflows 32-bit row indexing", who, N);
    return MVE_OK;
}

}  // namespace

extern "C" int mve_loftr_stem_rows(int dtype, const void* pixels, int B, int H, int W, void* rows, int ld, void* stream) {
    MVE_CHECK(is16(dtype), MVE_ERR_ARG, "loftr_stem_rows: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(pixels && rows, MVE_ERR_ARG, "loftr_stem_rows: null pointer (d_pixels / d_rows)");
    MVE_CHECK(B >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, MVE_ERR_ARG, "loftr_stem_rows: bad B %d / H %d / W %d (H and W must be even)", B, H, W);
    MVE_CHECK(ld == 56, MVE_ERR_ARG, "loftr_stem_rows: ld %d must be 56 (7 * 7 = 49 rounded up to a multiple of 8)", ld);
    MVE_CHECK((long long)B * H * W < (1ll << 31) && (long long)B * (H / 2) * (W / 2) * ld < (1ll << 31), MVE_ERR_ARG, "loftr_stem_rows: batch B %d overflows 32-bit indexing", B);
    MVE_CHECK(aligned16(rows), MVE_ERR_ARG, "loftr_stem_rows: d_rows must be 16-byte aligned");
    return MVE_DISPATCH_16(dtype, launch_stem_rows, pixels, rows, B, H, W, (hipStream_t)stream);
}

extern "C" int mve_loftr_leaky_relu(int dtype, const void* x, void* y, size_t n, float slope, void* stream) {
    MVE_CHECK(is16(dtype), MVE_ERR_ARG, "loftr_leaky_relu: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(x && y, MVE_ERR_ARG, "loftr_leaky_relu: null pointer (d_x / d_y)");
    MVE_CHECK(n >= 8 && n % 8 == 0, MVE_ERR_ARG, "loftr_leaky_relu: n %zu must be a multiple of 8", n);
    MVE_CHECK(aligned16(x) && aligned16(y), MVE_ERR_ARG, "loftr_leaky_relu: d_x / d_y must be 16-byte aligned");
    return MVE_DISPATCH_16(dtype, launch_leaky_relu, x, y, n, slope, (hipStream_t)stream);
}

extern "C" int mve_loftr_pos_add(int dtype, const void* x, const float* pos, void* y, int B, int HW, int C, void* stream) {
    MVE_CHECK(is16(dtype), MVE_ERR_ARG, "loftr_pos_add: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(x && pos && y, MVE_ERR_ARG, "loftr_pos_add: null pointer (d_x / d_pos / d_y)");
    MVE_CHECK(B >= 1 && HW >= 1 && C >= 8 && C % 8 == 0, MVE_ERR_ARG, "loftr_pos_add: bad B %d / HW %d / C %d (C must be a multiple of 8)", B, HW, C);
    MVE_CHECK((long long)B * HW * C < (1ll << 31), MVE_ERR_ARG, "loftr_pos_add: batch B %d overflows 32-bit indexing", B);
    MVE_CHECK(aligned16(x) && aligned16(y) && aligned16(pos), MVE_ERR_ARG, "loftr_pos_add: pointers must be 16-byte aligned");
    return MVE_DISPATCH_16(dtype, launch_pos_add, x, pos, y, B, HW, C, (hipStream_t)stream);
}

extern "C" size_t mve_linattn_workspace_bytes(int B, int S, int H, int D) {
    if (B < 1 || S < 1 || H < 1 || D < 1) return 0;
    const size_t nsplit = ((size_t)S + LA_CHUNK - 1) / LA_CHUNK;
    return nsplit > 1 ? (size_t)B * H * nsplit * ((size_t)D * D + D) * sizeof(float) : 0;
}

extern "C" int mve_linattn_kv(int dtype, const void* k, int ldk, const void* v, int ldv, int B, int S, int H, int D, float* kv, void* workspace, size_t workspace_bytes,
                              void* stream) {
    const int rc = check_linattn("linattn_kv", dtype, k, ldk, v, ldv, B, S, H, D);
    if (rc) return rc;
    MVE_CHECK(kv, MVE_ERR_ARG, "linattn_kv: null pointer (d_kv)");
    const size_t need = mve_linattn_workspace_bytes(B, S, H, D);
    MVE_CHECK((S + LA_CHUNK - 1) / LA_CHUNK <= 65535, MVE_ERR_ARG, "linattn_kv: S %d is too long", S);
    MVE_CHECK(need == 0 || (workspace && workspace_bytes >= need), MVE_ERR_ARG, "linattn_kv: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return MVE_DISPATCH_16(dtype, launch_linattn_kv, k, ldk, v, ldv, B, S, H, D, kv, (float*)workspace, (hipStream_t)stream);
}

extern "C" int mve_linattn_apply(int dtype, const void* q, int ldq, const float* kv, void* out, int ldo, int B, int L, int H, int D, float eps, void* stream) {
    const int rc = check_linattn("linattn_apply", dtype, q, ldq, out, ldo, B, L, H, D);
    if (rc) return rc;
    MVE_CHECK(kv, MVE_ERR_ARG, "linattn_apply: null pointer (d_kv)");
    MVE_CHECK((L + 63) / 64 <= 65535, MVE_ERR_ARG, "linattn_apply: L %d is too long", L);
    return MVE_DISPATCH_16(dtype, launch_linattn_apply, q, ldq, kv, out, ldo, B, L, H, D, eps, (hipStream_t)stream);
}

extern "C" int mve_dsmax_stats(const float* sim, int N, int L, int S, int ld, float* row_stats, float* col_stats, void* stream) {
    const int rc = check_sim("dsmax_stats", sim, N, L, S, ld);
    if (rc) return rc;
    MVE_CHECK(row_stats && col_stats, MVE_ERR_ARG, "dsmax_stats: null pointer (d_row_stats / d_col_stats)");
    const hipStream_t s = (hipStream_t)stream;
    const long long rows = (long long)N * L;
    k_dsmax_row_stats<<<mve_cdiv(rows, 4), 256, 0, s>>>(sim, rows, S, ld, row_stats);
    MVE_LAUNCH_CHECK();
    k_dsmax_col_stats<true><<<dim3(mve_cdiv(S, 32), (unsigned)N), 256, 0, s>>>(sim, L, S, ld, col_stats);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

extern "C" int mve_dsmax_conf(const float* sim, int N, int L, int S, int ld, const float* row_stats, const float* col_stats, float* conf, void* stream) {
    const int rc = check_sim("dsmax_conf", sim, N, L, S, ld);
    if (rc) return rc;
    MVE_CHECK(row_stats && col_stats && conf, MVE_ERR_ARG, "dsmax_conf: null pointer (d_row_stats / d_col_stats / d_conf)");
    const long long total = (long long)N * L * S;
    MVE_CHECK(total < (1ll << 39), MVE_ERR_ARG, "dsmax_conf: N %d x L %d x S %d is too large", N, L, S);
    k_dsmax_conf<<<mve_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(sim, L, S, ld, row_stats, col_stats, conf, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

extern "C" size_t mve_dsmax_select_workspace_bytes(int N, int L, int S) {
    if (N < 1 || L < 1 || S < 1) return 0;
    const size_t rows = (size_t)N * L, ntiles = (rows + SCAN_TILE - 1) / SCAN_TILE;
    return up256((size_t)N * S * 4) + 3 * up256(rows * 4) + up256(ntiles * 4);
}

extern "C" int mve_dsmax_select(const float* conf, int N, int H0, int W0, int H1, int W1, float thr, int border, float scale, int64_t* b_ids, int64_t* i_ids, int64_t* j_ids,
                                float* mconf, float* mkpts0_c, float* mkpts1_c, int* count, void* workspace, size_t workspace_bytes, void* stream) {
    MVE_CHECK(H0 >= 1 && W0 >= 1 && H1 >= 1 && W1 >= 1 && (long long)H0 * W0 < (1ll << 31) && (long long)H1 * W1 < (1ll << 31), MVE_ERR_ARG,
              "dsmax_select: bad grids %d x %d / %d x %d", H0, W0, H1, W1);
    const int L = H0 * W0, S = H1 * W1;
    const int rc = check_sim("dsmax_select", conf, N, L, S, S);
    if (rc) return rc;
    MVE_CHECK(b_ids && i_ids && j_ids && mconf && count, MVE_ERR_ARG, "dsmax_select: null pointer (d_b_ids / d_i_ids / d_j_ids / d_mconf / d_count)");
    const size_t need = mve_dsmax_select_workspace_bytes(N, L, S);
    MVE_CHECK(workspace && workspace_bytes >= need && aligned16(workspace), MVE_ERR_ARG, "dsmax_select: workspace of %zu bytes, %zu needed (16-byte aligned)", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const long long rows = (long long)N * L;
    char* w = (char*)workspace;
    float* colmax = (float*)w; w += up256((size_t)N * S * 4);
    int* flag = (int*)w; w += up256((size_t)rows * 4);
    int* jbest = (int*)w; w += up256((size_t)rows * 4);
    int* offs = (int*)w; w += up256((size_t)rows * 4);
    int* tile_sums = (int*)w;
    k_dsmax_col_stats<false><<<dim3(mve_cdiv(S, 32), (unsigned)N), 256, 0, s>>>(conf, L, S, S, colmax);
    MVE_LAUNCH_CHECK();
    k_dsmax_select_rows<<<mve_cdiv(rows, 4), 256, 0, s>>>(conf, colmax, rows, L, S, W0, H1, W1, H0, thr, border, flag, jbest);
    MVE_LAUNCH_CHECK();
    const int rs = exclusive_scan<int>(flag, offs, (size_t)rows, tile_sums, count, s);
    MVE_CHECK(rs == MVE_OK, MVE_ERR_HIP, "dsmax_select: scan launch failed");
    k_dsmax_compact<<<mve_cdiv(rows, 256), 256, 0, s>>>(conf, flag, jbest, offs, rows, L, S, W0, W1, scale, (long long*)b_ids, (long long*)i_ids, (long long*)j_ids, mconf, mkpts0_c,
                                                        mkpts1_c);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

extern "C" int mve_loftr_unfold(int dtype, const void* feat, int N, int Hf, int Wf, int C, const int64_t* b_ids, const int64_t* ids, int M, void* rows, void* stream) {
    MVE_CHECK(is16(dtype), MVE_ERR_ARG, "loftr_unfold: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(feat && b_ids && ids && rows, MVE_ERR_ARG, "loftr_unfold: null pointer (d_feat / d_b_ids / d_ids / d_rows)");
    MVE_CHECK(N >= 1 && Hf >= 4 && Wf >= 4 && Hf % 4 == 0 && Wf % 4 == 0, MVE_ERR_ARG, "loftr_unfold: bad N %d / Hf %d / Wf %d (the fine map is 4 x the coarse grid)", N, Hf, Wf);
    MVE_CHECK(C >= 8 && C % 8 == 0, MVE_ERR_ARG, "loftr_unfold: C %d must be a multiple of 8", C);
    MVE_CHECK(M >= 1, MVE_ERR_ARG, "loftr_unfold: M %d must be at least 1 (no launch for an empty match set)", M);
    MVE_CHECK((long long)N * Hf * Wf * C < (1ll << 31) && (long long)M * 25 * C < (1ll << 31), MVE_ERR_ARG, "loftr_unfold: N %d / M %d overflows 32-bit indexing", N, M);
    MVE_CHECK(aligned16(feat) && aligned16(rows), MVE_ERR_ARG, "loftr_unfold: d_feat / d_rows must be 16-byte aligned");
    const long long total = (long long)M * 25 * (C / 8);
    k_loftr_unfold<<<mve_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>((const u32x4*)feat, N, Hf, Wf, C / 8, (const long long*)b_ids, (const long long*)ids, (u32x4*)rows, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

extern "C" int mve_loftr_ln_add(int dtype, const void* o, int ldo, const void* x, int ldx, void* y, int ldy, int M, int C, const float* gamma, const float* beta, float eps,
                                void* stream) {
    MVE_CHECK(is16(dtype), MVE_ERR_ARG, "loftr_ln_add: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(o && x && y && gamma && beta, MVE_ERR_ARG, "loftr_ln_add: null pointer");
    MVE_CHECK(M >= 1 && C >= 64 && C <= 512 && C % 64 == 0, MVE_ERR_ARG, "loftr_ln_add: bad M %d / C %d (C must be a multiple of 64, at most 512)", M, C);
    MVE_CHECK(ldo >= C && ldx >= C && ldy >= C, MVE_ERR_ARG, "loftr_ln_add: leading dimensions %d / %d / %d must be at least C %d", ldo, ldx, ldy, C);
    MVE_CHECK((long long)M * (long long)(ldo > ldx ? (ldo > ldy ? ldo : ldy) : (ldx > ldy ? ldx : ldy)) < (1ll << 40), MVE_ERR_ARG, "loftr_ln_add: M %d is too large", M);
    return MVE_DISPATCH_16(dtype, launch_ln_add, o, ldo, x, ldx, y, ldy, M, C, gamma, beta, eps, (hipStream_t)stream);
}

extern "C" int mve_loftr_gather_rows(int dtype, const void* feat, int N, int L, int C, const int64_t* b_ids, const int64_t* ids, int M, void* rows, void* stream) {
    MVE_CHECK(is16(dtype), MVE_ERR_ARG, "loftr_gather_rows: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(feat && b_ids && ids && rows, MVE_ERR_ARG, "loftr_gather_rows: null pointer (d_feat / d_b_ids / d_ids / d_rows)");
    MVE_CHECK(N >= 1 && L >= 1 && M >= 1 && C >= 8 && C % 8 == 0, MVE_ERR_ARG, "loftr_gather_rows: bad N %d / L %d / M %d / C %d", N, L, M, C);
    MVE_CHECK((long long)N * L * C < (1ll << 31) && (long long)M * C < (1ll << 31), MVE_ERR_ARG, "loftr_gather_rows: N %d / M %d overflows 32-bit indexing", N, M);
    MVE_CHECK(aligned16(feat) && aligned16(rows), MVE_ERR_ARG, "loftr_gather_rows: d_feat / d_rows must be 16-byte aligned");
    const long long total = (long long)M * (C / 8);
    k_loftr_gather_rows<<<mve_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>((const u32x4*)feat, N, L, C / 8, (const long long*)b_ids, (const long long*)ids, (u32x4*)rows, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

extern "C" int mve_loftr_fine_match(int dtype, const void* feat0, const void* feat1, int M, int C, const float* mkpts1_c, float radius, float* expec_f, float* mkpts1_f,
                                    void* stream) {
    MVE_CHECK(is16(dtype), MVE_ERR_ARG, "loftr_fine_match: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(feat0 && feat1 && mkpts1_c && expec_f && mkpts1_f, MVE_ERR_ARG, "loftr_fine_match: null pointer");
    MVE_CHECK(M >= 1, MVE_ERR_ARG, "loftr_fine_match: M %d must be at least 1 (no launch for an empty match set)", M);
    MVE_CHECK(C >= 8 && C % 8 == 0 && (long long)M * 25 * C < (1ll << 31), MVE_ERR_ARG, "loftr_fine_match: C %d must be a multiple of 8 and M * 25 * C < 2^31", C);
    MVE_CHECK(aligned16(feat0) && aligned16(feat1), MVE_ERR_ARG, "loftr_fine_match: d_feat0 / d_feat1 must be 16-byte aligned");
    return MVE_DISPATCH_16(dtype, launch_fine_match, feat0, feat1, M, C, 1.0f / sqrtf((float)C), mkpts1_c, radius, expec_f, mkpts1_f, (hipStream_t)stream);
}
