// Occupancy-grid ray marching + alpha compositing for gfx950.
//
// Behavioural contract: lib/ops/raymarching/src/raymarching.cu of the reference
// (kernel line ranges cited per entry in include/mvedit_amd.h).  This file is a
// re-design, not a translation:
//   * one DDA core (GridWalker) shared by the training and inference marchers,
//     parameterised by a sample sink;
//   * the reference's "count pass -> atomicAdd -> host .item() -> write pass"
//     becomes count -> device prefix sum (ray order, deterministic) -> write,
//     all stream ordered;
//   * alive-list compaction is a device scan instead of a boolean-mask gather.
//
// Arithmetic is kept op-for-op identical to the reference source semantics
// (including the double-precision intermediates its literals imply), and this
// file is compiled with -ffp-contract=off so that index buffers (ray offsets,
// counts, Morton codes, bitfields) and marched positions are bit-exact against
// oracle/raymarching_oracle.c.
#include "raymarch_core.h"

#include "capacity_core.h"

namespace {

constexpr int kBlock = 256;              // 4 waves

// ---------------------------------------------------------------------------
// wave / block exclusive scan of one int per thread (kBlock threads)
// ---------------------------------------------------------------------------
__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// returns exclusive prefix of v within the block; *block_total gets the sum (valid in all threads)
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* block_total, int* lds /* NT/64 + 1 ints */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    constexpr int NW = NT / 64;
    int incl = wave_incl_scan(v);
    if (lane == 63) lds[wid] = incl;
    __syncthreads();
    if (wid == 0) {
        int w = (lane < NW) ? lds[lane] : 0;
        int wi = wave_incl_scan(w);
        if (lane < NW) lds[lane] = wi - w;   // exclusive wave bases
        if (lane == NW - 1) lds[NW] = wi;    // block total
    }
    __syncthreads();
    const int base = lds[wid];
    *block_total = lds[NW];
    __syncthreads();
    return base + incl - v;
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_near_far(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                     const float* __restrict__ aabb, uint32_t N, float min_near,
                                                     float* __restrict__ nears, float* __restrict__ fars) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const float3p o = reinterpret_cast<const float3p*>(rays_o)[n];
    const float3p d = reinterpret_cast<const float3p*>(rays_d)[n];
    const float lo[3] = {aabb[0], aabb[1], aabb[2]}, hi[3] = {aabb[3], aabb[4], aabb[5]};
    const float oo[3] = {o.x, o.y, o.z};
    const float rd[3] = {1 / d.x, 1 / d.y, 1 / d.z};

    // slab test, axis by axis, with the reference's early-out ordering (x,y then z)
    float near = (lo[0] - oo[0]) * rd[0], far = (hi[0] - oo[0]) * rd[0];
    if (near > far) { float s = near; near = far; far = s; }
    bool miss = false;
#pragma unroll
    for (int a = 1; a < 3; ++a) {
        float na = (lo[a] - oo[a]) * rd[a], fa = (hi[a] - oo[a]) * rd[a];
        if (na > fa) { float s = na; na = fa; fa = s; }
        if (!miss) {
            if (near > fa || na > far) {
                miss = true;
            } else {
                if (na > near) near = na;
                if (fa < far) far = fa;
            }
        }
    }
    if (miss) {
        near = far = FLT_MAX;
    } else if (near < min_near) {
        near = min_near;
    }
    nears[n] = near;
    fars[n] = far;
}

__global__ __launch_bounds__(kBlock) void k_morton(const int32_t* __restrict__ coords, uint32_t N, int32_t* __restrict__ idx) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const int32_t* c = coords + 3ull * n;
    idx[n] = (int32_t)morton_encode((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2]);
}

__global__ __launch_bounds__(kBlock) void k_morton_inv(const int32_t* __restrict__ idx, uint32_t N, int32_t* __restrict__ coords) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const int32_t v = idx[n];   // arithmetic shifts on the signed code, as in the reference
    int32_t* c = coords + 3ull * n;
    c[0] = (int32_t)gather3((uint32_t)(v >> 0));
    c[1] = (int32_t)gather3((uint32_t)(v >> 1));
    c[2] = (int32_t)gather3((uint32_t)(v >> 2));
}

// One thread packs 4 output bytes from 32 floats: 8 x 16-byte loads, one dword store.
__global__ __launch_bounds__(kBlock) void k_packbits(const float* __restrict__ grid, uint32_t n_bytes, float thresh,
                                                     uint8_t* __restrict__ bits) {
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;   // output dword index
    const uint32_t b0 = w * 4u;
    if (b0 >= n_bytes) return;
    if (b0 + 4u <= n_bytes && ((reinterpret_cast<uintptr_t>(bits) & 3u) == 0) &&
        ((reinterpret_cast<uintptr_t>(grid) & 15u) == 0)) {
        const f32x4* g = reinterpret_cast<const f32x4*>(grid) + 8ull * w;
        uint32_t out = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f32x4 v = g[q];
#pragma unroll
            for (int i = 0; i < 4; ++i) out |= (v[i] >= thresh ? 1u : 0u) << (q * 4 + i);
        }
        reinterpret_cast<uint32_t*>(bits)[w] = out;
    } else {
        for (uint32_t b = b0; b < n_bytes && b < b0 + 4u; ++b) {
            uint32_t o = 0;
            for (int i = 0; i < 8; ++i) o |= (grid[8ull * b + i] >= thresh ? 1u : 0u) << i;
            bits[b] = (uint8_t)o;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_flatten_rays(const int32_t* __restrict__ rays, uint32_t N, uint32_t M,
                                                         int32_t* __restrict__ res) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const uint32_t off = (uint32_t)rays[2ull * n], cnt = (uint32_t)rays[2ull * n + 1];
    for (uint32_t i = 0; i < cnt && off + i < M; ++i) res[off + i] = (int32_t)n;
}

// pass 1 of the training march: per-ray sample count + per-block sums
__global__ __launch_bounds__(kBlock) void k_march_count(MarchParams p, const float* __restrict__ rays_o,
                                                        const float* __restrict__ rays_d, uint32_t N,
                                                        const float* __restrict__ nears, const float* __restrict__ fars,
                                                        const float* __restrict__ noises, int32_t* __restrict__ rays,
                                                        int32_t* __restrict__ block_sums) {
    __shared__ int lds[kBlock / 64 + 1];
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    int cnt = 0;
    if (n < N) {
        GridWalker w;
        w.init(p, rays_o + 3ull * n, rays_d + 3ull * n);
        float t = nears[n];
        t += w.step_len(t) * noises[n];
        cnt = (int)w.walk(t, fars[n], p.max_steps, [](float, float, float, float, float) { return true; });
        rays[2ull * n + 1] = cnt;
    }
    int total;
    (void)block_excl_scan<kBlock>(cnt, &total, lds);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// single-block exclusive scan over the block sums (in place) + grand total
__global__ __launch_bounds__(1024) void k_scan_block_sums(int32_t* __restrict__ block_sums, uint32_t nblk,
                                                          int32_t* __restrict__ total_out) {
    __shared__ int lds[1024 / 64 + 1];
    int carry = 0;
    for (uint32_t base = 0; base < nblk; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const int v = (i < nblk) ? block_sums[i] : 0;
        int tot;
        const int ex = block_excl_scan<1024>(v, &tot, lds);
        if (i < nblk) block_sums[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) total_out[0] = carry;
}

// per-block local scan + block base -> rays[n].offset
__global__ __launch_bounds__(kBlock) void k_ray_offsets(int32_t* __restrict__ rays, uint32_t N,
                                                        const int32_t* __restrict__ block_bases) {
    __shared__ int lds[kBlock / 64 + 1];
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    const int cnt = (n < N) ? rays[2ull * n + 1] : 0;
    int tot;
    const int ex = block_excl_scan<kBlock>(cnt, &tot, lds);
    if (n < N) rays[2ull * n] = block_bases[blockIdx.x] + ex;
}

// pass 2 of the training march
__global__ __launch_bounds__(kBlock) void k_march_write(MarchParams p, const float* __restrict__ rays_o,
                                                        const float* __restrict__ rays_d, uint32_t N,
                                                        const float* __restrict__ nears, const float* __restrict__ fars,
                                                        const float* __restrict__ noises, const int32_t* __restrict__ rays,
                                                        uint32_t capacity, float* __restrict__ xyzs,
                                                        float* __restrict__ dirs, float* __restrict__ ts) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const uint32_t off = (uint32_t)rays[2ull * n], cnt = (uint32_t)rays[2ull * n + 1];
    if (cnt == 0 || (unsigned long long)off + cnt > capacity) return;
    GridWalker w;
    w.init(p, rays_o + 3ull * n, rays_d + 3ull * n);
    float t = nears[n];
    t += w.step_len(t) * noises[n];
    float3p* px = reinterpret_cast<float3p*>(xyzs) + off;
    float3p* pd = reinterpret_cast<float3p*>(dirs) + off;
    float2p* pt = reinterpret_cast<float2p*>(ts) + off;
    const float3p dir = {w.dx, w.dy, w.dz};
    w.walk(t, fars[n], cnt, [&](float cx, float cy, float cz, float tn, float dt) {
        *px++ = float3p{cx, cy, cz};
        *pd++ = dir;
        *pt++ = float2p{tn, dt};
        return true;
    });
}

// inference march: at most n_step samples per alive ray, fixed stride output
__global__ __launch_bounds__(kBlock) void k_march_infer(MarchParams p, uint32_t n_alive, uint32_t n_step,
                                                        const int32_t* __restrict__ rays_alive,
                                                        const float* __restrict__ rays_t, const float* __restrict__ rays_o,
                                                        const float* __restrict__ rays_d, const float* __restrict__ nears,
                                                        const float* __restrict__ fars, float* __restrict__ xyzs,
                                                        float* __restrict__ dirs, float* __restrict__ ts,
                                                        const float* __restrict__ noises) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= n_alive) return;
    const int ray = rays_alive[n];
    GridWalker w;
    w.init(p, rays_o + 3ll * ray, rays_d + 3ll * ray);
    float t = rays_t[ray];
    t += w.step_len(t) * noises[n];
    const unsigned long long base = (unsigned long long)n * n_step;
    float3p* px = reinterpret_cast<float3p*>(xyzs) + base;
    float3p* pd = reinterpret_cast<float3p*>(dirs) + base;
    float2p* pt = reinterpret_cast<float2p*>(ts) + base;
    const float3p dir = {w.dx, w.dy, w.dz};
    w.walk(t, fars[ray], n_step, [&](float cx, float cy, float cz, float tn, float dt) {
        *px++ = float3p{cx, cy, cz};
        *pd++ = dir;
        *pt++ = float2p{tn, dt};
        return true;
    });
}

// ---------------------------------------------------------------------------
// compositing
// ---------------------------------------------------------------------------
__device__ __forceinline__ float alpha_of(float sigma, float dt, int binarize) {
    const float a = 1.0f - __expf(-sigma * dt);
    return binarize ? (a > 0.5f ? 1.0f : 0.0f) : a;
}

__global__ __launch_bounds__(kBlock) void k_composite_train_fwd(const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                                                const float* __restrict__ ts, const int32_t* __restrict__ rays,
                                                                uint32_t M, uint32_t N, float T_thresh, int binarize,
                                                                float* __restrict__ weights, float* __restrict__ weights_sum,
                                                                float* __restrict__ depth, float* __restrict__ image) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const uint32_t off = (uint32_t)rays[2ull * n], cnt = (uint32_t)rays[2ull * n + 1];
    float r = 0, g = 0, b = 0, ws = 0, d = 0;
    if (cnt != 0 && (unsigned long long)off + cnt <= M) {
        float T = 1.0f;
        const float3p* c = reinterpret_cast<const float3p*>(rgbs) + off;
        const float2p* tt = reinterpret_cast<const float2p*>(ts) + off;
        for (uint32_t s = 0; s < cnt; ++s) {
            const float2p tv = tt[s];
            const float a = alpha_of(sigmas[off + s], tv.y, binarize);
            const float wgt = a * T;
            weights[off + s] = wgt;
            const float3p col = c[s];
            r += wgt * col.x;
            g += wgt * col.y;
            b += wgt * col.z;
            ws += wgt;
            d += wgt / tv.x;
            T *= 1.0f - a;
            if (T < T_thresh) break;
        }
    }
    weights_sum[n] = ws;
    depth[n] = d;
    reinterpret_cast<float3p*>(image)[n] = float3p{r, g, b};
}

__global__ __launch_bounds__(kBlock) void k_composite_train_bwd(
    const float* __restrict__ g_weights, const float* __restrict__ g_wsum, const float* __restrict__ g_depth,
    const float* __restrict__ g_image, const float* __restrict__ sigmas, const float* __restrict__ rgbs,
    const float* __restrict__ ts, const int32_t* __restrict__ rays, const float* __restrict__ weights_sum,
    const float* __restrict__ depth, const float* __restrict__ image, uint32_t M, uint32_t N, float T_thresh,
    int binarize, float* __restrict__ g_sigmas, float* __restrict__ g_rgbs) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const uint32_t off = (uint32_t)rays[2ull * n], cnt = (uint32_t)rays[2ull * n + 1];
    if (cnt == 0 || (unsigned long long)off + cnt > M) return;
    const float3p gi = reinterpret_cast<const float3p*>(g_image)[n];
    const float3p fin = reinterpret_cast<const float3p*>(image)[n];
    const float ws_fin = weights_sum[n], d_fin = depth[n], gws = g_wsum[n], gd = g_depth[n];
    const float3p* c = reinterpret_cast<const float3p*>(rgbs) + off;
    const float2p* tt = reinterpret_cast<const float2p*>(ts) + off;
    float3p* gc = reinterpret_cast<float3p*>(g_rgbs) + off;
    float T = 1.0f, r = 0, g = 0, b = 0, ws = 0, d = 0;
    for (uint32_t s = 0; s < cnt; ++s) {
        const float2p tv = tt[s];
        const float a = alpha_of(sigmas[off + s], tv.y, binarize);
        const float wgt = a * T;
        const float3p col = c[s];
        r += wgt * col.x;
        g += wgt * col.y;
        b += wgt * col.z;
        ws += wgt;
        d += wgt / tv.x;
        T *= 1.0f - a;
        gc[s] = float3p{gi.x * wgt, gi.y * wgt, gi.z * wgt};
        g_sigmas[off + s] = tv.y * (gi.x * (T * col.x - (fin.x - r)) + gi.y * (T * col.y - (fin.y - g)) +
                                    gi.z * (T * col.z - (fin.z - b)) + (gws + g_weights[off + s]) * (T - (ws_fin - ws)) +
                                    gd * (T / tv.x - (d_fin - d)));
        if (T < T_thresh) break;
    }
}

__global__ __launch_bounds__(kBlock) void k_composite_infer(uint32_t n_alive, uint32_t n_step, float T_thresh, int binarize,
                                                            int32_t* __restrict__ rays_alive, float* __restrict__ rays_t,
                                                            const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                                            const float* __restrict__ ts, float* __restrict__ weights_sum,
                                                            float* __restrict__ depth, float* __restrict__ image) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= n_alive) return;
    const int ray = rays_alive[n];
    const unsigned long long base = (unsigned long long)n * n_step;
    const float3p* c = reinterpret_cast<const float3p*>(rgbs) + base;
    const float2p* tt = reinterpret_cast<const float2p*>(ts) + base;
    float3p col = reinterpret_cast<float3p*>(image)[ray];
    float d = depth[ray], wsum = weights_sum[ray];
    float t = 0.0f;
    uint32_t s = 0;
    while (s < n_step) {
        const float2p tv = tt[s];
        if (tv.x == 0) break;   // marcher produced no sample here: ray left the volume
        const float a = alpha_of(sigmas[base + s], tv.y, binarize);
        const float T = 1 - wsum;
        const float wgt = a * T;
        wsum += wgt;
        t = tv.x;
        d += wgt / t;
        const float3p cs = c[s];
        col.x += wgt * cs.x;
        col.y += wgt * cs.y;
        col.z += wgt * cs.z;
        if (T < T_thresh) break;
        ++s;
    }
    if (s < n_step) rays_alive[n] = -1;
    else rays_t[ray] = t;
    weights_sum[ray] = wsum;
    depth[ray] = d;
    reinterpret_cast<float3p*>(image)[ray] = col;
}

// ---------------------------------------------------------------------------
// alive-list compaction (order preserving)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_alive_count(const int32_t* __restrict__ alive, uint32_t n,
                                                        int32_t* __restrict__ block_sums) {
    __shared__ int lds[kBlock / 64 + 1];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const int keep = (i < n && alive[i] >= 0) ? 1 : 0;
    int tot;
    (void)block_excl_scan<kBlock>(keep, &tot, lds);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}
__global__ __launch_bounds__(kBlock) void k_alive_scatter(const int32_t* __restrict__ alive, uint32_t n,
                                                          const int32_t* __restrict__ block_bases, int32_t* __restrict__ out) {
    __shared__ int lds[kBlock / 64 + 1];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const int v = (i < n) ? alive[i] : -1;
    const int keep = v >= 0 ? 1 : 0;
    int tot;
    const int ex = block_excl_scan<kBlock>(keep, &tot, lds);
    if (keep) out[block_bases[blockIdx.x] + ex] = v;
}

// ---------------------------------------------------------------------------
// train branch: cull samples whose composited weight is below a threshold and re-index the rays
// (lib/models/decoders/base_volume_renderer.py:222-243: boolean-mask gathers + cumsum on the host side there)
// ---------------------------------------------------------------------------
// (d_count == nullptr: every one of the M rows is live, the exact form.  Otherwise M is the capacity and the live rows are [0, *d_count):
// rows beyond it are never read, keep nothing, and the outputs' rows at and beyond the kept total are written as zeros.)
__global__ __launch_bounds__(kBlock) void k_cull_count(const float* __restrict__ weights, uint32_t M, const int32_t* __restrict__ d_count,
                                                       float th, int32_t* __restrict__ block_sums) {
    __shared__ int lds[kBlock / 64 + 1];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t live = cap_live(M, d_count);
    const int keep = (i < live && weights[i] > th) ? 1 : 0;
    int tot;
    (void)block_excl_scan<kBlock>(keep, &tot, lds);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}
__global__ __launch_bounds__(kBlock) void k_cull_scatter(const float* __restrict__ weights, uint32_t M, const int32_t* __restrict__ d_count,
                                                         float th, const int32_t* __restrict__ block_bases, const int32_t* __restrict__ total,
                                                         const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                         const float* __restrict__ ts, float* __restrict__ o_xyzs,
                                                         float* __restrict__ o_dirs, float* __restrict__ o_ts, int32_t* __restrict__ pref) {
    __shared__ int lds[kBlock / 64 + 1];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t live = cap_live(M, d_count);
    const int keep = (i < live && weights[i] > th) ? 1 : 0;
    int tot;
    const int ex = block_excl_scan<kBlock>(keep, &tot, lds);
    const int dst = block_bases[blockIdx.x] + ex;
    const int kept = *total;
    if (i < M) pref[i] = i < live ? dst : kept;   // = cumsum(mask)[i - 1], the reference's filt_inds[i]
    if (i == 0) pref[M] = kept;
    if (keep) {
        reinterpret_cast<float3p*>(o_xyzs)[dst] = reinterpret_cast<const float3p*>(xyzs)[i];
        reinterpret_cast<float3p*>(o_dirs)[dst] = reinterpret_cast<const float3p*>(dirs)[i];
        reinterpret_cast<float2p*>(o_ts)[dst] = reinterpret_cast<const float2p*>(ts)[i];
    }
    if (d_count && i < M && i >= (uint32_t)kept) {   // zero tail (dst < kept for every kept sample: no row is written twice)
        reinterpret_cast<float3p*>(o_xyzs)[i] = float3p{0.f, 0.f, 0.f};
        reinterpret_cast<float3p*>(o_dirs)[i] = float3p{0.f, 0.f, 0.f};
        reinterpret_cast<float2p*>(o_ts)[i] = float2p{0.f, 0.f};
    }
}
__global__ __launch_bounds__(kBlock) void k_cull_rays(const int32_t* __restrict__ rays, uint32_t N, const int32_t* __restrict__ pref,
                                                      uint32_t M, const int32_t* __restrict__ d_count, int32_t* __restrict__ o_rays) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const int off = rays[2 * n], cnt = rays[2 * n + 1];
    if (d_count) {   // a ray that did not fit keeps nothing and pref is not read past the live count
        cap_cull_ray(off, cnt, cap_live(M, d_count), pref, o_rays + 2 * n, o_rays + 2 * n + 1);
        return;
    }
    const int a = pref[off], b = pref[off + cnt];
    o_rays[2 * n] = a;
    o_rays[2 * n + 1] = b - a;
}

// clamp step of the capacity form: marched total -> live count of whole rays that fit, sticky overflow flag
__global__ __launch_bounds__(kBlock) void k_march_clamp(const int32_t* __restrict__ rays, uint32_t N, const int32_t* __restrict__ d_total,
                                                        uint32_t capacity, int32_t* __restrict__ n_samples, int32_t* __restrict__ d_count,
                                                        int32_t* __restrict__ d_overflow) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n == 0) {
        const int32_t total = *d_total;
        n_samples[0] = total;
        if (total < 0 || (uint32_t)total > capacity) *d_overflow = 1;
        if (N == 0) { *d_count = 0; n_samples[1] = 0; }
    }
    if (n >= N) return;
    int32_t count;
    if (cap_clamp_decides(rays, n, N, capacity, &count)) { *d_count = count; n_samples[1] = count; }
}

// ---------------------------------------------------------------------------
// density-grid refresh (update_extra_state, base_volume_renderer.py:105-177)
// ---------------------------------------------------------------------------
// cell coordinates -> Morton index and jittered query position.  coords == nullptr: cell i of the full grid in
// (x, y, z) meshgrid order, x slowest (custom_meshgrid 'ij').
__global__ __launch_bounds__(kBlock) void k_grid_points(const int32_t* __restrict__ coords, const float* __restrict__ noise, uint32_t N,
                                                        uint32_t H, float bound, float* __restrict__ xyzs, int32_t* __restrict__ indices) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    uint32_t c[3];
    if (coords) { c[0] = (uint32_t)coords[3 * i]; c[1] = (uint32_t)coords[3 * i + 1]; c[2] = (uint32_t)coords[3 * i + 2]; }
    else { c[0] = i / (H * H); c[1] = (i / H) % H; c[2] = i % H; }
    indices[i] = (int32_t)morton_encode(c[0], c[1], c[2]);
    const float half = bound / (float)H, cell = 2.0f * bound / (float)H, mid = ((float)H - 1.0f) / 2.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float x = ((float)c[k] - mid) * cell;
        x += noise ? noise[3 * i + k] * (2.0f * half) - half : 0.0f;
        xyzs[3 * i + k] = x;
    }
}
__global__ __launch_bounds__(kBlock) void k_grid_scatter(const float* __restrict__ sigmas, const int32_t* __restrict__ indices, uint32_t N,
                                                         float* __restrict__ tmp_grid) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    // sigmas.clamp(max=finfo.max) of the reference (base_volume_renderer.py:166): +inf becomes FLT_MAX, a NaN stays a NaN -- its
    // (tmp >= 0) test then fails and the cell keeps its old density, where fminf would have marked it occupied at maximum density
    if (i < N) { const float sg = sigmas[i]; tmp_grid[indices[i]] = sg != sg ? sg : fminf(sg, 3.4028234663852886e38f); }
}
// grid = where(grid >= 0 & tmp >= 0, max(grid * decay, tmp), grid); per-block partial sums of clamp(grid, 0) in fp64
__global__ __launch_bounds__(kBlock) void k_grid_ema(float* __restrict__ grid, const float* __restrict__ tmp, uint32_t n, float decay,
                                                     double* __restrict__ partial) {
    __shared__ double red[kBlock / 64];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        float g = grid[i];
        const float t = tmp[i];
        if (g >= 0.0f && t >= 0.0f) { g = fmaxf(g * decay, t); grid[i] = g; }
        v = (double)fmaxf(g, 0.0f);
    }
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < kBlock / 64; ++k) t += red[k];
        partial[blockIdx.x] = t;
    }
}
__global__ void k_grid_mean(const double* __restrict__ partial, uint32_t nblk, uint32_t n, float* __restrict__ mean) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double t = 0.0;
        for (uint32_t k = 0; k < nblk; ++k) t += partial[k];
        *mean = (float)(t / (double)n);
    }
}

MarchParams make_params(const uint8_t* grid, float bound, int contract, float dt_gamma, uint32_t max_steps, uint32_t C,
                        uint32_t H) {
    MarchParams p;
    p.grid = grid; p.bound = bound; p.contract = contract; p.dt_gamma = dt_gamma;
    p.max_steps = max_steps; p.C = C; p.H = H;
    return p;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int mve_near_far_from_aabb(const float* o, const float* d, const float* aabb, uint32_t N, float min_near, float* nears,
                           float* fars, void* stream) {
    if (N == 0) return MVE_OK;
    MVE_CHECK(o && d && aabb && nears && fars, MVE_ERR_ARG, "near_far_from_aabb: null pointer");
    k_near_far<<<mve_cdiv(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(o, d, aabb, N, min_near, nears, fars);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_morton3d(const int32_t* coords, uint32_t N, int32_t* indices, void* stream) {
    if (N == 0) return MVE_OK;
    MVE_CHECK(coords && indices, MVE_ERR_ARG, "morton3d: null pointer");
    k_morton<<<mve_cdiv(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(coords, N, indices);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_morton3d_invert(const int32_t* indices, uint32_t N, int32_t* coords, void* stream) {
    if (N == 0) return MVE_OK;
    MVE_CHECK(coords && indices, MVE_ERR_ARG, "morton3d_invert: null pointer");
    k_morton_inv<<<mve_cdiv(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(indices, N, coords);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_packbits(const float* grid, uint32_t n_bytes, float thresh, uint8_t* bits, void* stream) {
    if (n_bytes == 0) return MVE_OK;
    MVE_CHECK(grid && bits, MVE_ERR_ARG, "packbits: null pointer");
    const uint32_t n_words = mve_cdiv(n_bytes, 4);
    k_packbits<<<mve_cdiv(n_words, kBlock), kBlock, 0, (hipStream_t)stream>>>(grid, n_bytes, thresh, bits);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_flatten_rays(const int32_t* rays, uint32_t N, uint32_t M, int32_t* res, void* stream) {
    if (N == 0) return MVE_OK;
    MVE_CHECK(rays && res, MVE_ERR_ARG, "flatten_rays: null pointer");
    k_flatten_rays<<<mve_cdiv(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(rays, N, M, res);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

size_t mve_march_scratch_bytes(uint32_t N) { return sizeof(int32_t) * ((size_t)mve_cdiv(N, kBlock) + 64); }

int mve_march_rays_train_count(const float* o, const float* d, const uint8_t* grid, float bound, int contract,
                               float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H,
                               const float* nears, const float* fars, const float* noises, int32_t* rays,
                               int32_t* total, void* scratch, void* stream) {
    MVE_CHECK(total, MVE_ERR_ARG, "march_rays_train_count: null total");
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        MVE_HIP(hipMemsetAsync(total, 0, sizeof(int32_t), s));
        return MVE_OK;
    }
    MVE_CHECK(o && d && grid && nears && fars && noises && rays && scratch, MVE_ERR_ARG,
              "march_rays_train_count: null pointer");
    MVE_CHECK(H > 0 && H <= 1024 && C >= 1 && max_steps > 0, MVE_ERR_ARG,
              "march_rays_train_count: bad grid (C=%u H=%u max_steps=%u)", C, H, max_steps);
    const MarchParams p = make_params(grid, bound, contract, dt_gamma, max_steps, C, H);
    const uint32_t nblk = mve_cdiv(N, kBlock);
    int32_t* bs = (int32_t*)scratch;
    k_march_count<<<nblk, kBlock, 0, s>>>(p, o, d, N, nears, fars, noises, rays, bs);
    MVE_LAUNCH_CHECK();
    k_scan_block_sums<<<1, 1024, 0, s>>>(bs, nblk, total);
    MVE_LAUNCH_CHECK();
    k_ray_offsets<<<nblk, kBlock, 0, s>>>(rays, N, bs);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_march_rays_train_write(const float* o, const float* d, const uint8_t* grid, float bound, int contract,
                               float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H,
                               const float* nears, const float* fars, const float* noises, const int32_t* rays,
                               uint32_t capacity, float* xyzs, float* dirs, float* ts, void* stream) {
    if (N == 0 || capacity == 0) return MVE_OK;
    MVE_CHECK(o && d && grid && nears && fars && noises && rays && xyzs && dirs && ts, MVE_ERR_ARG,
              "march_rays_train_write: null pointer");
    const MarchParams p = make_params(grid, bound, contract, dt_gamma, max_steps, C, H);
    k_march_write<<<mve_cdiv(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(p, o, d, N, nears, fars, noises, rays,
                                                                           capacity, xyzs, dirs, ts);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* ts, const int32_t* rays,
                                     uint32_t M, uint32_t N, float T_thresh, int binarize, float* weights,
                                     float* weights_sum, float* depth, float* image, void* stream) {
    if (N == 0) return MVE_OK;
    MVE_CHECK(rays && weights_sum && depth && image, MVE_ERR_ARG, "composite_rays_train_forward: null pointer");
    MVE_CHECK(M == 0 || (sigmas && rgbs && ts && weights), MVE_ERR_ARG, "composite_rays_train_forward: null sample buffer");
    k_composite_train_fwd<<<mve_cdiv(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(
        sigmas, rgbs, ts, rays, M, N, T_thresh, binarize, weights, weights_sum, depth, image);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_composite_rays_train_backward(const float* g_weights, const float* g_wsum, const float* g_depth,
                                      const float* g_image, const float* sigmas, const float* rgbs, const float* ts,
                                      const int32_t* rays, const float* weights_sum, const float* depth,
                                      const float* image, uint32_t M, uint32_t N, float T_thresh, int binarize,
                                      float* g_sigmas, float* g_rgbs, void* stream) {
    if (N == 0 || M == 0) return MVE_OK;
    MVE_CHECK(g_weights && g_wsum && g_depth && g_image && sigmas && rgbs && ts && rays && weights_sum && depth &&
                  image && g_sigmas && g_rgbs,
              MVE_ERR_ARG, "composite_rays_train_backward: null pointer");
    k_composite_train_bwd<<<mve_cdiv(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(
        g_weights, g_wsum, g_depth, g_image, sigmas, rgbs, ts, rays, weights_sum, depth, image, M, N, T_thresh,
        binarize, g_sigmas, g_rgbs);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t, const float* o,
                   const float* d, float bound, int contract, float dt_gamma, uint32_t max_steps, uint32_t C,
                   uint32_t H, const uint8_t* grid, const float* nears, const float* fars, float* xyzs, float* dirs,
                   float* ts, const float* noises, void* stream) {
    if (n_alive == 0 || n_step == 0) return MVE_OK;
    MVE_CHECK(rays_alive && rays_t && o && d && grid && nears && fars && xyzs && dirs && ts && noises, MVE_ERR_ARG,
              "march_rays: null pointer");
    MVE_CHECK(H > 0 && H <= 1024 && C >= 1 && max_steps > 0, MVE_ERR_ARG, "march_rays: bad grid (C=%u H=%u)", C, H);
    const MarchParams p = make_params(grid, bound, contract, dt_gamma, max_steps, C, H);
    k_march_infer<<<mve_cdiv(n_alive, kBlock), kBlock, 0, (hipStream_t)stream>>>(
        p, n_alive, n_step, rays_alive, rays_t, o, d, nears, fars, xyzs, dirs, ts, noises);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int binarize, int32_t* rays_alive,
                       float* rays_t, const float* sigmas, const float* rgbs, const float* ts, float* weights_sum,
                       float* depth, float* image, void* stream) {
    if (n_alive == 0 || n_step == 0) return MVE_OK;
    MVE_CHECK(rays_alive && rays_t && sigmas && rgbs && ts && weights_sum && depth && image, MVE_ERR_ARG,
              "composite_rays: null pointer");
    k_composite_infer<<<mve_cdiv(n_alive, kBlock), kBlock, 0, (hipStream_t)stream>>>(
        n_alive, n_step, T_thresh, binarize, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_compact_alive(const int32_t* rays_alive, uint32_t n_alive, int32_t* out, int32_t* n_out, void* scratch,
                      void* stream) {
    MVE_CHECK(n_out, MVE_ERR_ARG, "compact_alive: null n_out");
    hipStream_t s = (hipStream_t)stream;
    if (n_alive == 0) {
        MVE_HIP(hipMemsetAsync(n_out, 0, sizeof(int32_t), s));
        return MVE_OK;
    }
    MVE_CHECK(rays_alive && out && scratch, MVE_ERR_ARG, "compact_alive: null pointer");
    const uint32_t nblk = mve_cdiv(n_alive, kBlock);
    int32_t* bs = (int32_t*)scratch;
    k_alive_count<<<nblk, kBlock, 0, s>>>(rays_alive, n_alive, bs);
    MVE_LAUNCH_CHECK();
    k_scan_block_sums<<<1, 1024, 0, s>>>(bs, nblk, n_out);
    MVE_LAUNCH_CHECK();
    k_alive_scatter<<<nblk, kBlock, 0, s>>>(rays_alive, n_alive, bs, out);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

size_t mve_cull_scratch_bytes(uint32_t M) { return sizeof(int32_t) * ((size_t)mve_cdiv(M, kBlock) + 64); }

// shared body of mve_cull_samples (d_count == nullptr, M exact) and mve_cull_samples_n (M = capacity, live rows from the device)
static int cull_samples_impl(const char* who, const float* weights, uint32_t M, const int32_t* d_count, float threshold, const int32_t* rays,
                             uint32_t N, const float* xyzs, const float* dirs, const float* ts, float* out_xyzs, float* out_dirs, float* out_ts,
                             int32_t* out_rays, int32_t* pref /* [M + 1] */, int32_t* n_out, void* scratch, void* stream) {
    MVE_CHECK(n_out && pref, MVE_ERR_ARG, "%s: null n_out / pref", who);
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        MVE_HIP(hipMemsetAsync(n_out, 0, sizeof(int32_t), s));
        MVE_HIP(hipMemsetAsync(pref, 0, sizeof(int32_t), s));
    } else {
        MVE_CHECK(weights && xyzs && dirs && ts && out_xyzs && out_dirs && out_ts && scratch, MVE_ERR_ARG, "%s: null pointer", who);
        const uint32_t nblk = mve_cdiv(M, kBlock);
        int32_t* bs = (int32_t*)scratch;
        k_cull_count<<<nblk, kBlock, 0, s>>>(weights, M, d_count, threshold, bs);
        MVE_LAUNCH_CHECK();
        k_scan_block_sums<<<1, 1024, 0, s>>>(bs, nblk, n_out);
        MVE_LAUNCH_CHECK();
        k_cull_scatter<<<nblk, kBlock, 0, s>>>(weights, M, d_count, threshold, bs, n_out, xyzs, dirs, ts, out_xyzs, out_dirs, out_ts, pref);
        MVE_LAUNCH_CHECK();
    }
    if (N) {
        MVE_CHECK(rays && out_rays, MVE_ERR_ARG, "%s: null rays", who);
        k_cull_rays<<<mve_cdiv(N, kBlock), kBlock, 0, s>>>(rays, N, pref, M, d_count, out_rays);
        MVE_LAUNCH_CHECK();
    }
    return MVE_OK;
}

int mve_cull_samples(const float* weights, uint32_t M, float threshold, const int32_t* rays, uint32_t N, const float* xyzs,
                     const float* dirs, const float* ts, float* out_xyzs, float* out_dirs, float* out_ts, int32_t* out_rays,
                     int32_t* pref /* [M + 1] */, int32_t* n_out, void* scratch, void* stream) {
    return cull_samples_impl("cull_samples", weights, M, nullptr, threshold, rays, N, xyzs, dirs, ts, out_xyzs, out_dirs, out_ts, out_rays, pref,
                             n_out, scratch, stream);
}

int mve_cull_samples_n(const float* weights, uint32_t capacity, const int32_t* d_count, float threshold, const int32_t* rays, uint32_t N,
                       const float* xyzs, const float* dirs, const float* ts, float* out_xyzs, float* out_dirs, float* out_ts,
                       int32_t* out_rays, int32_t* pref /* [capacity + 1] */, int32_t* n_out, void* scratch, void* stream) {
    MVE_CHECK(d_count && d_count != n_out, MVE_ERR_ARG, "cull_samples_n: the input count must be a device int32 other than n_out");
    return cull_samples_impl("cull_samples_n", weights, capacity, d_count, threshold, rays, N, xyzs, dirs, ts, out_xyzs, out_dirs, out_ts,
                             out_rays, pref, n_out, scratch, stream);
}

int mve_march_rays_train_clamp(const int32_t* rays, uint32_t N, const int32_t* d_total, uint32_t capacity, int32_t* d_n_samples,
                               int32_t* d_count, int32_t* d_overflow, void* stream) {
    MVE_CHECK(d_total && d_n_samples && d_count && d_overflow && (N == 0 || rays), MVE_ERR_ARG, "march_rays_train_clamp: null pointer");
    k_march_clamp<<<N ? mve_cdiv(N, kBlock) : 1, kBlock, 0, (hipStream_t)stream>>>(rays, N, d_total, capacity, d_n_samples, d_count, d_overflow);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_density_grid_points(const int32_t* coords, const float* noise, uint32_t N, uint32_t grid_size, float bound, float* xyzs,
                            int32_t* indices, void* stream) {
    if (N == 0) return MVE_OK;
    MVE_CHECK(xyzs && indices && grid_size > 0, MVE_ERR_ARG, "density_grid_points: bad arguments");
    MVE_CHECK(coords || (uint64_t)N == (uint64_t)grid_size * grid_size * grid_size, MVE_ERR_ARG,
              "density_grid_points: without coords N must be grid_size^3");
    k_grid_points<<<mve_cdiv(N, kBlock), kBlock, 0, (hipStream_t)stream>>>(coords, noise, N, grid_size, bound, xyzs, indices);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

size_t mve_density_grid_scratch_bytes(uint32_t n_cells) { return sizeof(double) * ((size_t)mve_cdiv(n_cells, kBlock) + 8); }

int mve_density_grid_update(float* density_grid, float* tmp_grid, uint32_t n_cells, const float* sigmas, const int32_t* indices,
                            uint32_t N, float decay, float* mean_density, void* scratch, void* stream) {
    MVE_CHECK(density_grid && tmp_grid && mean_density && scratch && n_cells > 0, MVE_ERR_ARG, "density_grid_update: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (N) {
        MVE_CHECK(sigmas && indices, MVE_ERR_ARG, "density_grid_update: null sigmas / indices");
        k_grid_scatter<<<mve_cdiv(N, kBlock), kBlock, 0, s>>>(sigmas, indices, N, tmp_grid);
        MVE_LAUNCH_CHECK();
    }
    const uint32_t nblk = mve_cdiv(n_cells, kBlock);
    k_grid_ema<<<nblk, kBlock, 0, s>>>(density_grid, tmp_grid, n_cells, decay, (double*)scratch);
    MVE_LAUNCH_CHECK();
    k_grid_mean<<<1, 64, 0, s>>>((const double*)scratch, nblk, n_cells, mean_density);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // extern "C"
