// Stand-alone tiny-cuda-nn HashGrid encoding for gfx950: forward, d/dtable and d/dx, the kernels behind mvedit_amd.tinycudann.Encoding.
//
// The reference builds its hash-grid encoder as `tcnn.Encoding(n_input_dims=3, {"otype": "HashGrid", ...}, dtype=torch.float32)`
// (lib/models/decoders/ingp_decoder.py:62-74, triplane_ingp_decoder.py:102-114) and owns the MLP as nn.Linear layers, so the
// reconstruct step back-propagates into `encoder.params` on its own.  nerf.hip / triplane.hip fuse the same encoding with an MLP;
// here it stands alone: x [N,3] in the unit cube -> enc [N, L*F], and the transposes of that map.
//
// Index rules are hashgrid.h's (dense strides while they fit, else the coherent prime hash of a 2^k-row level).  One lane per point,
// the level loop rolled (one level's 8 corner gathers in flight, not all 8 L: see the sched_barrier note in hashgrid.h).  The
// [N, L*F] rows are staged through LDS so global reads / writes of them are coalesced (a lane's own row is L*F*4 bytes wide).
#include "hashgrid.h"

namespace {

constexpr int MERGE_STEPS = 4;      // butterfly over aligned blocks of 2, 4, 8, 16 lanes (as k_decode_backward in nerf.hip)

struct EncodeParams {
    const float* table;             // [rows][F]
    float scale[MAX_LEVELS];
    uint32_t res[MAX_LEVELS], off[MAX_LEVELS], size[MAX_LEVELS];
    uint32_t hashed;                // bit l: level l is hashed
    int n_levels;
};

// T points per block; staging tile [T][L*F + 1] floats (odd row pitch: a lane's scalar writes hit distinct banks).  <= 33 KiB.
inline int block_points(int lf) { return lf <= 32 ? 256 : 64; }
inline size_t stage_bytes(int lf) { return sizeof(float) * (size_t)block_points(lf) * (lf + 1); }

template <int F>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float (&v)[F]) {
    if constexpr (F == 1) {
        v[0] = p[0];
    } else if constexpr (F == 2) {
        const float2p t = *reinterpret_cast<const float2p*>(p);
        v[0] = t.x; v[1] = t.y;
    } else {
#pragma unroll
        for (int q = 0; q < F / 4; ++q) {
            const f32x4 t = reinterpret_cast<const f32x4*>(p)[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[4 * q + k] = t[k];
        }
    }
}

// cell, interpolation weight and its derivative d w / d x (pos = scale x + 0.5) of one level, per axis
template <bool SMOOTH>
__device__ __forceinline__ void level_cell(float scale, const float (&u)[3], uint32_t (&cell)[3], float (&w)[3], float (&dw)[3]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float pos = fmaf(scale, u[d], 0.5f);
        const float fl = floorf(pos);
        cell[d] = (uint32_t)(int)fl;
        const float fr = pos - fl;
        if (SMOOTH) {
            w[d] = fr * fr * (3.0f - 2.0f * fr);
            dw[d] = 6.0f * fr * (1.0f - fr) * scale;
        } else {
            w[d] = fr;
            dw[d] = scale;
        }
    }
}

// row (within the level) and trilinear weight of corner `corner` (bit d set: cell + 1 along axis d)
__device__ __forceinline__ void corner_of(int corner, const uint32_t (&cell)[3], const float (&w)[3], bool hashed, uint32_t res, uint32_t size,
                                          uint32_t& row, float& wt) {
    uint32_t c[3];
    wt = 1.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (corner & (1 << d)) { wt = wt * w[d]; c[d] = cell[d] + 1u; }
        else { wt = wt * (1.0f - w[d]); c[d] = cell[d]; }
    }
    row = level_row(c, hashed, res, size);
}

template <int F, bool SMOOTH>
__global__ __launch_bounds__(256) void k_hashgrid_encode(EncodeParams p, const float* __restrict__ xyz, uint32_t N, float* __restrict__ out) {
    extern __shared__ float stage[];
    const int T = blockDim.x, L = p.n_levels, LF = L * F, S = LF + 1;
    const uint32_t base = blockIdx.x * (uint32_t)T;
    const uint32_t i = base + threadIdx.x;
    if (i < N) {
        const float3p q = reinterpret_cast<const float3p*>(xyz)[i];
        const float u[3] = {q.x, q.y, q.z};
        float* st = stage + threadIdx.x * S;
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            const uint32_t res = p.res[l], size = p.size[l];
            const bool hashed = (p.hashed >> l) & 1u;
            uint32_t cell[3];
            float w[3], dw[3];
            level_cell<SMOOTH>(p.scale[l], u, cell, w, dw);
            const float* tab = p.table + (size_t)p.off[l] * F;
            float acc[F];
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] = 0.0f;
#pragma unroll
            for (int corner = 0; corner < 8; ++corner) {
                uint32_t row;
                float wt;
                corner_of(corner, cell, w, hashed, res, size, row, wt);
                float v[F];
                load_row<F>(tab + (size_t)row * F, v);
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] = fmaf(wt, v[f], acc[f]);
            }
#pragma unroll
            for (int f = 0; f < F; ++f) st[l * F + f] = acc[f];
        }
    }
    __syncthreads();
    // the block's rows are T*L*F contiguous floats of `out`: element e = (row e / LF, column e % LF), walked incrementally
    const uint32_t cnt = min((uint32_t)T, N - base) * (uint32_t)LF;
    float* o = out + (size_t)base * LF;
    uint32_t r = threadIdx.x / LF, c = threadIdx.x % LF;
    const uint32_t dq = T / LF, dr = T % LF;
    for (uint32_t e = threadIdx.x; e < cnt; e += T) {
        o[e] = stage[r * S + c];
        r += dq; c += dr;
        if (c >= (uint32_t)LF) { c -= LF; ++r; }
    }
}

// d table [rows][F] += sum over points and corners of  corner weight * g[point][l F .. l F + F)   (float atomics, as tiny-cuda-nn)
// d x [N][3] = sum over levels, corners and features of  d(corner weight)/dx * table[row][f] * g[point][l F + f]   (when DX)
template <int F, bool SMOOTH, bool DX>
__global__ __launch_bounds__(256) void k_hashgrid_encode_backward(EncodeParams p, const float* __restrict__ xyz, uint32_t N,
                                                                  const float* __restrict__ genc, float* __restrict__ gtable,
                                                                  float* __restrict__ gx) {
    extern __shared__ float stage[];
    const int T = blockDim.x, L = p.n_levels, LF = L * F, S = LF + 1;
    const uint32_t base = blockIdx.x * (uint32_t)T;
    {   // coalesced read of the block's incoming gradient rows into the staging tile
        const uint32_t cnt = min((uint32_t)T, N - base) * (uint32_t)LF;
        const float* g = genc + (size_t)base * LF;
        uint32_t r = threadIdx.x / LF, c = threadIdx.x % LF;
        const uint32_t dq = T / LF, dr = T % LF;
        for (uint32_t e = threadIdx.x; e < cnt; e += T) {
            stage[r * S + c] = g[e];
            r += dq; c += dr;
            if (c >= (uint32_t)LF) { c -= LF; ++r; }
        }
    }
    __syncthreads();
    // every lane stays to the end (the merge below moves sums across lanes); a lane past the last point redoes point N - 1 with a zero
    // incoming gradient and scatters nothing
    const uint32_t i = base + threadIdx.x;
    const bool valid = i < N;
    const uint32_t m = valid ? i : N - 1;
    const float3p q = reinterpret_cast<const float3p*>(xyz)[m];
    const float u[3] = {q.x, q.y, q.z};
    const float* st = stage + threadIdx.x * S;
    const int lane = threadIdx.x & 63;
    float gxa[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
        const uint32_t res = p.res[l], size = p.size[l];
        const bool hashed = (p.hashed >> l) & 1u;
        uint32_t cell[3];
        float w[3], dw[3];
        level_cell<SMOOTH>(p.scale[l], u, cell, w, dw);
        float g[F];
#pragma unroll
        for (int f = 0; f < F; ++f) g[f] = valid ? st[l * F + f] : 0.0f;
        // Points arrive in ray order: neighbouring lanes share the cells of coarse levels and would send the same 8 rows F float atomics
        // each -- 64 lanes in 64 different rows per wave-instruction run ~17x below the chip's atomic rate.  So lanes merge first: the leader
        // of an aligned block of d lanes takes its partner block's leader's sums when both hold the same cell (exact comparison of all
        // three coordinates), and only lanes still holding sums scatter.  (Summation order changes, as it does with every run of the atomics.)
        bool alive = valid;
        bool take[MERGE_STEPS];
#pragma unroll
        for (int s = 0; s < MERGE_STEPS; ++s) {
            const int d = 1 << s;
            const uint32_t p0 = (uint32_t)__shfl_xor((int)cell[0], d, 64), p1 = (uint32_t)__shfl_xor((int)cell[1], d, 64),
                           p2 = (uint32_t)__shfl_xor((int)cell[2], d, 64);
            const int palive = __shfl_xor((int)alive, d, 64);
            const bool can = ((lane & (d - 1)) == 0) && alive && palive && p0 == cell[0] && p1 == cell[1] && p2 == cell[2];
            take[s] = can && !(lane & d);
            alive = alive && !(can && (lane & d));
        }
        bool any_take = false;
#pragma unroll
        for (int s = 0; s < MERGE_STEPS; ++s) any_take = any_take || take[s];
        const bool merge = __any(any_take);             // wave-uniform: fine levels hold ~1 point per cell, nothing to move
        const float* tab = p.table + (size_t)p.off[l] * F;
        float* gt = gtable + (size_t)p.off[l] * F;
        // four corners at a time (all 8 F sums at once would not leave registers for the merge at F = 8)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float cs[4][F];
            uint32_t rows[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int corner = 4 * half + j;
                float wt;
                corner_of(corner, cell, w, hashed, res, size, rows[j], wt);
#pragma unroll
                for (int f = 0; f < F; ++f) cs[j][f] = wt * g[f];
                if (DX) {
                    float v[F];
                    load_row<F>(tab + (size_t)rows[j] * F, v);
                    float dot = 0.0f;
#pragma unroll
                    for (int f = 0; f < F; ++f) dot = fmaf(g[f], v[f], dot);
                    // d wt / d x_d: the factor of axis d replaced by its derivative (+dw for the upper corner, -dw for the lower)
                    float fac[3];
#pragma unroll
                    for (int d = 0; d < 3; ++d) fac[d] = (corner & (1 << d)) ? w[d] : 1.0f - w[d];
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const float dd = (corner & (1 << d)) ? dw[d] : -dw[d];
                        const float o1 = fac[(d + 1) % 3], o2 = fac[(d + 2) % 3];
                        gxa[d] = fmaf(dd * o1 * o2, dot, gxa[d]);
                    }
                }
            }
            if (merge) {
#pragma unroll
                for (int s = 0; s < MERGE_STEPS; ++s) {
                    const int d = 1 << s;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
#pragma unroll
                        for (int f = 0; f < F; ++f) {
                            const float pv = __shfl_xor(cs[j][f], d, 64);
                            cs[j][f] += take[s] ? pv : 0.0f;
                        }
                    }
                }
            }
            if (alive) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int f = 0; f < F; ++f) atomicAdd(gt + (size_t)rows[j] * F + f, cs[j][f]);
                }
            }
        }
    }
    if (DX && valid) reinterpret_cast<float3p*>(gx)[i] = float3p{gxa[0], gxa[1], gxa[2]};
}

int fill_encode(EncodeParams& p, const float* table, uint32_t n_rows, int F, int n_levels, const float* scales, const uint32_t* res,
                const uint32_t* off, const uint32_t* size, int interpolation, const char* who) {
    MVE_CHECK(F == 1 || F == 2 || F == 4 || F == 8, MVE_ERR_ARG, "%s: n_features must be 1, 2, 4 or 8 (got %d)", who, F);
    MVE_CHECK(n_levels >= 1 && n_levels <= MAX_LEVELS, MVE_ERR_ARG, "%s: n_levels must be in [1, %d] (got %d)", who, MAX_LEVELS, n_levels);
    MVE_CHECK(interpolation == MVE_INTERP_LINEAR || interpolation == MVE_INTERP_SMOOTHSTEP, MVE_ERR_ARG,
              "%s: interpolation must be MVE_INTERP_LINEAR or MVE_INTERP_SMOOTHSTEP (got %d)", who, interpolation);
    MVE_CHECK(scales && res && off && size, MVE_ERR_ARG, "%s: null level table", who);
    p.table = table;
    p.n_levels = n_levels;
    p.hashed = 0;
    for (int l = 0; l < n_levels; ++l) {
        MVE_CHECK(size[l] > 0 && res[l] > 0, MVE_ERR_ARG, "%s: empty level %d", who, l);
        MVE_CHECK((uint64_t)off[l] + size[l] <= n_rows, MVE_ERR_ARG, "%s: level %d (rows %u..%u) lies outside the %u-row table", who, l, off[l],
                  off[l] + size[l], n_rows);
        const bool hashed = level_is_hashed(res[l], size[l]);
        MVE_CHECK(!hashed || (size[l] & (size[l] - 1u)) == 0u, MVE_ERR_ARG, "%s: hashed level %d has %u rows, not a power of two", who, l, size[l]);
        p.scale[l] = scales[l]; p.res[l] = res[l]; p.off[l] = off[l]; p.size[l] = size[l];
        p.hashed |= (hashed ? 1u : 0u) << l;
    }
    return MVE_OK;
}

}  // namespace

extern "C" {

int mve_hashgrid_encode(const float* d_x, uint32_t N, const float* d_table, uint32_t n_rows, int n_features, int n_levels,
                        const float* level_scale, const uint32_t* level_res, const uint32_t* level_offset, const uint32_t* level_size,
                        int interpolation, float* d_out, void* stream) {
    EncodeParams p;
    int rc = fill_encode(p, d_table, n_rows, n_features, n_levels, level_scale, level_res, level_offset, level_size, interpolation,
                         "hashgrid_encode");
    if (rc) return rc;
    if (N == 0) return MVE_OK;
    MVE_CHECK(d_x && d_table && d_out, MVE_ERR_ARG, "hashgrid_encode: null pointer");
    const int lf = n_levels * n_features, T = block_points(lf);
    const size_t lds = stage_bytes(lf);
    const unsigned grid = mve_cdiv(N, T);
    hipStream_t s = (hipStream_t)stream;
    const bool smooth = interpolation == MVE_INTERP_SMOOTHSTEP;
#define GO(FF) (smooth ? k_hashgrid_encode<FF, true><<<grid, T, lds, s>>>(p, d_x, N, d_out) : k_hashgrid_encode<FF, false><<<grid, T, lds, s>>>(p, d_x, N, d_out))
    switch (n_features) {
        case 1: GO(1); break;
        case 2: GO(2); break;
        case 4: GO(4); break;
        default: GO(8); break;
    }
#undef GO
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_hashgrid_encode_backward(const float* d_x, uint32_t N, const float* d_table, uint32_t n_rows, int n_features, int n_levels,
                                 const float* level_scale, const uint32_t* level_res, const uint32_t* level_offset,
                                 const uint32_t* level_size, int interpolation, const float* d_grad_enc, float* d_grad_table,
                                 float* d_grad_x, void* stream) {
    EncodeParams p;
    int rc = fill_encode(p, d_table, n_rows, n_features, n_levels, level_scale, level_res, level_offset, level_size, interpolation,
                         "hashgrid_encode_backward");
    if (rc) return rc;
    if (N == 0) return MVE_OK;
    MVE_CHECK(d_x && d_grad_enc && d_grad_table, MVE_ERR_ARG, "hashgrid_encode_backward: null pointer");
    MVE_CHECK(d_table || !d_grad_x, MVE_ERR_ARG, "hashgrid_encode_backward: d/dx needs the table");
    const int lf = n_levels * n_features, T = block_points(lf);
    const size_t lds = stage_bytes(lf);
    const unsigned grid = mve_cdiv(N, T);
    hipStream_t s = (hipStream_t)stream;
    const bool smooth = interpolation == MVE_INTERP_SMOOTHSTEP;
#define GO3(FF, SM, DX) k_hashgrid_encode_backward<FF, SM, DX><<<grid, T, lds, s>>>(p, d_x, N, d_grad_enc, d_grad_table, d_grad_x)
#define GO(FF)                                             \
    do {                                                   \
        if (d_grad_x) { if (smooth) GO3(FF, true, true); else GO3(FF, false, true); }      \
        else { if (smooth) GO3(FF, true, false); else GO3(FF, false, false); }             \
    } while (0)
    switch (n_features) {
        case 1: GO(1); break;
        case 2: GO(2); break;
        case 4: GO(4); break;
        default: GO(8); break;
    }
#undef GO
#undef GO3
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // extern "C"
