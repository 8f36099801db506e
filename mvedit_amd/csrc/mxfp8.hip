// MXFP8 (OCP MX: e4m3 elements, one E8M0 scale per 32 elements along K) on gfx950's block-scaled MFMA.
// The packed format, the scale rule and the argument constraints are specified in include/mvedit_amd.h (section 2b) and, as executable
// text, by mvedit_amd/mxfp8.py: quantize_host / dequantize_host.  Two kernels:
//   k_mxfp8_quantize : one pass over a [R, K] f32 / f16 / bf16 matrix -> q bytes + scale bytes, padding included
//   k_mxfp8_gemm     : out = A W^T (+ bias + residual) on v_mfma_scale_f32_16x16x128_f8f6f4, one accumulation chain per output tile
#include "common.h"

namespace {

constexpr int MX_BLOCK = 32;        // elements that share a scale
constexpr int MX_KSTEP = 128;       // K of one scaled MFMA = the granule Kp is padded to

typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------------------------------------------
// quantiser
// ---------------------------------------------------------------------------------------------------------------------------------
template <class T> struct MxSrc;
template <> struct MxSrc<float> { static __device__ __forceinline__ float f(float v) { return v; } };
template <> struct MxSrc<f16> { static __device__ __forceinline__ float f(f16 v) { return (float)v; } };
template <> struct MxSrc<bf16> { static __device__ __forceinline__ float f(bf16 v) { return (float)v; } };

// A thread owns 16 source bytes of a row (4 f32 or 8 16-bit elements); the 8 / 4 neighbouring lanes that hold one 32-element block share their
// amax by __shfl_xor.  Rows of the packed matrix are Kp / EPL threads long, a multiple of the 4 blocks whose scale bytes leave as one dword,
// so a block or a dword of scales never straddles two rows, two waves, or the end of the grid.  VEC: the row starts are 16-byte aligned.
template <class T, bool VEC>
__global__ __launch_bounds__(256) void k_mxfp8_quantize(const T* __restrict__ x, size_t ldx, int R, int K, int Kp, uint8_t* __restrict__ q,
                                                        uint8_t* __restrict__ e) {
    constexpr int EPL = 16 / (int)sizeof(T);          // elements per lane
    constexpr int LPB = MX_BLOCK / EPL;               // lanes per block
    const unsigned cpr = (unsigned)Kp / EPL;          // threads per row
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = idx < (size_t)R * cpr;
    const size_t r = live ? idx / cpr : 0;
    const int col = live ? (int)(idx % cpr) * EPL : 0;

    float v[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) v[j] = 0.f;
    if (live && col < K) {                            // K % 32 == 0: a block lies wholly inside K or wholly in the padding
        const T* src = x + r * ldx + col;
        if constexpr (VEC) {
            const u32x4 raw = *reinterpret_cast<const u32x4*>(src);
            T t[EPL];
            __builtin_memcpy(t, &raw, 16);
#pragma unroll
            for (int j = 0; j < EPL; ++j) v[j] = MxSrc<T>::f(t[j]);
        } else {
#pragma unroll
            for (int j = 0; j < EPL; ++j) v[j] = MxSrc<T>::f(src[j]);
        }
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        v[j] = v[j] == v[j] ? v[j] : 0.f;             // NaN -> 0 (as mve_lo8_scaled)
        amax = fmaxf(amax, fabsf(v[j]));
    }
#pragma unroll
    for (int d = 1; d < LPB; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d));

    // smallest s with amax 2^-s <= 448 = 0.875 * 2^9, on the exponent field alone: amax = 1.f * 2^(E - 127) = m * 2^(E - 126), m = 1.f / 2
    const unsigned bits = __float_as_uint(amax);
    const int E = (int)(bits >> 23), mant = (int)(bits & 0x7fffffu);
    int s = E - 126 - 9 + (mant > 0x600000 ? 1 : 0);  // an f32 subnormal (E = 0) lands below -127 and is clamped like every tiny block
    s = s < -127 ? -127 : s;                          // (s <= 121 for every f32: no upper clamp is ever taken)
    if (amax == 0.f) s = 0;

    float y[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j)                      // v_ldexp_f32: an exponent change, exact wherever the result is not an f32 subnormal (< 2^-126,
        y[j] = __builtin_amdgcn_fmed3f(__builtin_ldexpf(v[j], -s), -448.f, 448.f);      // 2^116 times below e4m3's rounding boundary 2^-10)
    unsigned w[EPL / 4];
#pragma unroll
    for (int g = 0; g < EPL / 4; ++g) {
        int p = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * g], y[4 * g + 1], 0, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * g + 2], y[4 * g + 3], p, true);
        w[g] = (unsigned)p;
    }
    // the four scale bytes of a 128-wide K step as one dword
    const int lane = (int)(threadIdx.x & 63);
    const int base = lane & ~(4 * LPB - 1);
    unsigned sw = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) sw |= (unsigned)__shfl(s + 127, base + LPB * j) << (8 * j);
    if (!live) return;
    uint8_t* dst = q + r * (size_t)Kp + col;
    if constexpr (EPL == 4) *reinterpret_cast<unsigned*>(dst) = w[0];
    else *reinterpret_cast<u32x2*>(dst) = u32x2{w[0], w[1]};
    if (lane == base) *reinterpret_cast<unsigned*>(e + r * (size_t)(Kp / MX_BLOCK) + col / MX_BLOCK) = sw;
}

template <class T>
int launch_quantize(const void* x, int ldx, int R, int K, int Kp, uint8_t* q, uint8_t* e, hipStream_t s) {
    constexpr int EPL = 16 / (int)sizeof(T);
    const size_t threads = (size_t)R * (Kp / EPL);
    const size_t blocks = (threads + 255) / 256;
    MVE_CHECK(blocks < (1ull << 31), MVE_ERR_ARG, "mve_mxfp8_quantize: R=%d x K=%d is too large for one launch", R, K);
    const bool vec = ((uintptr_t)x % 16 == 0) && (((size_t)ldx * sizeof(T)) % 16 == 0);
    if (vec) k_mxfp8_quantize<T, true><<<dim3((unsigned)blocks), 256, 0, s>>>((const T*)x, (size_t)ldx, R, K, Kp, q, e);
    else k_mxfp8_quantize<T, false><<<dim3((unsigned)blocks), 256, 0, s>>>((const T*)x, (size_t)ldx, R, K, Kp, q, e);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------------------------------------------------------------
// Operand lane map of v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands (cbsz = blgp = 0), as measured on exact data: lane l holds row
// l & 15 of its operand; its registers 0-3 are the 16 bytes k = 16 (l >> 4) .. + 15 and its registers 4-7 the 16 bytes k = 64 + 16 (l >> 4) .. + 15
// (the instruction is two K = 64 halves, each spread over the four lane groups) -- NOT the 32 consecutive bytes of one MX block.  The scale of
// MX block b (k = 32 b .. 32 b + 31) of row i is read from bits 7:0 (opsel 0) of the scale register of lane i + 16 b: lane l supplies the E8M0 byte
// of block l >> 4 of its row, whichever lanes hold that block's bytes.  The first operand's rows become D's rows, the second's D's columns,
// D in the standard 16 x 16 map (column = l & 15, row = 4 (l >> 4) + register).  Pinned by tests/test_mxfp8_gpu.py::test_gemm_exact.
//
// The kernel hands W to the instruction as the first operand and A as the second: D's four registers are then four consecutive n of one
// output row m, and the epilogue moves 16 / 8 bytes per lane.
//
// Block: 128 (m) x 128 (n) output tile, 256 threads = 2 x 2 waves of 64 x 64 (4 x 4 MFMA tiles), K in steps of 128, two LDS stages.
// LDS image of an operand tile: [16-row group g (8)][half h (2)][lane l (64)] x 16 bytes = the bytes k = 64 h + 16 (l >> 4) .. + 15 of row
// 16 g + (l & 15).  A fragment is two ds_read_b128 of 1 KiB each that the 64 lanes read back to back: no bank conflict by construction.
// The scale dwords (four E8M0 bytes of the K step) sit behind the tiles, one per row.
constexpr int GT = 128;                                   // tile rows of either operand
constexpr int GT_BYTES = GT * MX_KSTEP;                   // 16 KiB
constexpr int STAGE_BYTES = 2 * GT_BYTES + 2 * GT * 4;    // W tile, A tile, W scales, A scales

struct MxGemmArgs {
    const uint8_t *aq, *ae, *wq, *we;
    int M, N, Kp;
    void* out;
    size_t ldc;
    const float* bias;
    const void* residual;
    size_t ldr;
    int vec_io;                                           // out / residual rows allow 16-byte (f32) / 8-byte (16-bit) accesses
};

template <class TO>
__global__ __launch_bounds__(256) void k_mxfp8_gemm(const MxGemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const unsigned tiles_n = ((unsigned)p.N + GT - 1) / GT;
    const unsigned bid = mve_xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (int)(bid / tiles_n) * GT, n0 = (int)(bid % tiles_n) * GT;
    const int nk = p.Kp / MX_KSTEP;
    const size_t ldq = (size_t)p.Kp;                      // bytes per packed row
    const size_t lde = (size_t)(p.Kp / MX_KSTEP);         // scale dwords per row

    // staging: thread t moves the units u = t and u = t + 256 of each operand tile (unit u = the two 16-byte halves of fragment lane u & 63 of
    // 16-row group u >> 6, 64 bytes apart in the row)
    // and one scale dword (t < 128: W row t, else A row t - 128); rows past the matrix read as zeros with unit scales
    const uint8_t* gsrc[2][2];
    bool gok[2][2];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = tid + 256 * i, row = (u >> 6) * 16 + (u & 15), kb = (u & 63) >> 4;
            const int grow = (o == 0 ? n0 : m0) + row;
            gok[o][i] = grow < (o == 0 ? p.N : p.M);
            gsrc[o][i] = (o == 0 ? p.wq : p.aq) + (size_t)(gok[o][i] ? grow : 0) * ldq + kb * 16;
        }
    const int srow = (tid < GT ? n0 + tid : m0 + tid - GT);
    const bool sok = srow < (tid < GT ? p.N : p.M);
    const unsigned* ssrc = reinterpret_cast<const unsigned*>(tid < GT ? p.we : p.ae) + (size_t)(sok ? srow : 0) * lde;

    u32x4 st[2][2][2];
    unsigned ssc;
    auto load_global = [&](int ks) {
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const u32x4* g = reinterpret_cast<const u32x4*>(gsrc[o][i] + (size_t)ks * MX_KSTEP);
                st[o][i][0] = gok[o][i] ? g[0] : u32x4{0, 0, 0, 0};
                st[o][i][1] = gok[o][i] ? g[4] : u32x4{0, 0, 0, 0};
            }
        ssc = sok ? ssrc[ks] : 0x7f7f7f7fu;
    };
    auto store_lds = [&](int buf) {
        uint8_t* base = smem + buf * STAGE_BYTES;
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int u = tid + 256 * i, g = u >> 6, l = u & 63;
                u32x4* d = reinterpret_cast<u32x4*>(base + o * GT_BYTES + (g * 2 * 64 + l) * 16);
                d[0] = st[o][i][0];
                d[64] = st[o][i][1];
            }
        reinterpret_cast<unsigned*>(base + 2 * GT_BYTES)[tid] = ssc;
    };

    f32x4 acc[4][4];                                      // [n tile j][m tile i]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_global(0);
    store_lds(0);
    __syncthreads();
    const int sshift = 8 * (lane >> 4);
    for (int ks = 0; ks < nk; ++ks) {
        const bool more = ks + 1 < nk;
        if (more) load_global(ks + 1);
        const uint8_t* base = smem + (ks & 1) * STAGE_BYTES;
        const unsigned* sc = reinterpret_cast<const unsigned*>(base + 2 * GT_BYTES);
        i32x8 fa[4];
        int sa[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {                     // the A rows of this wave: second MFMA operand
            const int g = wm * 4 + i;
            const u32x4* f = reinterpret_cast<const u32x4*>(base + GT_BYTES + (g * 2 * 64 + lane) * 16);
            const u32x4 lo = f[0], hi = f[64];
            fa[i] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            sa[i] = (int)((sc[GT + g * 16 + (lane & 15)] >> sshift) & 0xffu);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {                     // the W rows (output columns): first MFMA operand
            const int g = wn * 4 + j;
            const u32x4* f = reinterpret_cast<const u32x4*>(base + (g * 2 * 64 + lane) * 16);
            const u32x4 lo = f[0], hi = f[64];
            const i32x8 fw = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            const int sw = (int)((sc[g * 16 + (lane & 15)] >> sshift) & 0xffu);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[j][i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa[i], acc[j][i], 0, 0, 0, sw, 0, sa[i]);
        }
        if (more) store_lds((ks + 1) & 1);                // last read in step ks - 1, which every wave left at the barrier below
        __syncthreads();
    }

    // epilogue: lane holds out[m][n .. n + 3], m = tile row + (lane & 15), n = tile column + 4 (lane >> 4); N % 8 == 0 keeps a group of 4 whole
    TO* out = (TO*)p.out;
    const TO* res = (const TO*)p.residual;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + i * 16 + (lane & 15);
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
            if (n >= p.N) continue;
            float v[4] = {acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]};
            if (p.bias) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] += b[c];
            }
            if (res) {
                TO rr[4];
                const TO* rp = res + (size_t)m * p.ldr + n;
                if (p.vec_io) __builtin_memcpy(rr, __builtin_assume_aligned(rp, 4 * sizeof(TO)), 4 * sizeof(TO));
                else { rr[0] = rp[0]; rr[1] = rp[1]; rr[2] = rp[2]; rr[3] = rp[3]; }
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] += (float)rr[c];
            }
            TO o[4] = {(TO)v[0], (TO)v[1], (TO)v[2], (TO)v[3]};
            TO* op = out + (size_t)m * p.ldc + n;
            if (p.vec_io) __builtin_memcpy(__builtin_assume_aligned(op, 4 * sizeof(TO)), o, 4 * sizeof(TO));
            else { op[0] = o[0]; op[1] = o[1]; op[2] = o[2]; op[3] = o[3]; }
        }
    }
}

template <class TO>
int launch_gemm(const MxGemmArgs& a, hipStream_t s) {
    const size_t blocks = (size_t)mve_cdiv(a.M, GT) * mve_cdiv(a.N, GT);
    MVE_CHECK(blocks < (1ull << 31), MVE_ERR_ARG, "mve_mxfp8_gemm: M=%d x N=%d is too large for one launch", a.M, a.N);
    return mve_launch_dyn_lds<&k_mxfp8_gemm<TO>>(dim3((unsigned)blocks), 256, 2 * STAGE_BYTES, s, a);      // 66 KiB of dynamic LDS: above the 64 KiB a kernel gets without asking
}

int elem_size(int dtype) { return dtype == MVE_F32 ? 4 : 2; }

}  // namespace

extern "C" {

int mve_mxfp8_packed_k(int K) {
    if (K <= 0 || K % MX_BLOCK != 0) return -1;
    return (K + MX_KSTEP - 1) / MX_KSTEP * MX_KSTEP;
}

int mve_mxfp8_quantize(int dtype, const void* d_x, int ldx, int R, int K, uint8_t* d_q, uint8_t* d_e, void* stream) {
    MVE_CHECK(dtype == MVE_F32 || dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "mve_mxfp8_quantize: dtype=%d must be MVE_F32, MVE_F16 or MVE_BF16",
              dtype);
    MVE_CHECK(K > 0 && K % MX_BLOCK == 0, MVE_ERR_ARG, "mve_mxfp8_quantize: K=%d must be a positive multiple of 32", K);
    MVE_CHECK(R >= 1, MVE_ERR_ARG, "mve_mxfp8_quantize: R=%d must be at least 1", R);
    MVE_CHECK(ldx >= K, MVE_ERR_ARG, "mve_mxfp8_quantize: ldx=%d must be at least K=%d", ldx, K);
    MVE_CHECK(d_x && d_q && d_e, MVE_ERR_ARG, "mve_mxfp8_quantize: d_x, d_q and d_e must not be NULL");
    MVE_CHECK((uintptr_t)d_q % 16 == 0 && (uintptr_t)d_e % 4 == 0, MVE_ERR_ARG, "mve_mxfp8_quantize: d_q must be 16-byte and d_e 4-byte aligned");
    MVE_CHECK((uintptr_t)d_x % (size_t)elem_size(dtype) == 0, MVE_ERR_ARG, "mve_mxfp8_quantize: d_x is not aligned to its element size");
    const int Kp = mve_mxfp8_packed_k(K);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MVE_F32) return launch_quantize<float>(d_x, ldx, R, K, Kp, d_q, d_e, s);
    if (dtype == MVE_F16) return launch_quantize<f16>(d_x, ldx, R, K, Kp, d_q, d_e, s);
    return launch_quantize<bf16>(d_x, ldx, R, K, Kp, d_q, d_e, s);
}

int mve_mxfp8_gemm(const uint8_t* d_aq, const uint8_t* d_ae, const uint8_t* d_wq, const uint8_t* d_we, int M, int N, int K, int out_dtype,
                   void* d_out, int ldc, const float* d_bias, const void* d_residual, int ldr, void* stream) {
    MVE_CHECK(K > 0 && K % MX_BLOCK == 0, MVE_ERR_ARG, "mve_mxfp8_gemm: K=%d must be a positive multiple of 32", K);
    MVE_CHECK(N > 0 && N % 8 == 0, MVE_ERR_ARG, "mve_mxfp8_gemm: N=%d must be a positive multiple of 8", N);
    MVE_CHECK(M >= 1, MVE_ERR_ARG, "mve_mxfp8_gemm: M=%d must be at least 1", M);
    MVE_CHECK(out_dtype == MVE_F32 || out_dtype == MVE_F16 || out_dtype == MVE_BF16, MVE_ERR_ARG,
              "mve_mxfp8_gemm: out_dtype=%d must be MVE_F32, MVE_F16 or MVE_BF16", out_dtype);
    MVE_CHECK(ldc >= N, MVE_ERR_ARG, "mve_mxfp8_gemm: ldc=%d must be at least N=%d", ldc, N);
    MVE_CHECK(!d_residual || ldr >= N, MVE_ERR_ARG, "mve_mxfp8_gemm: ldr=%d must be at least N=%d", ldr, N);
    MVE_CHECK(d_aq && d_ae && d_wq && d_we && d_out, MVE_ERR_ARG, "mve_mxfp8_gemm: d_aq, d_ae, d_wq, d_we and d_out must not be NULL");
    MVE_CHECK((uintptr_t)d_aq % 16 == 0 && (uintptr_t)d_wq % 16 == 0, MVE_ERR_ARG, "mve_mxfp8_gemm: d_aq and d_wq must be 16-byte aligned");
    MVE_CHECK((uintptr_t)d_ae % 4 == 0 && (uintptr_t)d_we % 4 == 0, MVE_ERR_ARG, "mve_mxfp8_gemm: d_ae and d_we must be 4-byte aligned");
    const size_t es = (size_t)elem_size(out_dtype);
    MVE_CHECK((uintptr_t)d_out % es == 0 && (uintptr_t)d_residual % es == 0, MVE_ERR_ARG,
              "mve_mxfp8_gemm: d_out / d_residual are not aligned to the element size of out_dtype");
    MVE_CHECK(!d_bias || (uintptr_t)d_bias % 16 == 0, MVE_ERR_ARG, "mve_mxfp8_gemm: d_bias must be 16-byte aligned");
    MxGemmArgs a;
    a.aq = d_aq; a.ae = d_ae; a.wq = d_wq; a.we = d_we;
    a.M = M; a.N = N; a.Kp = mve_mxfp8_packed_k(K);
    a.out = d_out; a.ldc = (size_t)ldc;
    a.bias = d_bias;
    a.residual = d_residual; a.ldr = (size_t)ldr;
    const size_t vb = 4 * es;                             // bytes of a lane's four outputs
    a.vec_io = (uintptr_t)d_out % vb == 0 && ((size_t)ldc * es) % vb == 0 &&
               (!d_residual || ((uintptr_t)d_residual % vb == 0 && ((size_t)ldr * es) % vb == 0));
    hipStream_t s = (hipStream_t)stream;
    if (out_dtype == MVE_F32) return launch_gemm<float>(a, s);
    if (out_dtype == MVE_F16) return launch_gemm<f16>(a, s);
    return launch_gemm<bf16>(a, s);
}

}  // extern "C"
