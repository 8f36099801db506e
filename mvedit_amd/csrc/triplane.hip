// Tri-plane radiance decoders (gfx950; FMA-bound per-point MLP, gather-bound plane fetches): TriPlaneDecoder.point_decode
// (lib/models/decoders/triplane_decoder.py:135-199) and TriPlaneiNGPDecoder.point_decode (lib/models/decoders/triplane_ingp_decoder.py:
// 142-212), forward.  One wave = 64 points.  The first layer is accumulated feature by feature as the plane fetches (and hash-grid levels)
// produce them -- the 96-wide feature vector never exists; weights are wave-uniform and transposed ([in][out]), so one input's fan-out is
// one contiguous scalar load; the activated hidden vector goes through LDS ([k][lane]: conflict-free) so that the second layer can loop over
// its inputs at run time with all its outputs in registers.  The hash-grid encoding is the one of nerf.hip (hashgrid.h).
// Two topologies (MveTriplaneDesc.topology): the classes' defaults (k_triplane_decode / k_triplane_backward) and the dir-net one of the
// reference's config files (k_triplane_dirnet_decode / k_triplane_dirnet_backward), which keeps the hidden vector in registers throughout.
#include "raymarch_core.h"

#include "hashgrid.h"
#include "sh_core.h"

namespace {

constexpr int WAVE = 64;

struct ShK16 { float k[MVE_SH_MAX_DEGREE * MVE_SH_MAX_DEGREE]; };

struct TriParams {
    const float *xyz, *dirs, *code;
    int N, C, h, w;
    int axes[6];
    int flip_z;
    const float *base_wT, *base_b, *ingp_wT, *ingp_b, *dens_w, *dens_b, *col1_wT, *col1_b, *col2_w, *col2_b;
    const float *dir_wT, *dir_b;          // dir-net topology: [16][H], [H] (col2_* is then its one-Linear colour net, [3][H])
    int activation, sigma_activation;
    float sat;
    float *sigmas, *rgbs;
    DecoderParams hg;         // table / level meta / bound of the hash grid (only .table, .bound, .g are used)
};

__device__ __forceinline__ float act_fn(int a, float x) {
    if (a == 0) return fmaxf(x, 0.f);
    if (a == 1) return x / (1.0f + __expf(-x));
    if (a == 2) return x > 20.f ? x : log1pf(__expf(x));          // torch.nn.Softplus (beta 1, threshold 20)
    return __expf(x);                                              // trunc_exp forward
}

// One plane's bilinear taps of a point: F.grid_sample(align_corners=False, padding_mode='border') -- unnormalise, clip to [0, size - 1]
struct TriTap { int x0, x1, y0, y1; float w[4]; };
__device__ __forceinline__ TriTap tri_tap(const TriParams& p, float u, float v) {
    float fx = ((u + 1.0f) * (float)p.w - 1.0f) * 0.5f, fy = ((v + 1.0f) * (float)p.h - 1.0f) * 0.5f;
    fx = fminf(fmaxf(fx, 0.f), (float)(p.w - 1));
    fy = fminf(fmaxf(fy, 0.f), (float)(p.h - 1));
    const float x0f = floorf(fx), y0f = floorf(fy);
    TriTap t;
    t.x0 = (int)x0f; t.y0 = (int)y0f;
    t.x1 = t.x0 + 1 < p.w ? t.x0 + 1 : p.w - 1; t.y1 = t.y0 + 1 < p.h ? t.y0 + 1 : p.h - 1;     // weight 0 where clipped
    const float tx = fx - x0f, ty = fy - y0f;
    t.w[0] = (1.f - tx) * (1.f - ty); t.w[1] = tx * (1.f - ty); t.w[2] = (1.f - tx) * ty; t.w[3] = tx * ty;
    return t;
}

// base_x, shared by the four kernels: base_b + base_net(plane features) [+ ingp_base_net(hash encoding) + ingp_b], accumulated feature by
// feature.  taps / ws_feat / ws_enc (the backward kernels: this point's taps, and its rows of the feature and encoding workspaces, NULL for
// a lane past N) are optional.
template <int H, int NL>
__device__ __forceinline__ void tri_base_x(const TriParams& p, const float (&x)[3], float (&acc)[H], TriTap* taps = nullptr,
                                           float* ws_feat = nullptr, float* ws_enc = nullptr) {
#pragma unroll
    for (int j = 0; j < H; ++j) acc[j] = p.base_b[j];
    for (int pl = 0; pl < 3; ++pl) {
        const TriTap t = tri_tap(p, x[p.axes[2 * pl]], x[p.axes[2 * pl + 1]]);
        if (taps) taps[pl] = t;
        const float* pc = p.code + (size_t)pl * p.h * p.w * p.C;
        const float* c00 = pc + ((size_t)t.y0 * p.w + t.x0) * p.C;
        const float* c10 = pc + ((size_t)t.y0 * p.w + t.x1) * p.C;
        const float* c01 = pc + ((size_t)t.y1 * p.w + t.x0) * p.C;
        const float* c11 = pc + ((size_t)t.y1 * p.w + t.x1) * p.C;
        for (int c = 0; c < p.C; ++c) {
            // torch's bilinear kernel sums nw, ne, sw, se in this order
            const float f = c00[c] * t.w[0] + c10[c] * t.w[1] + c01[c] * t.w[2] + c11[c] * t.w[3];
            if (ws_feat) ws_feat[c * 3 + pl] = f;
            const float* wr = p.base_wT + (size_t)(c * 3 + pl) * H;
#pragma unroll
            for (int j = 0; j < H; ++j) acc[j] = fmaf(wr[j], f, acc[j]);
        }
    }
    if constexpr (NL > 0) {
        float enc[2 * NL];
        hash_encode<NL>(p.hg, x[0], x[1], p.flip_z ? -x[2] : x[2], enc);          // the hash grid sees the un-flipped point
#pragma unroll
        for (int e = 0; e < 2 * NL; ++e) {
            if (ws_enc) ws_enc[e] = enc[e];
            const float* wr = p.ingp_wT + (size_t)e * H;
#pragma unroll
            for (int j = 0; j < H; ++j) acc[j] = fmaf(wr[j], enc[e], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < H; ++j) acc[j] += p.ingp_b[j];
    }
}

// acc (base_x) += dir_b + dir_net weights . SH_4(direction of point ii); the encoding goes to ws_sh (16 floats) when given.  The 16 SH values
// go through shs (LDS [16][WAVE], each lane reads back its own column: no barrier) so that the loop over them stays a run-time loop like the
// default topology's second layer: fully unrolled (16 x H FMAs on scalar weight loads) the H = 64 kernels spilled ~690 VGPRs to scratch.
template <int H>
__device__ __forceinline__ void tri_add_dir_net(const TriParams& p, const ShK16& kk, int ii, int lane, float* shs, float (&acc)[H], float* ws_sh) {
    {
        float sh[16];
        she_eval(kk.k, p.dirs[3 * ii], p.dirs[3 * ii + 1], p.dirs[3 * ii + 2], 4, sh, nullptr);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            shs[k * WAVE + lane] = sh[k];
            if (ws_sh) ws_sh[k] = sh[k];
        }
    }
#pragma unroll
    for (int j = 0; j < H; ++j) acc[j] += p.dir_b[j];
#pragma unroll 1
    for (int k = 0; k < 16; ++k) {
        const float a = shs[k * WAVE + lane];
        const float* wr = p.dir_wT + (size_t)k * H;
#pragma unroll
        for (int j = 0; j < H; ++j) acc[j] = fmaf(wr[j], a, acc[j]);
    }
}

template <int H, int H2, int NL>
__global__ __launch_bounds__(WAVE) void k_triplane_decode(const TriParams p, const ShK16 kk) {
    __shared__ float hid[(H + 16) * WAVE];            // activated hidden vector + SH encoding, [k][lane]
    const int lane = threadIdx.x;
    const int i = blockIdx.x * WAVE + lane;
    const bool live = i < p.N;
    const int ii = live ? i : p.N - 1;
    const float x[3] = {p.xyz[3 * ii], p.xyz[3 * ii + 1], p.flip_z ? -p.xyz[3 * ii + 2] : p.xyz[3 * ii + 2]};
    float acc[H];
    tri_base_x<H, NL>(p, x, acc);             // plane features (and hash-grid levels), accumulated into the first layer as they come
    // ---- density head; activated hidden vector to LDS ------------------------------------------------------------------------
    float sg = p.dens_b[0];
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const float a = act_fn(p.activation, acc[j]);
        hid[j * WAVE + lane] = a;
        sg = fmaf(p.dens_w[j], a, sg);
    }
    if (live) p.sigmas[i] = act_fn(p.sigma_activation, sg);
    if (p.dirs == nullptr) return;
    {
        float sh[16];
        she_eval(kk.k, p.dirs[3 * ii], p.dirs[3 * ii + 1], p.dirs[3 * ii + 2], 4, sh, nullptr);
#pragma unroll
        for (int k = 0; k < 16; ++k) hid[(H + k) * WAVE + lane] = sh[k];
    }
    // ---- colour net: Linear(H + 16 -> H2), act, Linear(H2 -> 3), sigmoid, saturation -------------------------------------------
    float a2[H2];
#pragma unroll
    for (int j = 0; j < H2; ++j) a2[j] = p.col1_b[j];
    for (int k = 0; k < H + 16; ++k) {
        const float a = hid[k * WAVE + lane];
        const float* wr = p.col1_wT + (size_t)k * H2;
#pragma unroll
        for (int j = 0; j < H2; ++j) a2[j] = fmaf(wr[j], a, a2[j]);
    }
    float o[3] = {p.col2_b[0], p.col2_b[1], p.col2_b[2]};
#pragma unroll
    for (int j = 0; j < H2; ++j) {
        const float a = act_fn(p.activation, a2[j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = fmaf(p.col2_w[c * H2 + j], a, o[c]);
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.rgbs[3 * i + c] = (1.0f / (1.0f + __expf(-o[c]))) * (1.0f + 2.0f * p.sat) - p.sat;
    }
}

// The dir-net topology (dir_layers = [16, H], color_layers = [H, 3]: every config file of the reference): the first layer as above; the density
// head reads act(base_x); the 16 x H dir_net product is added to the PRE-activation accumulator in registers, and the one-Linear colour net
// reads act of that.  There is no second hidden layer to loop over at run time, so the hidden vector is not staged in LDS (only the 16 SH
// values are, see tri_add_dir_net).  The sigma path does not depend
// on p.dirs: the density-only call gives the full call's sigmas bit for bit.
template <int H, int NL>
__global__ __launch_bounds__(WAVE) void k_triplane_dirnet_decode(const TriParams p, const ShK16 kk) {
    __shared__ float shs[16 * WAVE];                  // the SH encoding only, [k][lane] (tri_add_dir_net)
    const int lane = threadIdx.x;
    const int i = blockIdx.x * WAVE + lane;
    const bool live = i < p.N;
    const int ii = live ? i : p.N - 1;
    const float x[3] = {p.xyz[3 * ii], p.xyz[3 * ii + 1], p.flip_z ? -p.xyz[3 * ii + 2] : p.xyz[3 * ii + 2]};
    float acc[H];
    tri_base_x<H, NL>(p, x, acc);
    float sg = p.dens_b[0];
#pragma unroll
    for (int j = 0; j < H; ++j) sg = fmaf(p.dens_w[j], act_fn(p.activation, acc[j]), sg);
    if (live) p.sigmas[i] = act_fn(p.sigma_activation, sg);
    if (p.dirs == nullptr) return;
    tri_add_dir_net<H>(p, kk, ii, lane, shs, acc, nullptr);
    float o[3] = {p.col2_b[0], p.col2_b[1], p.col2_b[2]};
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const float a = act_fn(p.activation, acc[j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = fmaf(p.col2_w[c * H + j], a, o[c]);
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.rgbs[3 * i + c] = (1.0f / (1.0f + __expf(-o[c]))) * (1.0f + 2.0f * p.sat) - p.sat;
    }
}

// ---- fused eval render (VolumeRenderer.forward's eval branch, lib/models/decoders/base_volume_renderer.py:264-329, over a tri-plane scene) ----
// One launch: slab test, occupancy-grid DDA (GridWalker, raymarch_core.h), decode per occupied sample, front-to-back compositing with
// nerf.hip's k_render_rays' arithmetic and stop rule.  One ray per lane, one wave per 64 consecutive rays, weights wave-uniform, no atomics, no
// barrier: a ray's result depends on nothing but the ray.
// What depends on the direction alone is computed ONCE PER RAY and kept in LDS ([j][lane], each lane reads back its own column):
//   dir-net topology   v[j] = dir_b[j] + sum_k dir_wT[k][j] SH_k(d), H values; a sample adds it to base_x: z = base_x + v
//   default topology   v[j] = col1_b[j] + sum_k col1_wT[H + k][j] SH_k(d), H2 values: the start of the first colour layer's accumulator
// so a sample costs no SH evaluation and 16 x H (H2) fewer FMAs than point_decode, and the vector costs no VGPRs next to acc[H].  The sums
// run in another order than k_triplane_(dirnet_)decode's (bias and direction part first), i.e. not bit-identical with point_decode.
// LDS per wave: dir-net H * 256 B (16 / 32 KiB -> 10 / 5 waves per CU of 160 KiB); default (H2 + H) * 256 B (32 / 48 / 64 KiB -> 5 / 3 / 2).
struct TriRender {
    const float *rays_o, *rays_d, *aabb;
    uint32_t N;
    float min_near, T_thresh;
    float *weights_sum, *depth, *image;
    int32_t* n_samples;
};

// pre[j][lane] = b[j] + sum_k wT[k][j] SH_k(d), j < HV.  The 16 SH values are staged in the first 16 rows of pre itself (same lane, program
// order) so that the loop over them stays a run-time loop (see tri_add_dir_net).
template <int HV>
__device__ __forceinline__ void tri_ray_dir_vector(const float* b, const float* wT, const ShK16& kk, const float3p d, int lane, float* pre) {
    {
        float sh[16];
        she_eval(kk.k, d.x, d.y, d.z, 4, sh, nullptr);
#pragma unroll
        for (int k = 0; k < 16; ++k) pre[k * WAVE + lane] = sh[k];
    }
    float v[HV];
#pragma unroll
    for (int j = 0; j < HV; ++j) v[j] = b[j];
#pragma unroll 1
    for (int k = 0; k < 16; ++k) {
        const float a = pre[k * WAVE + lane];
        const float* wr = wT + (size_t)k * HV;
#pragma unroll
        for (int j = 0; j < HV; ++j) v[j] = fmaf(wr[j], a, v[j]);
    }
#pragma unroll
    for (int j = 0; j < HV; ++j) pre[j * WAVE + lane] = v[j];
}

__device__ __forceinline__ float tri_rgb_out(const TriParams& p, float o) { return (1.0f / (1.0f + __expf(-o))) * (1.0f + 2.0f * p.sat) - p.sat; }

// one sample of the dir-net topology: k_triplane_dirnet_decode with the ray's vector in place of tri_add_dir_net
template <int H, int NL>
__device__ __forceinline__ void tri_dirnet_sample(const TriParams& p, const float (&x)[3], const float* pre, int lane, float& sigma, float (&c)[3]) {
    float acc[H];
    tri_base_x<H, NL>(p, x, acc);
    float sg = p.dens_b[0];
#pragma unroll
    for (int j = 0; j < H; ++j) sg = fmaf(p.dens_w[j], act_fn(p.activation, acc[j]), sg);
    sigma = act_fn(p.sigma_activation, sg);
    float o[3] = {p.col2_b[0], p.col2_b[1], p.col2_b[2]};
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const float a = act_fn(p.activation, acc[j] + pre[j * WAVE + lane]);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = fmaf(p.col2_w[k * H + j], a, o[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = tri_rgb_out(p, o[k]);
}

// one sample of the default topology: k_triplane_decode with the first colour layer started from the ray's vector (hid: [H][WAVE])
template <int H, int H2, int NL>
__device__ __forceinline__ void tri_default_sample(const TriParams& p, const float (&x)[3], const float* pre, float* hid, int lane, float& sigma,
                                                   float (&c)[3]) {
    {
        float acc[H];
        tri_base_x<H, NL>(p, x, acc);
        float sg = p.dens_b[0];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float a = act_fn(p.activation, acc[j]);
            hid[j * WAVE + lane] = a;
            sg = fmaf(p.dens_w[j], a, sg);
        }
        sigma = act_fn(p.sigma_activation, sg);
    }
    float a2[H2];
#pragma unroll
    for (int j = 0; j < H2; ++j) a2[j] = pre[j * WAVE + lane];
    for (int k = 0; k < H; ++k) {
        const float a = hid[k * WAVE + lane];
        const float* wr = p.col1_wT + (size_t)k * H2;
#pragma unroll
        for (int j = 0; j < H2; ++j) a2[j] = fmaf(wr[j], a, a2[j]);
    }
    float o[3] = {p.col2_b[0], p.col2_b[1], p.col2_b[2]};
#pragma unroll
    for (int j = 0; j < H2; ++j) {
        const float a = act_fn(p.activation, a2[j]);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = fmaf(p.col2_w[k * H2 + j], a, o[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = tri_rgb_out(p, o[k]);
}

template <int TOPO, int H, int H2, int NL>
__global__ __launch_bounds__(WAVE) void k_triplane_render_rays(const TriParams p, const ShK16 kk, const MarchParams mp, const TriRender r) {
    constexpr bool DIRNET = TOPO == MVE_TRIPLANE_DIRNET;
    constexpr int HV = DIRNET ? H : H2;
    __shared__ float lds[(HV + (DIRNET ? 0 : H)) * WAVE];          // the ray's direction vector [HV][lane] (+ default topology: act(base_x) [H][lane])
    const int lane = threadIdx.x;
    const uint32_t n = blockIdx.x * WAVE + lane;
    if (n >= r.N) return;
    const float3p o = reinterpret_cast<const float3p*>(r.rays_o)[n];
    const float3p d = reinterpret_cast<const float3p*>(r.rays_d)[n];
    float near, far;
    near_far_one(o, d, r.aabb, r.min_near, near, far);
    if (near < far) {                                  // a ray that misses the box takes no sample
        if constexpr (DIRNET) tri_ray_dir_vector<HV>(p.dir_b, p.dir_wT, kk, d, lane, lds);
        else tri_ray_dir_vector<HV>(p.col1_b, p.col1_wT + (size_t)H * H2, kk, d, lane, lds);
    }
    GridWalker w;
    w.init(mp, r.rays_o + 3ull * n, r.rays_d + 3ull * n);
    float ws = 0.f, dep = 0.f, cr = 0.f, cg = 0.f, cb = 0.f;
    float t = near;
    t += w.step_len(t) * 0.0f;                        // eval mode: noise = 0 (as k_render_rays)
    const uint32_t cnt = w.walk(t, far, mp.max_steps, [&](float cx, float cy, float cz, float tn, float dt) {
        const float x[3] = {cx, cy, p.flip_z ? -cz : cz};
        float sigma, c[3];
        if constexpr (DIRNET) tri_dirnet_sample<H, NL>(p, x, lds, lane, sigma, c);
        else tri_default_sample<H, H2, NL>(p, x, lds, lds + HV * WAVE, lane, sigma, c);
        const float alpha = 1.0f - __expf(-sigma * dt);         // kernel_composite_rays, raymarching.cu:877-899
        const float T = 1 - ws;
        const float wgt = alpha * T;
        ws += wgt;
        dep += wgt / tn;
        cr += wgt * c[0];
        cg += wgt * c[1];
        cb += wgt * c[2];
        return !(T < r.T_thresh);
    });
    r.weights_sum[n] = ws;
    r.depth[n] = dep;
    reinterpret_cast<float3p*>(r.image)[n] = float3p{cr, cg, cb};
    if (r.n_samples) r.n_samples[n] = (int32_t)cnt;
}

// d act(x) / dx for the hidden activations and the density head (trunc_exp: lib/ops/activation.py:17-20, g * clamp(exp(x), 1e-6, 1e6))
__device__ __forceinline__ float act_grad(int a, float x) {
    if (a == 0) return x > 0.f ? 1.f : 0.f;
    if (a == 1) { const float s = 1.0f / (1.0f + __expf(-x)); return s * (1.0f + x * (1.0f - s)); }
    if (a == 2) return x > 20.f ? 1.f : 1.0f / (1.0f + __expf(-x));
    return fminf(fmaxf(__expf(x), 1e-6f), 1e6f);
}

// Backward of k_triplane_decode (what autograd supplies when the reference optimises a TriPlane(iNGP)Decoder scene inside nerf_optim,
// lib/pipelines/mvedit_3d_pipeline.py:507-633): gradients of sum(g_sigma * sigma) + sum(g_rgb * rgb) w.r.t. the code planes, the hash table
// and every Linear.  One wave = 64 points, forward recomputed (nothing is saved).  The per-point factors of the weight gradients go to a
// workspace and k_tri_xty reduces them in a fixed order (deterministic); the plane and table gradients are scattered with float atomics, as
// F.grid_sample's and tiny-cuda-nn's backward do.
struct TriBwd {
    const float *g_sigma, *g_rgb;
    float *g_code, *g_table;
    float *ws_feat, *ws_enc, *ws_dbase, *ws_hid, *ws_da2, *ws_act2, *ws_do;      // [N][3C], [N][2NL], [N][H], [N][H+16], [N][H2], [N][H2], [N][4]
};

// The scatter both backward kernels end with, acc holding d base_x of a live point: d feature (c, plane) = base_wT[c * 3 + plane][:] . d base_x
// into the code planes with the bilinear weights, d encoding = ingp_wT . d base_x into the hash table (float atomics)
template <int H, int NL>
__device__ __forceinline__ void tri_scatter(const TriParams& p, const TriBwd& b, const float (&x)[3], const TriTap (&taps)[3], const float (&acc)[H]) {
    if (b.g_code) {
        for (int pl = 0; pl < 3; ++pl) {
            const TriTap& t = taps[pl];
            float* gp = b.g_code + (size_t)pl * p.h * p.w * p.C;
            for (int c = 0; c < p.C; ++c) {
                const float* wr = p.base_wT + (size_t)(c * 3 + pl) * H;
                float g = 0.f;
#pragma unroll
                for (int j = 0; j < H; ++j) g = fmaf(wr[j], acc[j], g);
                atomicAdd(gp + ((size_t)t.y0 * p.w + t.x0) * p.C + c, g * t.w[0]);
                atomicAdd(gp + ((size_t)t.y0 * p.w + t.x1) * p.C + c, g * t.w[1]);
                atomicAdd(gp + ((size_t)t.y1 * p.w + t.x0) * p.C + c, g * t.w[2]);
                atomicAdd(gp + ((size_t)t.y1 * p.w + t.x1) * p.C + c, g * t.w[3]);
            }
        }
    }
    if constexpr (NL > 0) {
        if (b.g_table) {
            float denc[2 * NL];
#pragma unroll
            for (int e = 0; e < 2 * NL; ++e) {
                const float* wr = p.ingp_wT + (size_t)e * H;
                float g = 0.f;
#pragma unroll
                for (int j = 0; j < H; ++j) g = fmaf(wr[j], acc[j], g);
                denc[e] = g;
            }
            hash_scatter<NL>(p.hg, x[0], x[1], p.flip_z ? -x[2] : x[2], denc, b.g_table);
        }
    }
}

template <int H, int H2, int NL>
__global__ __launch_bounds__(WAVE) void k_triplane_backward(const TriParams p, const TriBwd b, const ShK16 kk) {
    __shared__ float hid[(H + 16) * WAVE];
    __shared__ float da2s[H2 * WAVE];
    const int lane = threadIdx.x;
    const int i = blockIdx.x * WAVE + lane;
    const bool live = i < p.N;
    const int ii = live ? i : p.N - 1;
    const float x[3] = {p.xyz[3 * ii], p.xyz[3 * ii + 1], p.flip_z ? -p.xyz[3 * ii + 2] : p.xyz[3 * ii + 2]};
    const int F3 = 3 * p.C;
    float acc[H];
    TriTap taps[3];                           // plane taps of this point: kept for the scatter at the end
    tri_base_x<H, NL>(p, x, acc, taps, live ? b.ws_feat + (size_t)i * F3 : nullptr, live ? b.ws_enc + (size_t)i * (2 * NL) : nullptr);
    float sg = p.dens_b[0];
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const float a = act_fn(p.activation, acc[j]);
        hid[j * WAVE + lane] = a;
        sg = fmaf(p.dens_w[j], a, sg);
    }
    const float d_sg = live ? b.g_sigma[i] * act_grad(p.sigma_activation, sg) : 0.f;
    float d_o[3] = {0.f, 0.f, 0.f};
    const bool colour = p.dirs != nullptr && b.g_rgb != nullptr;
    if (colour) {
        float sh[16];
        she_eval(kk.k, p.dirs[3 * ii], p.dirs[3 * ii + 1], p.dirs[3 * ii + 2], 4, sh, nullptr);
#pragma unroll
        for (int k = 0; k < 16; ++k) hid[(H + k) * WAVE + lane] = sh[k];
        float a2[H2];
#pragma unroll
        for (int j = 0; j < H2; ++j) a2[j] = p.col1_b[j];
        for (int k = 0; k < H + 16; ++k) {
            const float a = hid[k * WAVE + lane];
            const float* wr = p.col1_wT + (size_t)k * H2;
#pragma unroll
            for (int j = 0; j < H2; ++j) a2[j] = fmaf(wr[j], a, a2[j]);
        }
        float o[3] = {p.col2_b[0], p.col2_b[1], p.col2_b[2]};
#pragma unroll
        for (int j = 0; j < H2; ++j) {
            const float a = act_fn(p.activation, a2[j]);
            if (live) b.ws_act2[(size_t)i * H2 + j] = a;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = fmaf(p.col2_w[c * H2 + j], a, o[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float s = 1.0f / (1.0f + __expf(-o[c]));
            d_o[c] = live ? b.g_rgb[3 * (size_t)i + c] * (1.0f + 2.0f * p.sat) * s * (1.0f - s) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < H2; ++j) {
            float g = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) g = fmaf(p.col2_w[c * H2 + j], d_o[c], g);
            g *= act_grad(p.activation, a2[j]);
            da2s[j * WAVE + lane] = g;
            if (live) b.ws_da2[(size_t)i * H2 + j] = g;
        }
    }
    if (live) {
        reinterpret_cast<f32x4*>(b.ws_do)[i] = f32x4{d_o[0], d_o[1], d_o[2], d_sg};
        for (int k = 0; k < H + 16; ++k) b.ws_hid[(size_t)i * (H + 16) + k] = (k < H || colour) ? hid[k * WAVE + lane] : 0.f;
    }
    // d base_x[k] = (dens_w[k] d_sg + sum_j col1_wT[k][j] d_a2[j]) * act'(base_x[k]); acc becomes d base_x
#pragma unroll
    for (int k = 0; k < H; ++k) {
        float g = p.dens_w[k] * d_sg;
        if (colour) {
            const float* wr = p.col1_wT + (size_t)k * H2;
            for (int j = 0; j < H2; ++j) g = fmaf(wr[j], da2s[j * WAVE + lane], g);
        }
        g *= act_grad(p.activation, acc[k]);
        acc[k] = g;
        if (live) b.ws_dbase[(size_t)i * H + k] = g;
    }
    if (!live) return;
    tri_scatter<H, NL>(p, b, x, taps, acc);
}

// Backward of k_triplane_dirnet_decode, in the design of k_triplane_backward: forward recomputed, per-point factors to the workspace.  The
// sections are the default topology's under other names: ws_hid [N][H + 16] holds act(base_x) | SH, ws_da2 [N][H] holds d z (z = base_x +
// dir_net(SH), the colour net's pre-activation), ws_act2 [N][H] holds act(z).  d base_x = dens_w d_sg act'(base_x) + d z.
template <int H, int NL>
__global__ __launch_bounds__(WAVE) void k_triplane_dirnet_backward(const TriParams p, const TriBwd b, const ShK16 kk) {
    __shared__ float shs[16 * WAVE];
    const int lane = threadIdx.x;
    const int i = blockIdx.x * WAVE + lane;
    const bool live = i < p.N;
    const int ii = live ? i : p.N - 1;
    const float x[3] = {p.xyz[3 * ii], p.xyz[3 * ii + 1], p.flip_z ? -p.xyz[3 * ii + 2] : p.xyz[3 * ii + 2]};
    const int F3 = 3 * p.C;
    float acc[H], gb[H];                      // base_x, then z, then d base_x; the density head's part of d base_x
    TriTap taps[3];
    tri_base_x<H, NL>(p, x, acc, taps, live ? b.ws_feat + (size_t)i * F3 : nullptr, live ? b.ws_enc + (size_t)i * (2 * NL) : nullptr);
    float* hid = live ? b.ws_hid + (size_t)i * (H + 16) : nullptr;
    float sg = p.dens_b[0];
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const float a = act_fn(p.activation, acc[j]);
        if (live) hid[j] = a;
        sg = fmaf(p.dens_w[j], a, sg);
    }
    const float d_sg = live ? b.g_sigma[i] * act_grad(p.sigma_activation, sg) : 0.f;
#pragma unroll
    for (int j = 0; j < H; ++j) gb[j] = p.dens_w[j] * d_sg * act_grad(p.activation, acc[j]);
    float d_o[3] = {0.f, 0.f, 0.f};
    const bool colour = p.dirs != nullptr && b.g_rgb != nullptr;
    if (colour) {
        tri_add_dir_net<H>(p, kk, ii, lane, shs, acc, live ? hid + H : nullptr);
        float o[3] = {p.col2_b[0], p.col2_b[1], p.col2_b[2]};
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float a = act_fn(p.activation, acc[j]);
            if (live) b.ws_act2[(size_t)i * H + j] = a;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = fmaf(p.col2_w[c * H + j], a, o[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float s = 1.0f / (1.0f + __expf(-o[c]));
            d_o[c] = live ? b.g_rgb[3 * (size_t)i + c] * (1.0f + 2.0f * p.sat) * s * (1.0f - s) : 0.f;
        }
    }
    if (live) reinterpret_cast<f32x4*>(b.ws_do)[i] = f32x4{d_o[0], d_o[1], d_o[2], d_sg};
#pragma unroll
    for (int j = 0; j < H; ++j) {
        float g = gb[j];
        if (colour) {
            float dz = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) dz = fmaf(p.col2_w[c * H + j], d_o[c], dz);
            dz *= act_grad(p.activation, acc[j]);
            if (live) b.ws_da2[(size_t)i * H + j] = dz;
            g += dz;
        }
        acc[j] = g;
        if (live) b.ws_dbase[(size_t)i * H + j] = g;
    }
    if (!live) return;
    // the scatter reads base_wT / ingp_wT a second time; the fence keeps those loads from being merged with (or hoisted into) the first pass.
    // OPEN: H = 64 with a hash branch still spills (NL = 12: 1255 VGPRs, 5 KB of scratch per lane; none at H = 64 without one, 200-380 VGPRs at H = 128)
    asm volatile("" ::: "memory");
    tri_scatter<H, NL>(p, b, x, taps, acc);
}

// out[pi][qi] = sum_m X[m][pi] Y[m][qi] and colsum[pi] = sum_m X[m][pi], for column windows of two row-major workspaces (leading dimensions
// ldx, ldy): per-block partials over 1024-row chunks, folded in block order by k_tri_xty_reduce -- deterministic.  P <= 64, Q <= 64, P * Q <= 2048.
constexpr int TXR = 1024, TXS = 32;
__global__ __launch_bounds__(256) void k_tri_xty(const float* __restrict__ X, int ldx, int P, const float* __restrict__ Y, int ldy, int Q, int M,
                                                 float* __restrict__ partial /*[nblk][P*Q + P]*/) {
    __shared__ float xs[TXS][64], ys[TXS][64];
    const int r0 = blockIdx.x * TXR, r1 = min(M, r0 + TXR);
    const int nout = P * Q;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float cs = 0.f;
    for (int r = r0; r < r1; r += TXS) {
        for (int t = threadIdx.x; t < TXS * P; t += 256) { const int rr = t / P, c = t - rr * P; xs[rr][c] = (r + rr < r1) ? X[(size_t)(r + rr) * ldx + c] : 0.f; }
        for (int t = threadIdx.x; t < TXS * Q; t += 256) { const int rr = t / Q, c = t - rr * Q; ys[rr][c] = (r + rr < r1) ? Y[(size_t)(r + rr) * ldy + c] : 0.f; }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int oi = threadIdx.x + 256 * k;
            if (oi < nout) {
                const int pi = oi / Q, qi = oi - pi * Q;
                float a = acc[k];
                for (int rr = 0; rr < TXS; ++rr) a = fmaf(xs[rr][pi], ys[rr][qi], a);
                acc[k] = a;
            }
        }
        if ((int)threadIdx.x < P) for (int rr = 0; rr < TXS; ++rr) cs += xs[rr][threadIdx.x];
        __syncthreads();
    }
    float* out = partial + (size_t)blockIdx.x * (nout + P);
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int oi = threadIdx.x + 256 * k; if (oi < nout) out[oi] = acc[k]; }
    if ((int)threadIdx.x < P) out[nout + threadIdx.x] = cs;
}
// out_mat[pi * ldo + qi] (a [P][Q] window of a row-major matrix), out_col[pi]
__global__ __launch_bounds__(256) void k_tri_xty_reduce(const float* __restrict__ partial, int nblk, int P, int Q, float* __restrict__ out_mat, int ldo,
                                                        float* __restrict__ out_col) {
    const int t = blockIdx.x * 256 + threadIdx.x, n = P * Q + P;
    if (t >= n) return;
    float a = 0.f;
    for (int bb = 0; bb < nblk; ++bb) a += partial[(size_t)bb * n + t];
    if (t < P * Q) { const int pi = t / Q, qi = t - pi * Q; out_mat[(size_t)pi * ldo + qi] = a; }
    else if (out_col) out_col[t - P * Q] = a;
}

// G [P][Q] (leading dimension ldo) = X^T Y over M rows, in column windows that fit the reduction kernel; colsum(X) once
int tri_xty(const float* X, int ldx, int P, const float* Y, int ldy, int Q, int M, float* G, int ldo, float* colsum, float* partial, hipStream_t s) {
    const int nblk = (M + TXR - 1) / TXR;
    for (int p0 = 0; p0 < P; p0 += 64) {
        const int pc = P - p0 < 64 ? P - p0 : 64;
        const int qstep = 2048 / pc < 64 ? 2048 / pc : 64;
        for (int q0 = 0; q0 < Q; q0 += qstep) {
            const int qc = Q - q0 < qstep ? Q - q0 : qstep;
            k_tri_xty<<<nblk, 256, 0, s>>>(X + p0, ldx, pc, Y + q0, ldy, qc, M, partial);
            MVE_LAUNCH_CHECK();
            k_tri_xty_reduce<<<mve_cdiv(pc * qc + pc, 256), 256, 0, s>>>(partial, nblk, pc, qc, G + (size_t)p0 * ldo + q0, ldo,
                                                                      (q0 == 0 && colsum) ? colsum + p0 : nullptr);
            MVE_LAUNCH_CHECK();
        }
    }
    return MVE_OK;
}

template <int H, int H2>
int launch_bwd_nl(const TriParams& p, const TriBwd& b, const ShK16& kk, int n_levels, hipStream_t s) {
    const unsigned grid = mve_cdiv((unsigned)p.N, WAVE);
    switch (n_levels) {
        case 0: k_triplane_backward<H, H2, 0><<<grid, WAVE, 0, s>>>(p, b, kk); break;
        case 12: k_triplane_backward<H, H2, 12><<<grid, WAVE, 0, s>>>(p, b, kk); break;
        case 14: k_triplane_backward<H, H2, 14><<<grid, WAVE, 0, s>>>(p, b, kk); break;
        case 16: k_triplane_backward<H, H2, 16><<<grid, WAVE, 0, s>>>(p, b, kk); break;
        default: mve_set_error("triplane_backward: n_levels must be 0 (no hash grid), 12, 14 or 16 (got %d)", n_levels); return MVE_ERR_ARG;
    }
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

template <int H, int H2>
int launch_nl(const TriParams& p, const ShK16& kk, int n_levels, hipStream_t s) {
    const unsigned grid = mve_cdiv((unsigned)p.N, WAVE);
    switch (n_levels) {
        case 0: k_triplane_decode<H, H2, 0><<<grid, WAVE, 0, s>>>(p, kk); break;
        case 12: k_triplane_decode<H, H2, 12><<<grid, WAVE, 0, s>>>(p, kk); break;
        case 14: k_triplane_decode<H, H2, 14><<<grid, WAVE, 0, s>>>(p, kk); break;
        case 16: k_triplane_decode<H, H2, 16><<<grid, WAVE, 0, s>>>(p, kk); break;
        default: mve_set_error("triplane_decode: n_levels must be 0 (no hash grid), 12, 14 or 16 (got %d)", n_levels); return MVE_ERR_ARG;
    }
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

template <int H>
int launch_dirnet_nl(const TriParams& p, const ShK16& kk, int n_levels, hipStream_t s) {
    const unsigned grid = mve_cdiv((unsigned)p.N, WAVE);
    switch (n_levels) {
        case 0: k_triplane_dirnet_decode<H, 0><<<grid, WAVE, 0, s>>>(p, kk); break;
        case 12: k_triplane_dirnet_decode<H, 12><<<grid, WAVE, 0, s>>>(p, kk); break;
        case 14: k_triplane_dirnet_decode<H, 14><<<grid, WAVE, 0, s>>>(p, kk); break;
        case 16: k_triplane_dirnet_decode<H, 16><<<grid, WAVE, 0, s>>>(p, kk); break;
        default: mve_set_error("triplane_decode: n_levels must be 0 (no hash grid), 12, 14 or 16 (got %d)", n_levels); return MVE_ERR_ARG;
    }
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

template <int H>
int launch_dirnet_bwd_nl(const TriParams& p, const TriBwd& b, const ShK16& kk, int n_levels, hipStream_t s) {
    const unsigned grid = mve_cdiv((unsigned)p.N, WAVE);
    switch (n_levels) {
        case 0: k_triplane_dirnet_backward<H, 0><<<grid, WAVE, 0, s>>>(p, b, kk); break;
        case 12: k_triplane_dirnet_backward<H, 12><<<grid, WAVE, 0, s>>>(p, b, kk); break;
        case 14: k_triplane_dirnet_backward<H, 14><<<grid, WAVE, 0, s>>>(p, b, kk); break;
        case 16: k_triplane_dirnet_backward<H, 16><<<grid, WAVE, 0, s>>>(p, b, kk); break;
        default: mve_set_error("triplane_backward: n_levels must be 0 (no hash grid), 12, 14 or 16 (got %d)", n_levels); return MVE_ERR_ARG;
    }
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // namespace

namespace {

// validation shared by the forward and the backward; fills p, returns the number of hash-grid levels through *nl_out
// (render: the fused ray-march render brings its own sample points and directions -- d_xyz, d_dirs, N, d_sigmas and d_rgbs are not read, the
// colour net is always needed)
int fill_tri(const char* who, const MveTriplaneDesc* d, TriParams& p, int* nl_out, bool render = false) {
    MVE_CHECK((render || d->d_xyz) && d->d_code && d->d_base_wT && d->d_base_b && d->d_dens_w && d->d_dens_b, MVE_ERR_ARG, "%s: null pointer", who);
    MVE_CHECK((render || d->N > 0) && d->C > 0 && d->h > 0 && d->w > 0, MVE_ERR_ARG, "%s: bad sizes N=%d C=%d h=%d w=%d", who, d->N, d->C, d->h, d->w);
    MVE_CHECK(d->topology == MVE_TRIPLANE_DEFAULT || d->topology == MVE_TRIPLANE_DIRNET, MVE_ERR_ARG, "%s: unknown topology %d", who, d->topology);
    const bool dirnet = d->topology == MVE_TRIPLANE_DIRNET;
    if (dirnet) {            // hidden2 is not read
        MVE_CHECK(d->hidden == 64 || d->hidden == 128, MVE_ERR_ARG, "%s: the hidden width must be 64 or 128 (got %d)", who, d->hidden);
        MVE_CHECK(d->d_dir_wT && d->d_dir_b, MVE_ERR_ARG, "%s: the dir-net topology needs d_dir_wT and d_dir_b", who);
    } else {
        MVE_CHECK((d->hidden == 64 || d->hidden == 128) && (d->hidden2 == 64 || d->hidden2 == 128), MVE_ERR_ARG,
                  "%s: hidden widths must be 64 or 128 (got %d, %d)", who, d->hidden, d->hidden2);
        MVE_CHECK(!d->d_dir_wT && !d->d_dir_b, MVE_ERR_ARG, "%s: dir_net pointers given with the default topology (set topology = MVE_TRIPLANE_DIRNET)", who);
    }
    MVE_CHECK(d->activation >= 0 && d->activation <= 2 && d->sigma_activation >= 0 && d->sigma_activation <= 3, MVE_ERR_ARG, "%s: bad activation code", who);
    for (int k = 0; k < 6; ++k) MVE_CHECK(d->axes[k] >= 0 && d->axes[k] < 3, MVE_ERR_ARG, "%s: bad plane axis %d", who, d->axes[k]);
    if (d->d_dirs || render) MVE_CHECK((dirnet || (d->d_col1_wT && d->d_col1_b)) && d->d_col2_w && d->d_col2_b, MVE_ERR_ARG, "%s: null colour-net pointer", who);
    memset(&p, 0, sizeof(p));
    if (!render) { p.xyz = d->d_xyz; p.dirs = d->d_dirs; p.N = d->N; p.sigmas = d->d_sigmas; p.rgbs = d->d_rgbs; }
    p.code = d->d_code; p.C = d->C; p.h = d->h; p.w = d->w;
    for (int k = 0; k < 6; ++k) p.axes[k] = d->axes[k];
    p.flip_z = d->flip_z;
    p.base_wT = d->d_base_wT; p.base_b = d->d_base_b; p.ingp_wT = d->d_ingp_wT; p.ingp_b = d->d_ingp_b;
    p.dens_w = d->d_dens_w; p.dens_b = d->d_dens_b; p.col1_wT = d->d_col1_wT; p.col1_b = d->d_col1_b; p.col2_w = d->d_col2_w; p.col2_b = d->d_col2_b;
    p.dir_wT = d->d_dir_wT; p.dir_b = d->d_dir_b;
    p.activation = d->activation; p.sigma_activation = d->sigma_activation; p.sat = d->sigmoid_saturation;
    int nl = 0;
    if (d->d_ingp_wT) {
        nl = d->n_levels;
        MVE_CHECK(d->d_ingp_b && d->d_table && d->level_scale && d->level_res && d->level_offset && d->level_size && nl > 0 && nl <= MAX_LEVELS, MVE_ERR_ARG,
                  "%s: incomplete hash-grid description", who);
        p.hg.table = d->d_table; p.hg.bound = d->bound; p.hg.g.n_levels = nl;
        for (int l = 0; l < nl; ++l) { p.hg.g.scale[l] = d->level_scale[l]; p.hg.g.res[l] = d->level_res[l]; p.hg.g.off[l] = d->level_offset[l]; p.hg.g.size[l] = d->level_size[l]; }
    }
    *nl_out = nl;
    return MVE_OK;
}

size_t tri_ws_floats(size_t N, int C, int H, int H2, int nl) {
    const size_t nblk = (N + TXR - 1) / TXR;
    return N * (size_t)(3 * C + 2 * nl + H + (H + 16) + H2 + H2 + 4) + nblk * (size_t)(2048 + 64) + 64;
}

}  // namespace

extern "C" int mve_triplane_decode(const MveTriplaneDesc* d, void* stream) {
    MVE_CHECK(d, MVE_ERR_ARG, "triplane_decode: null descriptor");
    if (d->N == 0) return MVE_OK;
    TriParams p;
    int nl = 0;
    if (int rc = fill_tri("triplane_decode", d, p, &nl)) return rc;
    MVE_CHECK(d->d_sigmas && (!d->d_dirs || d->d_rgbs), MVE_ERR_ARG, "triplane_decode: null output pointer");
    ShK16 kk;
    she_constants(kk.k);
    hipStream_t s = (hipStream_t)stream;
    if (d->topology == MVE_TRIPLANE_DIRNET) return d->hidden == 128 ? launch_dirnet_nl<128>(p, kk, nl, s) : launch_dirnet_nl<64>(p, kk, nl, s);
    if (d->hidden == 128 && d->hidden2 == 128) return launch_nl<128, 128>(p, kk, nl, s);
    if (d->hidden == 128 && d->hidden2 == 64) return launch_nl<128, 64>(p, kk, nl, s);
    if (d->hidden == 64 && d->hidden2 == 128) return launch_nl<64, 128>(p, kk, nl, s);
    return launch_nl<64, 64>(p, kk, nl, s);
}

extern "C" size_t mve_triplane_backward_workspace_bytes(int N, int C, int hidden, int hidden2, int n_levels) {
    return sizeof(float) * tri_ws_floats((size_t)(N > 0 ? N : 0), C, hidden, hidden2, n_levels);
}

// the dir-net topology's sections are the default's with hidden2 = hidden (k_triplane_dirnet_backward)
extern "C" size_t mve_triplane_dirnet_backward_workspace_bytes(int N, int C, int hidden, int n_levels) {
    return sizeof(float) * tri_ws_floats((size_t)(N > 0 ? N : 0), C, hidden, hidden, n_levels);
}

extern "C" int mve_triplane_backward(const MveTriplaneDesc* d, const float* d_grad_sigmas, const float* d_grad_rgbs, const MveTriplaneGrads* g,
                                     void* d_workspace, size_t workspace_bytes, void* stream) {
    MVE_CHECK(d && g, MVE_ERR_ARG, "triplane_backward: null descriptor");
    MVE_CHECK(g->d_base_w && g->d_base_b && g->d_dens_w && g->d_dens_b, MVE_ERR_ARG, "triplane_backward: null gradient output");
    hipStream_t s = (hipStream_t)stream;
    const bool dirnet = d->topology == MVE_TRIPLANE_DIRNET;
    const int H = d->hidden, H2 = dirnet ? d->hidden : d->hidden2, F3 = 3 * d->C;
    const bool colour = d->d_dirs != nullptr && d_grad_rgbs != nullptr;
    if (colour && dirnet) MVE_CHECK(g->d_dir_w && g->d_dir_b && g->d_col2_w && g->d_col2_b, MVE_ERR_ARG, "triplane_backward: null dir-net / colour-net gradient output");
    if (colour && !dirnet) MVE_CHECK(g->d_col1_w && g->d_col1_b && g->d_col2_w && g->d_col2_b, MVE_ERR_ARG, "triplane_backward: null colour-net gradient output");
    if (d->N == 0) return MVE_OK;
    TriParams p;
    int nl = 0;
    if (int rc = fill_tri("triplane_backward", d, p, &nl)) return rc;
    if (nl) MVE_CHECK(g->d_ingp_w && g->d_ingp_b, MVE_ERR_ARG, "triplane_backward: null hash-branch gradient output");
    MVE_CHECK(d_grad_sigmas && d_workspace, MVE_ERR_ARG, "triplane_backward: null pointer");
    MVE_CHECK(workspace_bytes >= mve_triplane_backward_workspace_bytes(d->N, d->C, H, H2, nl), MVE_ERR_NOMEM, "triplane_backward: workspace too small");      // (dir-net: H2 = H)
    const size_t N = (size_t)d->N;
    float* ws = (float*)d_workspace;
    TriBwd b;
    b.g_sigma = d_grad_sigmas; b.g_rgb = colour ? d_grad_rgbs : nullptr;
    b.g_code = g->d_code; b.g_table = nl ? g->d_table : nullptr;
    MVE_CHECK(((uintptr_t)d_workspace & 15) == 0, MVE_ERR_ARG, "triplane_backward: the workspace must be 16-byte aligned");
    b.ws_do = ws; ws += N * 4;            // first: it is written as f32x4 (16-byte stores) -- behind N * (3C + ...) floats it was only 8-byte aligned for odd N, C = 6
    b.ws_feat = ws; ws += N * F3;
    b.ws_enc = ws; ws += N * 2 * nl;
    b.ws_dbase = ws; ws += N * H;
    b.ws_hid = ws; ws += N * (H + 16);
    b.ws_da2 = ws; ws += N * H2;
    b.ws_act2 = ws; ws += N * H2;
    ws = (float*)(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    float* partial = ws;
    if (!colour) p.dirs = nullptr;
    ShK16 kk;
    she_constants(kk.k);
    int rc;
    if (dirnet) rc = H == 128 ? launch_dirnet_bwd_nl<128>(p, b, kk, nl, s) : launch_dirnet_bwd_nl<64>(p, b, kk, nl, s);
    else if (H == 128 && H2 == 128) rc = launch_bwd_nl<128, 128>(p, b, kk, nl, s);
    else if (H == 128 && H2 == 64) rc = launch_bwd_nl<128, 64>(p, b, kk, nl, s);
    else if (H == 64 && H2 == 128) rc = launch_bwd_nl<64, 128>(p, b, kk, nl, s);
    else rc = launch_bwd_nl<64, 64>(p, b, kk, nl, s);
    if (rc) return rc;
    const int M = d->N;
    // torch layouts: base_net.0.weight [H][3C] = d base^T feat, bias = colsum(d base); ingp likewise; density_net.0.weight [1][H] = d_sg^T act(base)
    if ((rc = tri_xty(b.ws_dbase, H, H, b.ws_feat, F3, F3, M, g->d_base_w, F3, g->d_base_b, partial, s))) return rc;
    if (nl) {
        if ((rc = tri_xty(b.ws_dbase, H, H, b.ws_enc, 2 * nl, 2 * nl, M, g->d_ingp_w, 2 * nl, g->d_ingp_b, partial, s))) return rc;
    }
    if ((rc = tri_xty(b.ws_do + 3, 4, 1, b.ws_hid, H + 16, H, M, g->d_dens_w, H, g->d_dens_b, partial, s))) return rc;
    if (colour && dirnet) {
        // dir_net.0.weight [H][16] = d z^T SH, bias = colsum(d z); color_net.0.weight [3][H] = d o^T act(z)
        if ((rc = tri_xty(b.ws_da2, H, H, b.ws_hid + H, H + 16, 16, M, g->d_dir_w, 16, g->d_dir_b, partial, s))) return rc;
        if ((rc = tri_xty(b.ws_do, 4, 3, b.ws_act2, H, H, M, g->d_col2_w, H, g->d_col2_b, partial, s))) return rc;
    } else if (colour) {
        if ((rc = tri_xty(b.ws_da2, H2, H2, b.ws_hid, H + 16, H + 16, M, g->d_col1_w, H + 16, g->d_col1_b, partial, s))) return rc;
        if ((rc = tri_xty(b.ws_do, 4, 3, b.ws_act2, H2, H2, M, g->d_col2_w, H2, g->d_col2_b, partial, s))) return rc;
    }
    return MVE_OK;
}

namespace {

template <int TOPO, int H, int H2>
int launch_render_nl(const TriParams& p, const ShK16& kk, const MarchParams& mp, const TriRender& r, int n_levels, hipStream_t s) {
    const unsigned grid = mve_cdiv(r.N, (uint32_t)WAVE);
    switch (n_levels) {
        case 0: k_triplane_render_rays<TOPO, H, H2, 0><<<grid, WAVE, 0, s>>>(p, kk, mp, r); break;
        case 12: k_triplane_render_rays<TOPO, H, H2, 12><<<grid, WAVE, 0, s>>>(p, kk, mp, r); break;
        case 14: k_triplane_render_rays<TOPO, H, H2, 14><<<grid, WAVE, 0, s>>>(p, kk, mp, r); break;
        case 16: k_triplane_render_rays<TOPO, H, H2, 16><<<grid, WAVE, 0, s>>>(p, kk, mp, r); break;
        default: return MVE_ERR_ARG;          // (checked by the caller before any launch)
    }
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // namespace

extern "C" int mve_triplane_render_rays(const MveTriplaneDesc* d, const float* d_rays_o, const float* d_rays_d, uint32_t N, const uint8_t* d_bitfield,
                                        uint32_t grid_size, const float* d_aabb, float min_near, float dt_gamma, uint32_t max_steps, float T_thresh,
                                        float* d_weights_sum, float* d_depth, float* d_image, int32_t* d_n_samples, void* stream) {
    if (N == 0) return MVE_OK;
    MVE_CHECK(d, MVE_ERR_ARG, "triplane_render_rays: null descriptor");
    MVE_CHECK(d_rays_o && d_rays_d && d_bitfield && d_aabb && d_weights_sum && d_depth && d_image, MVE_ERR_ARG, "triplane_render_rays: null pointer");
    MVE_CHECK(grid_size > 0 && grid_size <= 1024 && max_steps > 0, MVE_ERR_ARG, "triplane_render_rays: bad grid (grid_size %u, max_steps %u)", grid_size, max_steps);
    MVE_CHECK(d->bound > 0.f, MVE_ERR_ARG, "triplane_render_rays: the descriptor's bound must be positive (got %g)", (double)d->bound);
    TriParams p;
    int nl = 0;
    if (int rc = fill_tri("triplane_render_rays", d, p, &nl, true)) return rc;
    MVE_CHECK(nl == 0 || nl == 12 || nl == 14 || nl == 16, MVE_ERR_ARG, "triplane_render_rays: n_levels must be 0 (no hash grid), 12, 14 or 16 (got %d)", nl);
    MarchParams mp;
    mp.grid = d_bitfield; mp.bound = d->bound; mp.contract = 0; mp.dt_gamma = dt_gamma; mp.max_steps = max_steps; mp.C = 1; mp.H = grid_size;
    TriRender r;
    r.rays_o = d_rays_o; r.rays_d = d_rays_d; r.aabb = d_aabb; r.N = N; r.min_near = min_near; r.T_thresh = T_thresh;
    r.weights_sum = d_weights_sum; r.depth = d_depth; r.image = d_image; r.n_samples = d_n_samples;
    ShK16 kk;
    she_constants(kk.k);
    hipStream_t s = (hipStream_t)stream;
    if (d->topology == MVE_TRIPLANE_DIRNET)
        return d->hidden == 128 ? launch_render_nl<MVE_TRIPLANE_DIRNET, 128, 128>(p, kk, mp, r, nl, s) : launch_render_nl<MVE_TRIPLANE_DIRNET, 64, 64>(p, kk, mp, r, nl, s);
    if (d->hidden == 128 && d->hidden2 == 128) return launch_render_nl<MVE_TRIPLANE_DEFAULT, 128, 128>(p, kk, mp, r, nl, s);
    if (d->hidden == 128 && d->hidden2 == 64) return launch_render_nl<MVE_TRIPLANE_DEFAULT, 128, 64>(p, kk, mp, r, nl, s);
    if (d->hidden == 64 && d->hidden2 == 128) return launch_render_nl<MVE_TRIPLANE_DEFAULT, 64, 128>(p, kk, mp, r, nl, s);
    return launch_render_nl<MVE_TRIPLANE_DEFAULT, 64, 64>(p, kk, mp, r, nl, s);
}
