// Triangle rasteriser + attribute interpolation for gfx950, with the output convention of nvdiffrast's dr.rasterize /
// dr.interpolate as the reference consumes it (lib/models/decoders/mesh_renderer/base_mesh_renderer.py:240-252:
// rast = [u, v, z/w, triangle_id + 1], foreground <=> rast[..., 3] > 0).
//
// nvdiffrast (requirements.txt:3) is third-party and not available: the coverage, snapping and tie rules implemented here are
// the ones SPECIFIED in oracle/raster_oracle.c, reproduced bit-for-bit (exact int64 edge functions on 1/256-pixel snapped
// vertices, float32 barycentrics with the same operation order, -ffp-contract=off).
//
// Design: meshes on this path are dense (1e4..1e5 faces, a few pixels each), so visibility is resolved with one 64-bit
// atomicMin per covered sample on a packed (order-preserving depth bits << 32 | triangle id) buffer:
//   pass 1  one thread per (view, triangle): set-up, bounding box, and for small boxes the pixel loop itself; triangles
//           whose box exceeds 1024 pixels are queued and swept by a whole block each (pass 1b);
//   pass 2  one thread per pixel decodes the winner and recomputes its barycentrics -> (u, v, z/w, id+1).
// min() is order independent and ties on depth fall to the lower triangle id, so the image is deterministic although the
// atomics race.  The depth/id buffer (8 B/pixel) lives in L2 / Infinity Cache for the 512^2 x 6 view batches of the pipeline.
#include "common.h"

#include "mesh_capacity_core.h"

namespace {

constexpr int RB = 256;
constexpr int SMALL_BOX = 1024;     // pixels

struct TriSetup {
    long long X[3], Y[3];
    float zw[3], iw[3];
    long long sgn;
    int own[3];
    int px0, px1, py0, py1;
    bool valid;
};

__device__ __forceinline__ long long edge_fn(long long ax, long long ay, long long bx, long long by, long long px, long long py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
__device__ __forceinline__ int edge_owns_tie(long long ax, long long ay, long long bx, long long by) {
    const long long dx = bx - ax, dy = by - ay;
    return (dy > 0) || (dy == 0 && dx < 0);
}

__device__ __forceinline__ void tri_setup(const float* __restrict__ P, int V, const int32_t* __restrict__ tri, int f, int H, int W,
                                          TriSetup& t) {
    t.valid = false;
    const int i0 = tri[3 * f], i1 = tri[3 * f + 1], i2 = tri[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return;
    const int idx[3] = {i0, i1, i2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(P + 4ll * idx[k]);
        if (v[3] <= 1e-6f) return;
        const float sx = (v[0] / v[3] * 0.5f + 0.5f) * (float)W;
        const float sy = (v[1] / v[3] * 0.5f + 0.5f) * (float)H;
        t.X[k] = (long long)floorf(sx * 256.0f + 0.5f);
        t.Y[k] = (long long)floorf(sy * 256.0f + 0.5f);
        t.zw[k] = v[2] / v[3];
        t.iw[k] = 1.0f / v[3];
    }
    const long long area = edge_fn(t.X[0], t.Y[0], t.X[1], t.Y[1], t.X[2], t.Y[2]);
    if (area == 0) return;
    t.sgn = area > 0 ? 1 : -1;
    long long xmin = t.X[0], xmax = t.X[0], ymin = t.Y[0], ymax = t.Y[0];
#pragma unroll
    for (int k = 1; k < 3; ++k) {
        xmin = t.X[k] < xmin ? t.X[k] : xmin; xmax = t.X[k] > xmax ? t.X[k] : xmax;
        ymin = t.Y[k] < ymin ? t.Y[k] : ymin; ymax = t.Y[k] > ymax ? t.Y[k] : ymax;
    }
    long long px0 = (xmin - 128 + 255) >> 8, px1 = (xmax - 128) >> 8, py0 = (ymin - 128 + 255) >> 8, py1 = (ymax - 128) >> 8;
    px0 = px0 < 0 ? 0 : px0; py0 = py0 < 0 ? 0 : py0;
    px1 = px1 > W - 1 ? W - 1 : px1; py1 = py1 > H - 1 ? H - 1 : py1;
    if (px1 < px0 || py1 < py0) return;
    t.px0 = (int)px0; t.px1 = (int)px1; t.py0 = (int)py0; t.py1 = (int)py1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, c = (k + 2) % 3;
        t.own[k] = t.sgn > 0 ? edge_owns_tie(t.X[a], t.Y[a], t.X[c], t.Y[c]) : edge_owns_tie(t.X[c], t.Y[c], t.X[a], t.Y[a]);
    }
    t.valid = true;
}

// coverage + depth of pixel (px,py); on a hit fills the screen-space barycentrics
__device__ __forceinline__ bool tri_sample(const TriSetup& t, int px, int py, float& z, float (&bary)[3]) {
    const long long cx = (long long)px * 256 + 128, cy = (long long)py * 256 + 128;
    long long E[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, c = (k + 2) % 3;
        E[k] = t.sgn * edge_fn(t.X[a], t.Y[a], t.X[c], t.Y[c], cx, cy);
        if (E[k] < 0 || (E[k] == 0 && !t.own[k])) return false;
    }
    const float tot = (float)(E[0] + E[1] + E[2]);
    bary[0] = (float)E[0] / tot; bary[1] = (float)E[1] / tot; bary[2] = (float)E[2] / tot;
    z = bary[0] * t.zw[0] + bary[1] * t.zw[1] + bary[2] * t.zw[2];
    return z >= -1.0f && z <= 1.0f;
}

__device__ __forceinline__ unsigned long long depth_key(float z, int f) {
    z = z + 0.0f;                                             // -0 -> +0
    const unsigned bits = __float_as_uint(z);
    const unsigned ord = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);      // order preserving
    return ((unsigned long long)ord << 32) | (unsigned)f;
}

__global__ __launch_bounds__(RB) void k_raster_tris(const float* __restrict__ pos, int B, int V, const int32_t* __restrict__ tri,
                                                    int F, int H, int W, unsigned long long* __restrict__ zbuf,
                                                    int* __restrict__ big_count, int2* __restrict__ big_list) {
    const long long i = (long long)blockIdx.x * RB + threadIdx.x;
    if (i >= (long long)B * F) return;
    const int b = (int)(i / F), f = (int)(i - (long long)b * F);
    TriSetup t;
    tri_setup(pos + (size_t)b * V * 4, V, tri, f, H, W, t);
    if (!t.valid) return;
    const int bw = t.px1 - t.px0 + 1, bh = t.py1 - t.py0 + 1;
    if (bw * bh > SMALL_BOX) {
        const int slot = atomicAdd(big_count, 1);
        big_list[slot] = make_int2(b, f);
        return;
    }
    unsigned long long* zb = zbuf + (size_t)b * H * W;
    for (int py = t.py0; py <= t.py1; ++py)
        for (int px = t.px0; px <= t.px1; ++px) {
            float z, bary[3];
            if (tri_sample(t, px, py, z, bary)) atomicMin(zb + (size_t)py * W + px, depth_key(z, f));
        }
}

__global__ __launch_bounds__(RB) void k_raster_big(const float* __restrict__ pos, int V, const int32_t* __restrict__ tri, int H, int W,
                                                   unsigned long long* __restrict__ zbuf, const int* __restrict__ big_count,
                                                   const int2* __restrict__ big_list) {
    const int n = *big_count;
    for (int item = blockIdx.x; item < n; item += gridDim.x) {
        const int b = big_list[item].x, f = big_list[item].y;
        TriSetup t;
        tri_setup(pos + (size_t)b * V * 4, V, tri, f, H, W, t);
        if (!t.valid) continue;
        const int bw = t.px1 - t.px0 + 1, bh = t.py1 - t.py0 + 1;
        unsigned long long* zb = zbuf + (size_t)b * H * W;
        for (int k = threadIdx.x; k < bw * bh; k += RB) {
            const int px = t.px0 + k % bw, py = t.py0 + k / bw;
            float z, bary[3];
            if (tri_sample(t, px, py, z, bary)) atomicMin(zb + (size_t)py * W + px, depth_key(z, f));
        }
    }
}

__global__ __launch_bounds__(RB) void k_raster_resolve(const float* __restrict__ pos, int B, int V, const int32_t* __restrict__ tri, int H,
                                                       int W, const unsigned long long* __restrict__ zbuf, float* __restrict__ rast) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    const size_t npix = (size_t)H * W;
    if (i >= (size_t)B * npix) return;
    const unsigned long long key = zbuf[i];
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
    if (key != ~0ull) {
        const int b = (int)(i / npix), f = (int)(unsigned)(key & 0xFFFFFFFFull);
        const int px = (int)(i % W), py = (int)((i % npix) / W);
        TriSetup t;
        tri_setup(pos + (size_t)b * V * 4, V, tri, f, H, W, t);
        float z, bary[3];
        if (t.valid && tri_sample(t, px, py, z, bary)) {
            const float q0 = bary[0] * t.iw[0], q1 = bary[1] * t.iw[1], q2 = bary[2] * t.iw[2];
            const float S = q0 + q1 + q2;
            out = f32x4{q0 / S, q1 / S, z, (float)(f + 1)};
        }
    }
    reinterpret_cast<f32x4*>(rast)[i] = out;
}

__global__ __launch_bounds__(RB) void k_interpolate(const float* __restrict__ attr, int Battr, int Vattr, int A, const float* __restrict__ rast,
                                                    int B, size_t npix, const int32_t* __restrict__ tri, int F, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= (size_t)B * npix) return;
    const f32x4 r = reinterpret_cast<const f32x4*>(rast)[i];
    float* o = out + i * A;
    const int id = (int)r[3] - 1;
    if (id < 0 || id >= F) {
        for (int a = 0; a < A; ++a) o[a] = 0.0f;
        return;
    }
    const int b = (int)(i / npix);
    const float* at = attr + (Battr > 1 ? (size_t)b * Vattr * A : 0);
    const float u = r[0], v = r[1], w = 1.0f - u - v;
    const float* a0 = at + (size_t)tri[3 * id] * A;
    const float* a1 = at + (size_t)tri[3 * id + 1] * A;
    const float* a2 = at + (size_t)tri[3 * id + 2] * A;
    for (int a = 0; a < A; ++a) o[a] = u * a0[a] + v * a1[a] + w * a2[a];
}

}  // namespace

extern "C" {

size_t mve_rasterize_workspace_bytes(int B, int H, int W, int F) {
    return (size_t)B * H * W * 8 + (size_t)B * F * sizeof(int2) + 256;
}

int mve_rasterize(const float* d_pos, int B, int V, const int32_t* d_tri, int F, int H, int W, float* d_rast, void* d_workspace,
                  size_t workspace_bytes, void* stream) {
    if (B == 0 || H == 0 || W == 0) return MVE_OK;
    MVE_CHECK(d_pos && d_rast && d_workspace && (F == 0 || d_tri), MVE_ERR_ARG, "rasterize: null pointer");
    MVE_CHECK(H <= 8192 && W <= 8192, MVE_ERR_ARG, "rasterize: resolution %dx%d too large", H, W);
    MVE_CHECK(workspace_bytes >= mve_rasterize_workspace_bytes(B, H, W, F), MVE_ERR_NOMEM, "rasterize: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* zbuf = (unsigned long long*)d_workspace;
    const size_t npix = (size_t)B * H * W;
    int* big_count = (int*)(zbuf + npix);
    int2* big_list = (int2*)(big_count + 16);
    MVE_HIP(hipMemsetAsync(zbuf, 0xFF, npix * 8, s));
    MVE_HIP(hipMemsetAsync(big_count, 0, 64, s));
    if (F > 0) {
        k_raster_tris<<<mve_cdiv((size_t)B * F, RB), RB, 0, s>>>(d_pos, B, V, d_tri, F, H, W, zbuf, big_count, big_list);
        MVE_LAUNCH_CHECK();
        k_raster_big<<<1024, RB, 0, s>>>(d_pos, V, d_tri, H, W, zbuf, big_count, big_list);
        MVE_LAUNCH_CHECK();
    }
    k_raster_resolve<<<mve_cdiv(npix, RB), RB, 0, s>>>(d_pos, B, V, d_tri, H, W, zbuf, d_rast);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_interpolate(const float* d_attr, int Battr, int Vattr, int A, const float* d_rast, int B, int H, int W, const int32_t* d_tri,
                    int F, float* d_out, void* stream) {
    const size_t n = (size_t)B * H * W;
    if (n == 0 || A == 0) return MVE_OK;
    MVE_CHECK(d_attr && d_rast && d_tri && d_out, MVE_ERR_ARG, "interpolate: null pointer");
    MVE_CHECK(Battr == 1 || Battr == B, MVE_ERR_ARG, "interpolate: attribute batch %d must be 1 or %d", Battr, B);
    k_interpolate<<<mve_cdiv(n, RB), RB, 0, (hipStream_t)stream>>>(d_attr, Battr, Vattr, A, d_rast, B, (size_t)H * W, d_tri, F, d_out);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // extern "C"

// =========================================================================================================
// Multi-view texture back-projection (MeshRenderer.bake_multiview, base_mesh_renderer.py:507-603).
//
// The reference obtains per-texel visibility as the gradient of dr.texture(ones, texc) w.r.t. the texture, i.e. the sum of
// the texture-filter footprint weights of every screen pixel that samples the texel.  For the bilinear filter that is a
// scatter-add of the four bilinear weights of each foreground pixel, which is what k_splat_visibility does -- in 2^-32
// fixed point through 64-bit integer atomics, so the result does not depend on the order the atomics land (deterministic).
// The reference's default filter is 'linear-mipmap-linear' (nvdiffrast, unavailable here); the mip pyramid is NOT
// reproduced: both the visibility splat and the image fetch use the plain bilinear filter with wrap addressing
// (nvdiffrast's default boundary mode).  DESIGN.md lists this as a known deviation.
// =========================================================================================================
namespace {

__device__ __forceinline__ int wrapi(int i, int n) { i %= n; return i < 0 ? i + n : i; }

// bilinear taps of texture coordinate (u,v) on an n_x x n_y grid with texel centres at (i + 0.5)/n
__device__ __forceinline__ void bilinear_taps(float u, float v, int nx, int ny, int (&ix)[2], int (&iy)[2], float (&wx)[2], float (&wy)[2]) {
    const float x = u * (float)nx - 0.5f, y = v * (float)ny - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    wx[1] = x - fx; wx[0] = 1.0f - wx[1];
    wy[1] = y - fy; wy[0] = 1.0f - wy[1];
    ix[0] = wrapi((int)fx, nx); ix[1] = wrapi((int)fx + 1, nx);
    iy[0] = wrapi((int)fy, ny); iy[1] = wrapi((int)fy + 1, ny);
}

__global__ __launch_bounds__(RB) void k_splat_visibility(const float* __restrict__ texc /*[n,h,w,2]*/, const float* __restrict__ rast,
                                                         size_t npix_total, size_t npix_view, int map, unsigned long long* __restrict__ acc) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= npix_total) return;
    if (!(rast[4 * i + 3] > 0.0f)) return;
    const size_t view = i / npix_view;
    int ix[2], iy[2];
    float wx[2], wy[2];
    bilinear_taps(texc[2 * i], texc[2 * i + 1], map, map, ix, iy, wx, wy);
    unsigned long long* a = acc + view * (size_t)map * map;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double wgt = (double)(wx[k] * wy[j]);
            atomicAdd(a + (size_t)iy[j] * map + ix[k], (unsigned long long)(wgt * 4294967296.0 + 0.5));
        }
}

// cos weight of a view pixel: clamp(-n.dir, 0)^pow * alpha with n = depth_to_normal(depth, normalised dirs, 'opencv')*2-1
// (base_mesh_renderer.py:559-564)
__global__ __launch_bounds__(RB) void k_view_cos_weight(const float* __restrict__ depth, const float* __restrict__ alpha,
                                                        const float* __restrict__ intr, int nb, int h, int w, float pw, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= (size_t)nb * h * w) return;
    const int x = (int)(i % w), y = (int)((i / w) % h), v = (int)(i / ((size_t)w * h));
    const float fx = intr[4 * v], fy = intr[4 * v + 1], cx = intr[4 * v + 2], cy = intr[4 * v + 3];
    auto dirn = [&](int xx, int yy, float (&d)[3]) {
        const float dx = ((float)xx + 0.5f - cx) / fx, dy = ((float)yy + 0.5f - cy) / fy;
        const float n = fmaxf(sqrtf(dx * dx + dy * dy + 1.0f), 1e-12f);
        d[0] = dx / n; d[1] = dy / n; d[2] = 1.0f / n;
    };
    auto point = [&](int xx, int yy, float (&p)[3]) {
        float d[3];
        dirn(xx, yy, d);
        const float inv = 1.0f / fmaxf(depth[((size_t)v * h + yy) * w + xx], 1e-6f);
        p[0] = d[0] * inv; p[1] = d[1] * inv; p[2] = d[2] * inv;
    };
    const int xr = x < w - 1 ? x : w - 2, xl = x > 0 ? x - 1 : 0, yd = y < h - 1 ? y : h - 2, yu = y > 0 ? y - 1 : 0;
    float a[3], b[3], right[3], left[3], up[3], down[3];
    point(xr + 1, y, a); point(xr, y, b);
    for (int k = 0; k < 3; ++k) right[k] = a[k] - b[k];
    point(xl + 1, y, a); point(xl, y, b);
    for (int k = 0; k < 3; ++k) left[k] = -(a[k] - b[k]);
    point(x, yu + 1, a); point(x, yu, b);
    for (int k = 0; k < 3; ++k) up[k] = -(a[k] - b[k]);
    point(x, yd + 1, a); point(x, yd, b);
    for (int k = 0; k < 3; ++k) down[k] = a[k] - b[k];
    float s[3] = {0.f, 0.f, 0.f};
    auto acc_cross = [&](const float (&p)[3], const float (&q)[3]) {
        const float c0 = p[1] * q[2] - p[2] * q[1], c1 = p[2] * q[0] - p[0] * q[2], c2 = p[0] * q[1] - p[1] * q[0];
        const float n = fmaxf(sqrtf(c0 * c0 + c1 * c1 + c2 * c2), 1e-12f);
        s[0] += c0 / n; s[1] += c1 / n; s[2] += c2 / n;
    };
    acc_cross(right, up); acc_cross(up, left); acc_cross(left, down); acc_cross(down, right);
    const float n = fmaxf(sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]), 1e-12f);
    // opencv format: no sign flip; the reference maps to [0,1] and back (x/2+0.5)*2-1
    float nn[3];
    for (int k = 0; k < 3; ++k) nn[k] = (s[k] / n / 2 + 0.5f) * 2 - 1;
    float d[3];
    dirn(x, y, d);
    const float c = fmaxf(-(nn[0] * d[0] + nn[1] * d[1] + nn[2] * d[2]), 0.0f);
    out[i] = powf(c, pw) * alpha[i];
}

// -max_pool2d(-x, 5, stride 1, padding 2): minimum over the in-image part of the 5x5 window
__global__ __launch_bounds__(RB) void k_minpool5(const float* __restrict__ in, int nb, int h, int w, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= (size_t)nb * h * w) return;
    const int x = (int)(i % w), y = (int)((i / w) % h);
    const float* img = in + (i / ((size_t)w * h)) * (size_t)w * h;
    float m = INFINITY;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) m = fminf(m, img[(size_t)yy * w + xx]);
        }
    out[i] = m;
}

// per texel: for every view of the batch fetch (image rgb, view weight) at the texel's projected position and accumulate
// sum(rgb * weight), sum(weight) with weight = view_weight * visibility     (base_mesh_renderer.py:566-582)
__global__ __launch_bounds__(RB) void k_bake_accumulate(const float* __restrict__ tex_rast, const int32_t* __restrict__ f, int F,
                                                        const float* __restrict__ v_img /*[n,V,2]*/, int V, const float* __restrict__ images /*[n,h,w,3]*/,
                                                        const float* __restrict__ w_img /*[n,h,w]*/, const unsigned long long* __restrict__ vis /*[n,map,map]*/,
                                                        int n, int h, int w, int map, float* __restrict__ accum /*[map,map,4]*/) {
    const size_t t = (size_t)blockIdx.x * RB + threadIdx.x;
    if (t >= (size_t)map * map) return;
    const f32x4 r = reinterpret_cast<const f32x4*>(tex_rast)[t];
    const int id = (int)r[3] - 1;
    f32x4 acc = reinterpret_cast<f32x4*>(accum)[t];
    for (int v = 0; v < n; ++v) {
        float cu = 0.f, cv = 0.f;                           // dr.interpolate gives 0 on empty texels
        if (id >= 0 && id < F) {
            const float* vi = v_img + (size_t)v * V * 2;
            const int i0 = f[3 * id], i1 = f[3 * id + 1], i2 = f[3 * id + 2];
            const float bw = 1.0f - r[0] - r[1];
            cu = r[0] * vi[2 * i0] + r[1] * vi[2 * i1] + bw * vi[2 * i2];
            cv = r[0] * vi[2 * i0 + 1] + r[1] * vi[2 * i1 + 1] + bw * vi[2 * i2 + 1];
        }
        int ix[2], iy[2];
        float wx[2], wy[2];
        bilinear_taps(cu, cv, w, h, ix, iy, wx, wy);
        const float* img = images + (size_t)v * h * w * 3;
        const float* wi = w_img + (size_t)v * h * w;
        float c0 = 0.f, c1 = 0.f, c2 = 0.f, cw = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float wt = wx[k] * wy[j];
                const size_t p = (size_t)iy[j] * w + ix[k];
                c0 += wt * img[3 * p]; c1 += wt * img[3 * p + 1]; c2 += wt * img[3 * p + 2];
                cw += wt * wi[p];
            }
        const float visib = (float)((double)vis[(size_t)v * map * map + t] * (1.0 / 4294967296.0));
        const float weight = cw * visib;
        acc[0] += c0 * weight; acc[1] += c1 * weight; acc[2] += c2 * weight; acc[3] += weight;
    }
    reinterpret_cast<f32x4*>(accum)[t] = acc;
}

__global__ __launch_bounds__(RB) void k_bake_finalize(const float* __restrict__ accum, size_t ntex, float* __restrict__ albedo_chw) {
    const size_t t = (size_t)blockIdx.x * RB + threadIdx.x;
    if (t >= ntex) return;
    const f32x4 a = reinterpret_cast<const f32x4*>(accum)[t];
    const float d = fmaxf(a[3], 1e-8f);
    albedo_chw[t] = a[0] / d; albedo_chw[ntex + t] = a[1] / d; albedo_chw[2 * ntex + t] = a[2] / d;
}

}  // namespace

extern "C" {

int mve_splat_visibility(const float* d_texc, const float* d_rast, int n, int h, int w, int map_size, void* d_vis_u64, void* stream) {
    const size_t total = (size_t)n * h * w;
    if (total == 0) return MVE_OK;
    MVE_CHECK(d_texc && d_rast && d_vis_u64 && map_size > 0, MVE_ERR_ARG, "splat_visibility: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    MVE_HIP(hipMemsetAsync(d_vis_u64, 0, (size_t)n * map_size * map_size * 8, s));
    k_splat_visibility<<<mve_cdiv(total, RB), RB, 0, s>>>(d_texc, d_rast, total, (size_t)h * w, map_size, (unsigned long long*)d_vis_u64);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_view_weight(const float* d_depth, const float* d_alpha, const float* d_intrinsics, int n, int h, int w, float cos_weight_pow,
                    float* d_tmp, float* d_out, void* stream) {
    const size_t total = (size_t)n * h * w;
    if (total == 0) return MVE_OK;
    MVE_CHECK(d_depth && d_alpha && d_intrinsics && d_tmp && d_out && h >= 2 && w >= 2, MVE_ERR_ARG, "view_weight: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    k_view_cos_weight<<<mve_cdiv(total, RB), RB, 0, s>>>(d_depth, d_alpha, d_intrinsics, n, h, w, cos_weight_pow, d_tmp);
    MVE_LAUNCH_CHECK();
    k_minpool5<<<mve_cdiv(total, RB), RB, 0, s>>>(d_tmp, n, h, w, d_out);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_bake_accumulate(const float* d_tex_rast, const int32_t* d_f, int F, const float* d_v_img, int V, const float* d_images,
                        const float* d_w_img, const void* d_vis_u64, int n, int h, int w, int map_size, float* d_accum, void* stream) {
    if (n == 0 || map_size == 0) return MVE_OK;
    MVE_CHECK(d_tex_rast && d_f && d_v_img && d_images && d_w_img && d_vis_u64 && d_accum, MVE_ERR_ARG, "bake_accumulate: null pointer");
    k_bake_accumulate<<<mve_cdiv((size_t)map_size * map_size, RB), RB, 0, (hipStream_t)stream>>>(
        d_tex_rast, d_f, F, d_v_img, V, d_images, d_w_img, (const unsigned long long*)d_vis_u64, n, h, w, map_size, d_accum);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_bake_finalize(const float* d_accum, int map_size, float* d_albedo_chw, void* stream) {
    if (map_size == 0) return MVE_OK;
    MVE_CHECK(d_accum && d_albedo_chw, MVE_ERR_ARG, "bake_finalize: null pointer");
    const size_t ntex = (size_t)map_size * map_size;
    k_bake_finalize<<<mve_cdiv(ntex, RB), RB, 0, (hipStream_t)stream>>>(d_accum, ntex, d_albedo_chw);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // extern "C"

// =========================================================================================================
// dr.antialias, dr.texture (bilinear) and the SSAA box filter of MeshRenderer.forward (base_mesh_renderer.py:258-263, :289-293,
// :380-383).  The antialias rules are the ones specified in oracle/raster_oracle.c (nvdiffrast itself is unavailable).
// =========================================================================================================
namespace {

constexpr unsigned long long EMPTY_KEY = ~0ull;

__device__ __forceinline__ unsigned long long edge_key(int a, int b) {
    const unsigned ua = (unsigned)a, ub = (unsigned)b;
    return ua < ub ? ((unsigned long long)ua << 32 | ub) : ((unsigned long long)ub << 32 | ua);
}
__device__ __forceinline__ unsigned edge_hash(unsigned long long k, unsigned mask) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned)k & mask;
}

// open-addressing table keyed by the undirected edge; every slot counts its users and remembers the first two
__global__ __launch_bounds__(RB) void k_edge_insert(const int32_t* __restrict__ tri, int F, const int32_t* __restrict__ f_live, unsigned mask,
                                                    unsigned long long* __restrict__ keys, int* __restrict__ cnt, int* __restrict__ ent) {
    const int i = blockIdx.x * RB + threadIdx.x;
    if (i >= 3 * mcap_live(F, f_live)) return;              // capacity form: padded faces would all insert the key (0, 0)
    const int f = i / 3, e = i - 3 * f;
    const unsigned long long key = edge_key(tri[3 * f + e], tri[3 * f + (e + 1) % 3]);
    unsigned h = edge_hash(key, mask);
    for (;;) {
        const unsigned long long old = atomicCAS(keys + h, EMPTY_KEY, key);
        if (old == EMPTY_KEY || old == key) {
            const int slot = atomicAdd(cnt + h, 1);
            if (slot < 2) ent[2 * h + slot] = i;
            return;
        }
        h = (h + 1) & mask;
    }
}
__global__ __launch_bounds__(RB) void k_edge_opposites(const int32_t* __restrict__ tri, int F, const int32_t* __restrict__ f_live, unsigned mask,
                                                       const unsigned long long* __restrict__ keys, const int* __restrict__ cnt,
                                                       const int* __restrict__ ent, int32_t* __restrict__ opp) {
    const int i = blockIdx.x * RB + threadIdx.x;
    if (i >= 3 * F) return;
    if (i >= 3 * mcap_live(F, f_live)) { opp[i] = MVE_MCAP_PAD_OPP; return; }
    const int f = i / 3, e = i - 3 * f;
    const unsigned long long key = edge_key(tri[3 * f + e], tri[3 * f + (e + 1) % 3]);
    unsigned h = edge_hash(key, mask);
    while (keys[h] != key) h = (h + 1) & mask;
    int o = -1;
    if (cnt[h] == 2) {
        const int other = ent[2 * h] == i ? ent[2 * h + 1] : ent[2 * h];
        o = tri[3 * (other / 3) + (other % 3 + 2) % 3];
    }
    opp[i] = o;
}

struct AAView { const float* rast; const float* pos; const int32_t* tri; const int32_t* opp; int V, F, H, W; };

// the pair rule of oracle/raster_oracle.c:aa_pair, operation for operation
__device__ __forceinline__ bool aa_pair(const AAView& a, int px, int py, int qx, int qy, bool& dst_is_p, float& wgt) {
    const f32x4 rp = reinterpret_cast<const f32x4*>(a.rast)[(size_t)py * a.W + px];
    const f32x4 rq = reinterpret_cast<const f32x4*>(a.rast)[(size_t)qy * a.W + qx];
    const int ip = (int)rp[3] - 1, iq = (int)rq[3] - 1;
    if (ip == iq) return false;
    bool use_p;
    if (ip < 0) use_p = false;
    else if (iq < 0) use_p = true;
    else if (rp[2] != rq[2]) use_p = rp[2] < rq[2];
    else use_p = (py * a.W + px) < (qy * a.W + qx);
    const int t = use_p ? ip : iq;
    if (t < 0 || t >= a.F) return false;
    const int ox = use_p ? px : qx, oy = use_p ? py : qy, nx = use_p ? qx : px, ny = use_p ? qy : py;
    float sx[3], sy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int vi = a.tri[3 * t + k];
        if (vi < 0 || vi >= a.V) return false;
        const f32x4 v = reinterpret_cast<const f32x4*>(a.pos)[vi];
        if (v[3] <= 1e-6f) return false;
        sx[k] = (v[0] / v[3] * 0.5f + 0.5f) * (float)a.W;
        sy[k] = (v[1] / v[3] * 0.5f + 0.5f) * (float)a.H;
    }
    const float cx = (float)ox + 0.5f, cy = (float)oy + 0.5f;
    const float dx = (float)(nx - ox), dy = (float)(ny - oy);
    float best = 2.0f;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int ia = e, ib = (e + 1) % 3, ic = (e + 2) % 3;
        const float ex = sx[ib] - sx[ia], ey = sy[ib] - sy[ia];
        const int o = a.opp[3 * t + e];
        if (o >= 0) {
            if (o >= a.V) continue;
            const f32x4 v = reinterpret_cast<const f32x4*>(a.pos)[o];
            if (v[3] <= 1e-6f) continue;
            const float oxs = (v[0] / v[3] * 0.5f + 0.5f) * (float)a.W, oys = (v[1] / v[3] * 0.5f + 0.5f) * (float)a.H;
            const float sc = ex * (sy[ic] - sy[ia]) - ey * (sx[ic] - sx[ia]);
            const float so = ex * (oys - sy[ia]) - ey * (oxs - sx[ia]);
            if (!(sc * so >= 0.0f)) continue;
        }
        float s, tt;
        if (dy == 0.0f) {
            if (ey == 0.0f) continue;
            s = (cy - sy[ia]) / ey;
            tt = ((sx[ia] + s * ex) - cx) * dx;
        } else {
            if (ex == 0.0f) continue;
            s = (cx - sx[ia]) / ex;
            tt = ((sy[ia] + s * ey) - cy) * dy;
        }
        if (s >= 0.0f && s <= 1.0f && tt >= 0.0f && tt <= 1.0f && tt < best) best = tt;
    }
    if (best > 1.0f) return false;
    if (best > 0.5f) { dst_is_p = !use_p; wgt = best - 0.5f; }
    else if (best < 0.5f) { dst_is_p = use_p; wgt = 0.5f - best; }
    else return false;
    return true;
}

template <int C>
__global__ __launch_bounds__(RB) void k_antialias(const float* __restrict__ color, int B, int H, int W, int Cdyn, const float* __restrict__ rast,
                                                  const float* __restrict__ pos, int V, const int32_t* __restrict__ tri, int F,
                                                  const int32_t* __restrict__ opp, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    const size_t npix = (size_t)H * W;
    if (i >= (size_t)B * npix) return;
    const int b = (int)(i / npix), y = (int)((i % npix) / W), x = (int)(i % W);
    const int Cn = C > 0 ? C : Cdyn;
    AAView a{rast + (size_t)b * npix * 4, pos + (size_t)b * V * 4, tri, opp, V, F, H, W};
    const float* col = color + (size_t)b * npix * Cn;
    const float* self = col + ((size_t)y * W + x) * Cn;
    float* dst = out + i * Cn;
    for (int c = 0; c < Cn; ++c) dst[c] = self[c];
    const int ddx[4] = {-1, 1, 0, 0}, ddy[4] = {0, 0, -1, 1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = x + ddx[k], qy = y + ddy[k];
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        bool dst_is_p;
        float w;
        if (!aa_pair(a, x, y, qx, qy, dst_is_p, w) || !dst_is_p) continue;
        const float* nb = col + ((size_t)qy * W + qx) * Cn;
        for (int c = 0; c < Cn; ++c) dst[c] = dst[c] + w * (nb[c] - self[c]);
    }
}

__global__ __launch_bounds__(RB) void k_texture_bilinear(const float* __restrict__ tex, int Bt, int th, int tw, int C,
                                                         const float* __restrict__ uv, const float* __restrict__ rast, size_t npix_total,
                                                         size_t npix_view, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= npix_total) return;
    float* o = out + i * C;
    if (rast && !(rast[4 * i + 3] > 0.0f)) { for (int c = 0; c < C; ++c) o[c] = 0.0f; return; }
    const float* t = tex + (Bt > 1 ? (i / npix_view) * (size_t)th * tw * C : 0);
    int ix[2], iy[2];
    float wx[2], wy[2];
    bilinear_taps(uv[2 * i], uv[2 * i + 1], tw, th, ix, iy, wx, wy);
    for (int c = 0; c < C; ++c) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) acc += (wx[k] * wy[j]) * t[((size_t)iy[j] * tw + ix[k]) * C + c];
        o[c] = acc;
    }
}

// F.interpolate(mode='area', scale 1/f) on channel-last images: mean over f x f boxes
__global__ __launch_bounds__(RB) void k_box_downsample(const float* __restrict__ x, int B, int H, int W, int C, int f, float* __restrict__ y) {
    const int Ho = H / f, Wo = W / f;
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= (size_t)B * Ho * Wo * C) return;
    const int c = (int)(i % C), xo = (int)((i / C) % Wo), yo = (int)((i / ((size_t)C * Wo)) % Ho), b = (int)(i / ((size_t)C * Wo * Ho));
    float acc = 0.0f;
    for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) acc += x[(((size_t)b * H + yo * f + dy) * W + xo * f + dx) * C + c];
    y[i] = acc / (float)(f * f);
}

}  // namespace

extern "C" {

size_t mve_edge_opposites_workspace_bytes(int F) {
    size_t T = 16;
    while (T < (size_t)12 * (F > 0 ? F : 1)) T <<= 1;
    return T * (8 + 4 + 8) + 256;
}

// exact (d_f_live == nullptr) and capacity form (F = f_cap, *d_f_live = live faces) in one body
static int edge_opposites_impl(const int32_t* d_tri, int F, const int32_t* d_f_live, int32_t* d_opp, void* d_workspace, size_t workspace_bytes,
                               void* stream) {
    if (F == 0) return MVE_OK;
    MVE_CHECK(d_tri && d_opp && d_workspace, MVE_ERR_ARG, "edge_opposites: null pointer");
    MVE_CHECK(workspace_bytes >= mve_edge_opposites_workspace_bytes(F), MVE_ERR_NOMEM, "edge_opposites: workspace too small");
    size_t T = 16;
    while (T < (size_t)12 * F) T <<= 1;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)d_workspace;
    int* cnt = (int*)(keys + T);
    int* ent = cnt + T;
    MVE_HIP(hipMemsetAsync(keys, 0xff, T * 8, s));
    MVE_HIP(hipMemsetAsync(cnt, 0, T * 4, s));
    k_edge_insert<<<mve_cdiv(3 * F, RB), RB, 0, s>>>(d_tri, F, d_f_live, (unsigned)(T - 1), keys, cnt, ent);
    MVE_LAUNCH_CHECK();
    k_edge_opposites<<<mve_cdiv(3 * F, RB), RB, 0, s>>>(d_tri, F, d_f_live, (unsigned)(T - 1), keys, cnt, ent, d_opp);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_edge_opposites(const int32_t* d_tri, int F, int32_t* d_opp, void* d_workspace, size_t workspace_bytes, void* stream) {
    return edge_opposites_impl(d_tri, F, nullptr, d_opp, d_workspace, workspace_bytes, stream);
}

int mve_edge_opposites_n(const int32_t* d_tri, int f_cap, const int32_t* d_live, int32_t* d_opp, void* d_workspace, size_t workspace_bytes,
                         void* stream) {
    MVE_CHECK(f_cap > 0 && d_live, MVE_ERR_ARG, "edge_opposites_n: capacity must be positive and the live counts given");
    return edge_opposites_impl(d_tri, f_cap, d_live + 1, d_opp, d_workspace, workspace_bytes, stream);
}

int mve_antialias(const float* d_color, int B, int H, int W, int C, const float* d_rast, const float* d_pos, int V, const int32_t* d_tri,
                  int F, const int32_t* d_opp, float* d_out, void* stream) {
    const size_t total = (size_t)B * H * W;
    if (total == 0 || C == 0) return MVE_OK;
    MVE_CHECK(d_color && d_rast && d_pos && d_tri && d_opp && d_out && d_out != d_color, MVE_ERR_ARG, "antialias: bad arguments (out must not alias color)");
    hipStream_t s = (hipStream_t)stream;
    if (C == 8) k_antialias<8><<<mve_cdiv(total, RB), RB, 0, s>>>(d_color, B, H, W, C, d_rast, d_pos, V, d_tri, F, d_opp, d_out);
    else if (C == 4) k_antialias<4><<<mve_cdiv(total, RB), RB, 0, s>>>(d_color, B, H, W, C, d_rast, d_pos, V, d_tri, F, d_opp, d_out);
    else k_antialias<0><<<mve_cdiv(total, RB), RB, 0, s>>>(d_color, B, H, W, C, d_rast, d_pos, V, d_tri, F, d_opp, d_out);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_texture_bilinear(const float* d_tex, int Bt, int th, int tw, int C, const float* d_uv, const float* d_rast, int n, int h, int w,
                         float* d_out, void* stream) {
    const size_t total = (size_t)n * h * w;
    if (total == 0 || C == 0) return MVE_OK;
    MVE_CHECK(d_tex && d_uv && d_out && th > 0 && tw > 0 && (Bt == 1 || Bt == n), MVE_ERR_ARG, "texture_bilinear: bad arguments");
    k_texture_bilinear<<<mve_cdiv(total, RB), RB, 0, (hipStream_t)stream>>>(d_tex, Bt, th, tw, C, d_uv, d_rast, total, (size_t)h * w, d_out);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_box_downsample(const float* d_x, int B, int H, int W, int C, int factor, float* d_y, void* stream) {
    MVE_CHECK(factor >= 1 && H % factor == 0 && W % factor == 0, MVE_ERR_ARG, "box_downsample: %dx%d not divisible by %d", H, W, factor);
    const size_t total = (size_t)B * (H / factor) * (W / factor) * C;
    if (total == 0) return MVE_OK;
    MVE_CHECK(d_x && d_y, MVE_ERR_ARG, "box_downsample: null pointer");
    k_box_downsample<<<mve_cdiv(total, RB), RB, 0, (hipStream_t)stream>>>(d_x, B, H, W, C, factor, d_y);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // extern "C"

// =========================================================================================================
// Backward of the linear render ops w.r.t. their colour-like input (mesh half): what optimising a
// texture map or vertex colours through MeshRenderer.forward needs.  All three forward ops are LINEAR in that input, so each
// backward is the exact transpose (tests check <forward(x), g> == <x, backward(g)>).  Geometry (rast, positions) carries no
// gradient here.
//   interpolate : d attr[vertex] += barycentric weight * d out[pixel]                       (float atomics)
//   texture     : d tex[texel]   += bilinear weight   * d out[pixel]                        (float atomics)
//   antialias   : gathered per input pixel from its four neighbours -- deterministic, no atomics
// =========================================================================================================
namespace {

__global__ __launch_bounds__(RB) void k_interpolate_bwd(const float* __restrict__ g_out, int Battr, int Vattr, int A, const float* __restrict__ rast,
                                                        int B, size_t npix, const int32_t* __restrict__ tri, int F, float* __restrict__ g_attr) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= (size_t)B * npix) return;
    const f32x4 r = reinterpret_cast<const f32x4*>(rast)[i];
    const int id = (int)r[3] - 1;
    if (id < 0 || id >= F) return;
    const int b = (int)(i / npix);
    float* at = g_attr + (Battr > 1 ? (size_t)b * Vattr * A : 0);
    const float u = r[0], v = r[1], w = 1.0f - u - v;
    float* a0 = at + (size_t)tri[3 * id] * A;
    float* a1 = at + (size_t)tri[3 * id + 1] * A;
    float* a2 = at + (size_t)tri[3 * id + 2] * A;
    const float* g = g_out + i * A;
    for (int a = 0; a < A; ++a) {
        const float ga = g[a];
        atomicAdd(a0 + a, u * ga); atomicAdd(a1 + a, v * ga); atomicAdd(a2 + a, w * ga);
    }
}

__global__ __launch_bounds__(RB) void k_texture_bilinear_bwd(const float* __restrict__ g_out, int Bt, int th, int tw, int C, const float* __restrict__ uv,
                                                             const float* __restrict__ rast, size_t npix_total, size_t npix_view,
                                                             float* __restrict__ g_tex) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= npix_total) return;
    if (rast && !(rast[4 * i + 3] > 0.0f)) return;
    float* t = g_tex + (Bt > 1 ? (i / npix_view) * (size_t)th * tw * C : 0);
    int ix[2], iy[2];
    float wx[2], wy[2];
    bilinear_taps(uv[2 * i], uv[2 * i + 1], tw, th, ix, iy, wx, wy);
    const float* g = g_out + i * C;
    for (int c = 0; c < C; ++c) {
        const float gc = g[c];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) atomicAdd(t + ((size_t)iy[j] * tw + ix[k]) * C + c, (wx[k] * wy[j]) * gc);
    }
}

// forward: out[p] = in[p] + sum_{k: p receives} w_k (in[q_k] - in[p]).  Transpose, gathered at input pixel q:
//   g_in[q] = g[q] (1 - sum_{k: q receives} w_k) + sum_{neighbours p that receive from q} w(p,q) g[p]
__global__ __launch_bounds__(RB) void k_antialias_bwd(const float* __restrict__ g_out, int B, int H, int W, int C, const float* __restrict__ rast,
                                                      const float* __restrict__ pos, int V, const int32_t* __restrict__ tri, int F,
                                                      const int32_t* __restrict__ opp, float* __restrict__ g_in) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    const size_t npix = (size_t)H * W;
    if (i >= (size_t)B * npix) return;
    const int b = (int)(i / npix), y = (int)((i % npix) / W), x = (int)(i % W);
    AAView a{rast + (size_t)b * npix * 4, pos + (size_t)b * V * 4, tri, opp, V, F, H, W};
    const float* g = g_out + (size_t)b * npix * C;
    const float* gs = g + ((size_t)y * W + x) * C;
    float* dst = g_in + i * C;
    float keep = 1.0f;
    for (int c = 0; c < C; ++c) dst[c] = 0.0f;
    const int ddx[4] = {-1, 1, 0, 0}, ddy[4] = {0, 0, -1, 1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = x + ddx[k], qy = y + ddy[k];
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        bool dst_is_p;
        float w;
        if (!aa_pair(a, x, y, qx, qy, dst_is_p, w)) continue;      // the pair rule is symmetric in which pixel asks
        if (dst_is_p) {
            keep -= w;                                               // this pixel received from the neighbour
        } else {
            const float* gn = g + ((size_t)qy * W + qx) * C;         // the neighbour received from this pixel
            for (int c = 0; c < C; ++c) dst[c] += w * gn[c];
        }
    }
    for (int c = 0; c < C; ++c) dst[c] += keep * gs[c];
}

}  // namespace

extern "C" {

int mve_interpolate_backward(const float* d_grad_out, int Battr, int Vattr, int A, const float* d_rast, int B, int H, int W,
                             const int32_t* d_tri, int F, float* d_grad_attr, void* stream) {
    const size_t n = (size_t)B * H * W;
    if (n == 0 || A == 0) return MVE_OK;
    MVE_CHECK(d_grad_out && d_rast && d_tri && d_grad_attr && (Battr == 1 || Battr == B), MVE_ERR_ARG, "interpolate_backward: bad arguments");
    k_interpolate_bwd<<<mve_cdiv(n, RB), RB, 0, (hipStream_t)stream>>>(d_grad_out, Battr, Vattr, A, d_rast, B, (size_t)H * W, d_tri, F, d_grad_attr);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_texture_bilinear_backward(const float* d_grad_out, int Bt, int th, int tw, int C, const float* d_uv, const float* d_rast, int n, int h,
                                  int w, float* d_grad_tex, void* stream) {
    const size_t total = (size_t)n * h * w;
    if (total == 0 || C == 0) return MVE_OK;
    MVE_CHECK(d_grad_out && d_uv && d_grad_tex && th > 0 && tw > 0 && (Bt == 1 || Bt == n), MVE_ERR_ARG, "texture_bilinear_backward: bad arguments");
    k_texture_bilinear_bwd<<<mve_cdiv(total, RB), RB, 0, (hipStream_t)stream>>>(d_grad_out, Bt, th, tw, C, d_uv, d_rast, total, (size_t)h * w, d_grad_tex);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_antialias_backward(const float* d_grad_out, int B, int H, int W, int C, const float* d_rast, const float* d_pos, int V,
                           const int32_t* d_tri, int F, const int32_t* d_opp, float* d_grad_color, void* stream) {
    const size_t total = (size_t)B * H * W;
    if (total == 0 || C == 0) return MVE_OK;
    MVE_CHECK(d_grad_out && d_rast && d_pos && d_tri && d_opp && d_grad_color && d_grad_color != d_grad_out, MVE_ERR_ARG,
              "antialias_backward: bad arguments");
    k_antialias_bwd<<<mve_cdiv(total, RB), RB, 0, (hipStream_t)stream>>>(d_grad_out, B, H, W, C, d_rast, d_pos, V, d_tri, F, d_opp, d_grad_color);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // extern "C"

// =========================================================================================================
// Geometry gradients (mesh half): d rast / d clip-space vertices with every pixel's triangle held fixed,
// d interpolate / d (u, v), and the silhouette term of dr.antialias (d |tt - 1/2| / d the crossed edge's vertices).  Together they carry
// image-space gradients back to the DMTet vertices the reference optimises through dr.rasterize / dr.interpolate / dr.antialias
// (base_mesh_renderer.py:240-263).  The per-pixel arithmetic lives in raster_grad_core.h, which also compiles for the host: the CPU
// tests run that very source against autograd and against finite differences of the C oracle (oracle/raster_grad_oracle.py).
// =========================================================================================================
#include "raster_grad_core.h"

namespace {

__global__ __launch_bounds__(RB) void k_interpolate_bwd_rast(const float* __restrict__ attr, int Battr, int Vattr, int A, const float* __restrict__ rast,
                                                             int B, size_t npix, const int32_t* __restrict__ tri, int F,
                                                             const float* __restrict__ g_out, float* __restrict__ g_rast) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    if (i >= (size_t)B * npix) return;
    const int b = (int)(i / npix);
    rg_interpolate_bwd_rast(attr + (Battr > 1 ? (size_t)b * Vattr * A : 0), A, rast + 4 * i, tri, F, g_out + i * A, g_rast + 4 * i);
}

__global__ __launch_bounds__(RB) void k_rasterize_bwd(const float* __restrict__ pos, int B, int V, const int32_t* __restrict__ tri, int F, int H,
                                                      int W, const float* __restrict__ rast, const float* __restrict__ g_rast,
                                                      float* __restrict__ g_pos) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    const size_t npix = (size_t)H * W;
    if (i >= (size_t)B * npix) return;
    const int b = (int)(i / npix);
    rg_rasterize_bwd(pos + (size_t)b * V * 4, tri, F, H, W, rast + 4 * i, g_rast + 4 * i, (int)(i % W), (int)((i % npix) / W), g_pos + (size_t)b * V * 4);
}

__global__ __launch_bounds__(RB) void k_antialias_bwd_pos(const float* __restrict__ color, const float* __restrict__ g_out, int B, int H, int W,
                                                          int C, const float* __restrict__ rast, const float* __restrict__ pos, int V,
                                                          const int32_t* __restrict__ tri, int F, const int32_t* __restrict__ opp,
                                                          float* __restrict__ g_pos) {
    const size_t i = (size_t)blockIdx.x * RB + threadIdx.x;
    const size_t npix = (size_t)H * W;
    if (i >= (size_t)B * npix) return;
    const int b = (int)(i / npix), y = (int)((i % npix) / W), x = (int)(i % W);
    const RGView a{rast + (size_t)b * npix * 4, pos + (size_t)b * V * 4, tri, opp, V, F, H, W};
    rg_antialias_bwd_pos(a, color + (size_t)b * npix * C, g_out + i * C, C, x, y, g_pos + (size_t)b * V * 4);
}

}  // namespace

extern "C" {

int mve_interpolate_backward_rast(const float* d_attr, int Battr, int Vattr, int A, const float* d_rast, int B, int H, int W,
                                  const int32_t* d_tri, int F, const float* d_grad_out, float* d_grad_rast, void* stream) {
    const size_t n = (size_t)B * H * W;
    if (n == 0) return MVE_OK;
    MVE_CHECK(d_attr && d_rast && d_tri && d_grad_out && d_grad_rast && (Battr == 1 || Battr == B), MVE_ERR_ARG, "interpolate_backward_rast: bad arguments");
    k_interpolate_bwd_rast<<<mve_cdiv(n, RB), RB, 0, (hipStream_t)stream>>>(d_attr, Battr, Vattr, A, d_rast, B, (size_t)H * W, d_tri, F, d_grad_out, d_grad_rast);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_rasterize_backward(const float* d_pos, int B, int V, const int32_t* d_tri, int F, int H, int W, const float* d_rast,
                           const float* d_grad_rast, float* d_grad_pos, void* stream) {
    const size_t n = (size_t)B * H * W;
    if (n == 0) return MVE_OK;
    MVE_CHECK(d_pos && d_tri && d_rast && d_grad_rast && d_grad_pos, MVE_ERR_ARG, "rasterize_backward: null pointer");
    k_rasterize_bwd<<<mve_cdiv(n, RB), RB, 0, (hipStream_t)stream>>>(d_pos, B, V, d_tri, F, H, W, d_rast, d_grad_rast, d_grad_pos);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_antialias_backward_pos(const float* d_color, const float* d_grad_out, int B, int H, int W, int C, const float* d_rast,
                               const float* d_pos, int V, const int32_t* d_tri, int F, const int32_t* d_opp, float* d_grad_pos,
                               void* stream) {
    const size_t total = (size_t)B * H * W;
    if (total == 0 || C == 0) return MVE_OK;
    MVE_CHECK(d_color && d_grad_out && d_rast && d_pos && d_tri && d_opp && d_grad_pos, MVE_ERR_ARG, "antialias_backward_pos: null pointer");
    k_antialias_bwd_pos<<<mve_cdiv(total, RB), RB, 0, (hipStream_t)stream>>>(d_color, d_grad_out, B, H, W, C, d_rast, d_pos, V, d_tri, F, d_opp, d_grad_pos);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // extern "C"
