// Geometry gradient of the texture path (gfx950): from a texture fetch back to the texture coordinates, and from there through the second
// outputs of dr.interpolate and dr.rasterize to the attributes and the clip-space vertices -- what nvdiffrast propagates when a textured mesh
// is optimised and mvedit_amd.nvdiffrast.torch provides:
//   mve_texture_grad_uv          d dr.texture / d uv and (linear-mipmap-linear) / d uv_da: one lane per pixel, gathers only
//   mve_interpolate_da_backward  d interpolate(...)[1] / d rast_db (per pixel) and / d attr (float atomics, ADDED into the caller's buffer)
//   mve_rasterize_db_backward    d rasterize(...)[1] / d pos (float atomics, ADDED) and / d the stored (b0, b1) (per pixel)
// Every kernel is an HBM / gather-latency bound per-pixel pass.  Arithmetic in texgrad_core.h (host/device; the CPU tests run a host build of
// it against float64 autograd over oracle/texture_mip_oracle.py).
#include "common.h"

#include "texgrad_core.h"

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void k_texture_grad_uv(const float* __restrict__ tex0, const float* __restrict__ mips, size_t tex_stride,
                                                        size_t mip_stride, int H, int W, int C, int max_level, const float* __restrict__ uv,
                                                        const float* __restrict__ uv_da, const float* __restrict__ g_out, size_t total,
                                                        size_t npix, float* __restrict__ g_uv, float* __restrict__ g_da) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const size_t n = i / npix;
    float da[4], guv[2] = {0.f, 0.f}, gda[4] = {0.f, 0.f, 0.f, 0.f};
    if (uv_da) {
        const f32x4 d4 = reinterpret_cast<const f32x4*>(uv_da)[i];
        da[0] = d4[0]; da[1] = d4[1]; da[2] = d4[2]; da[3] = d4[3];
    }
    tg_texture_grad_uv(tex0 + n * tex_stride, mips ? mips + n * mip_stride : nullptr, H, W, C, max_level, uv[2 * i], uv[2 * i + 1],
                       uv_da ? da : nullptr, g_out + i * C, guv, gda);
    if (g_uv) { g_uv[2 * i] = guv[0]; g_uv[2 * i + 1] = guv[1]; }
    if (g_da) reinterpret_cast<f32x4*>(g_da)[i] = f32x4{gda[0], gda[1], gda[2], gda[3]};
}

__global__ __launch_bounds__(NT) void k_interpolate_da_bwd(const float* __restrict__ attr, size_t attr_stride, int V, int C,
                                                           const float* __restrict__ rast, const float* __restrict__ rast_db, size_t total,
                                                           size_t npix, const int32_t* __restrict__ tri, int F, const float* __restrict__ g_da,
                                                           float* __restrict__ g_db, float* __restrict__ g_attr) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const f32x4 r = reinterpret_cast<const f32x4*>(rast)[i];
    const int id = (int)r[3] - 1;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (id >= 0 && id < F) {
        const int i0 = tri[3 * id], i1 = tri[3 * id + 1], i2 = tri[3 * id + 2];
        if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
            const f32x4 db4 = reinterpret_cast<const f32x4*>(rast_db)[i];
            const float db[4] = {db4[0], db4[1], db4[2], db4[3]};
            const size_t ao = (i / npix) * attr_stride;
            const float* g = g_da + i * 2 * C;
            float gdb[4] = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < C; ++c) {
                float ga[3];
                tg_attr_da_bwd(attr[ao + (size_t)i0 * C + c], attr[ao + (size_t)i1 * C + c], attr[ao + (size_t)i2 * C + c], db, g[2 * c],
                               g[2 * c + 1], gdb, ga);
                if (g_attr) {
                    atomicAdd(g_attr + ao + (size_t)i0 * C + c, ga[0]);
                    atomicAdd(g_attr + ao + (size_t)i1 * C + c, ga[1]);
                    atomicAdd(g_attr + ao + (size_t)i2 * C + c, ga[2]);
                }
            }
            o = f32x4{gdb[0], gdb[1], gdb[2], gdb[3]};
        }
    }
    if (g_db) reinterpret_cast<f32x4*>(g_db)[i] = o;
}

__global__ __launch_bounds__(NT) void k_rasterize_db_bwd(const float* __restrict__ pos, int V, const int32_t* __restrict__ tri, int F,
                                                         const float* __restrict__ rast, int B, int H, int W, const float* __restrict__ g_db,
                                                         float* __restrict__ g_pos, float* __restrict__ g_rast) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (size_t)B * H * W) return;
    const f32x4 r = reinterpret_cast<const f32x4*>(rast)[i];
    const int id = (int)r[3] - 1;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (id >= 0 && id < F) {
        const int i0 = tri[3 * id], i1 = tri[3 * id + 1], i2 = tri[3 * id + 2];
        if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
            const size_t b = i / ((size_t)H * W);
            const int pix = (int)(i - b * (size_t)H * W), py = pix / W, px = pix - py * W;
            const float* pb = pos + b * (size_t)V * 4;
            const f32x4 g4 = reinterpret_cast<const f32x4*>(g_db)[i];
            const float g[4] = {g4[0], g4[1], g4[2], g4[3]};
            float gp[9], gb[2];
            tg_rast_db_bwd(pb + 4 * (size_t)i0, pb + 4 * (size_t)i1, pb + 4 * (size_t)i2, r[0], r[1], px, py, W, H, g, gp, gb);
            o[0] = gb[0]; o[1] = gb[1];
            if (g_pos) {
                float* gpb = g_pos + b * (size_t)V * 4;
                const int vi[3] = {i0, i1, i2};
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    float* d = gpb + 4 * (size_t)vi[k];
                    atomicAdd(d, gp[3 * k]); atomicAdd(d + 1, gp[3 * k + 1]); atomicAdd(d + 3, gp[3 * k + 2]);
                }
            }
        }
    }
    if (g_rast) reinterpret_cast<f32x4*>(g_rast)[i] = o;
}

}  // namespace

extern "C" {

int mve_texture_grad_uv(const float* d_tex0, const float* d_mips, int Bt, int H, int W, int C, int max_level, const float* d_uv,
                        const float* d_uv_da, const float* d_g_out, int n, int h, int w, float* d_g_uv, float* d_g_uv_da, void* stream) {
    const size_t total = (size_t)n * h * w;
    if (total == 0) return MVE_OK;
    MVE_CHECK(Bt > 0 && H > 0 && W > 0 && C > 0 && (Bt == 1 || Bt == n), MVE_ERR_ARG, "texture_grad_uv: bad texture shape [%d,%d,%d,%d] for %d images",
              Bt, H, W, C, n);
    MVE_CHECK(d_tex0 && d_uv && d_g_out && (d_g_uv || d_g_uv_da), MVE_ERR_ARG, "texture_grad_uv: null pointer");
    if (d_uv_da) {
        MVE_CHECK(max_level >= 0 && max_level <= 30 && (d_mips || max_level == 0), MVE_ERR_ARG, "texture_grad_uv: bad max_level %d or no level stack", max_level);
        for (int l = 0; l < max_level; ++l) {
            const int hl = tm_dim(H, l), wl = tm_dim(W, l);
            MVE_CHECK((hl == 1 || hl % 2 == 0) && (wl == 1 || wl % 2 == 0), MVE_ERR_ARG, "texture_grad_uv: mip level %d of a %dx%d texture has an odd extent",
                      l + 1, H, W);
        }
    } else {
        MVE_CHECK(!d_g_uv_da, MVE_ERR_ARG, "texture_grad_uv: a gradient w.r.t. uv_da needs uv_da");
    }
    const size_t ts = Bt == 1 ? 0 : (size_t)H * W * C, ms = Bt == 1 ? 0 : (size_t)tm_mip_offset(H, W, max_level + 1) * C;
    k_texture_grad_uv<<<mve_cdiv(total, NT), NT, 0, (hipStream_t)stream>>>(d_tex0, d_uv_da ? d_mips : nullptr, ts, ms, H, W, C, max_level, d_uv, d_uv_da,
                                                                          d_g_out, total, (size_t)h * w, d_g_uv, d_g_uv_da);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_interpolate_da_backward(const float* d_attr, int attr_batch, int V, int C, const float* d_rast, const float* d_rast_db, int B, int npix,
                                const int32_t* d_tri, int F, const float* d_g_da, float* d_g_rast_db, float* d_g_attr, void* stream) {
    const size_t total = (size_t)B * npix;
    if (total == 0 || C == 0) return MVE_OK;
    MVE_CHECK(d_attr && d_rast && d_rast_db && d_tri && d_g_da && (d_g_rast_db || d_g_attr), MVE_ERR_ARG, "interpolate_da_backward: null pointer");
    MVE_CHECK(V > 0 && C > 0 && (attr_batch == 1 || attr_batch == B), MVE_ERR_ARG, "interpolate_da_backward: attribute batch %d vs %d images", attr_batch, B);
    k_interpolate_da_bwd<<<mve_cdiv(total, NT), NT, 0, (hipStream_t)stream>>>(d_attr, attr_batch == 1 ? 0 : (size_t)V * C, V, C, d_rast, d_rast_db, total,
                                                                             (size_t)npix, d_tri, F, d_g_da, d_g_rast_db, d_g_attr);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

int mve_rasterize_db_backward(const float* d_pos, int B, int V, const int32_t* d_tri, int F, const float* d_rast, int H, int W, const float* d_g_db,
                              float* d_g_pos, float* d_g_rast, void* stream) {
    const size_t total = (size_t)B * H * W;
    if (total == 0) return MVE_OK;
    MVE_CHECK(d_pos && d_tri && d_rast && d_g_db && (d_g_pos || d_g_rast), MVE_ERR_ARG, "rasterize_db_backward: null pointer");
    MVE_CHECK(V > 0 && F >= 0, MVE_ERR_ARG, "rasterize_db_backward: bad mesh (%d vertices, %d triangles)", V, F);
    k_rasterize_db_bwd<<<mve_cdiv(total, NT), NT, 0, (hipStream_t)stream>>>(d_pos, V, d_tri, F, d_rast, B, H, W, d_g_db, d_g_pos, d_g_rast);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

}  // extern "C"
