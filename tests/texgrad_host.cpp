// Host build of mvedit_amd/csrc/texgrad_core.h for tests/test_nvdr_core_cpu.py: the per-pixel bodies of the kernels of
// mvedit_amd/csrc/texture_grad.hip, looped sequentially in fp32 (atomics become plain adds).  Built by tests/nvdr_chain.py into a temporary directory.
#include <stdint.h>

#include "texgrad_core.h"

extern "C" {

// tex0 [Bt,H,W,C], mips [Bt, mip_texels * C] (or NULL), uv [n,npix,2], da [n,npix,4] or NULL, g [n,npix,C] -> g_uv [n,npix,2], g_da [n,npix,4]
void th_texture_grad_uv(const float* tex0, const float* mips, int Bt, int H, int W, int C, int max_level, const float* uv, const float* da,
                        const float* g, int n, int npix, float* g_uv, float* g_da) {
    const size_t ts = Bt == 1 ? 0 : (size_t)H * W * C, ms = Bt == 1 ? 0 : (size_t)tm_mip_offset(H, W, max_level + 1) * C;
    for (size_t i = 0; i < (size_t)n * npix; ++i) {
        const size_t b = i / npix;
        float gda[4] = {0.f, 0.f, 0.f, 0.f};
        tg_texture_grad_uv(tex0 + b * ts, mips ? mips + b * ms : nullptr, H, W, C, max_level, uv[2 * i], uv[2 * i + 1], da ? da + 4 * i : nullptr,
                           g + i * C, g_uv + 2 * i, gda);
        if (g_da) for (int k = 0; k < 4; ++k) g_da[4 * i + k] = gda[k];
    }
}

// attr [Ba,V,C], rast / rast_db [B,npix,4], g_da [B,npix,2C] -> g_db [B,npix,4] (written), g_attr [Ba,V,C] (added to)
void th_interpolate_da_backward(const float* attr, int Ba, int V, int C, const float* rast, const float* rast_db, int B, int npix, const int32_t* tri,
                                int F, const float* g_da, float* g_db, float* g_attr) {
    for (size_t i = 0; i < (size_t)B * npix; ++i) {
        float* o = g_db + 4 * i;
        o[0] = o[1] = o[2] = o[3] = 0.f;
        const int id = (int)rast[4 * i + 3] - 1;
        if (id < 0 || id >= F) continue;
        const size_t ao = Ba == 1 ? 0 : (i / npix) * (size_t)V * C;
        const int vi[3] = {tri[3 * id], tri[3 * id + 1], tri[3 * id + 2]};
        for (int c = 0; c < C; ++c) {
            float ga[3];
            tg_attr_da_bwd(attr[ao + (size_t)vi[0] * C + c], attr[ao + (size_t)vi[1] * C + c], attr[ao + (size_t)vi[2] * C + c], rast_db + 4 * i,
                           g_da[i * 2 * C + 2 * c], g_da[i * 2 * C + 2 * c + 1], o, ga);
            for (int k = 0; k < 3; ++k) g_attr[ao + (size_t)vi[k] * C + c] += ga[k];
        }
    }
}

// pos [B,V,4], rast [B,H,W,4], g_db [B,H,W,4] -> g_pos [B,V,4] (added to), g_rast [B,H,W,4] (written)
void th_rasterize_db_backward(const float* pos, int B, int V, const int32_t* tri, int F, const float* rast, int H, int W, const float* g_db,
                              float* g_pos, float* g_rast) {
    for (size_t i = 0; i < (size_t)B * H * W; ++i) {
        float* o = g_rast + 4 * i;
        o[0] = o[1] = o[2] = o[3] = 0.f;
        const int id = (int)rast[4 * i + 3] - 1;
        if (id < 0 || id >= F) continue;
        const size_t b = i / ((size_t)H * W);
        const int pix = (int)(i - b * (size_t)H * W), py = pix / W, px = pix - py * W;
        const float* pb = pos + b * (size_t)V * 4;
        const int vi[3] = {tri[3 * id], tri[3 * id + 1], tri[3 * id + 2]};
        float gp[9], gb[2];
        tg_rast_db_bwd(pb + 4 * (size_t)vi[0], pb + 4 * (size_t)vi[1], pb + 4 * (size_t)vi[2], rast[4 * i], rast[4 * i + 1], px, py, W, H, g_db + 4 * i, gp, gb);
        o[0] = gb[0]; o[1] = gb[1];
        for (int k = 0; k < 3; ++k) {
            float* d = g_pos + (b * (size_t)V + vi[k]) * 4;
            d[0] += gp[3 * k]; d[1] += gp[3 * k + 1]; d[3] += gp[3 * k + 2];
        }
    }
}

}  // extern "C"
