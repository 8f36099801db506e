// Per-pixel reverse-mode arithmetic of the texture path's geometry gradient (texture_grad.hip), host/device so that the CPU tests can run the
// same source (tests/texgrad_host.cpp).  Differentiates the forward formulas of texmip_core.h, nothing else:
//   tg_texture_grad_uv     d <g, dr.texture(tex, uv, uv_da)> / d uv and / d uv_da          (tm_taps, tm_level)
//   tg_attr_da_bwd         d <g, tm_attr_da(a0, a1, a2, db)> / d db and / d (a0, a1, a2)     per attribute channel
//   tg_rast_db_bwd         d <g, tm_rast_db(p0, p1, p2, b0, b1)> / d the triangle's clip (x, y, w) and / d (b0, b1)
// with the discrete choices of the forward (tap indices, level pair, the pixel's triangle) held fixed.  The derivative jumps where a tap
// index or the level pair changes; where the level is clamped (magnification, top level) it does not depend on uv_da at all.
#pragma once
#include <stddef.h>

#include "texmip_core.h"

// one level (w x h texels, C channels, base pointer p): s = <g, fetch>, du = d s / d u, dv = d s / d v (the wrap has slope 1)
MVE_TM_FN void tg_fetch_grad(const float* p, int w, int h, int C, float u, float v, const float* g, float* s, float* du, float* dv) {
    int ix[2], iy[2];
    float fu, fv;
    tm_taps(u, v, w, h, ix, iy, &fu, &fv);
    const float* r0 = p + (size_t)iy[0] * w * C;
    const float* r1 = p + (size_t)iy[1] * w * C;
    float S = 0.0f, DU = 0.0f, DV = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float a00 = r0[(size_t)ix[0] * C + c], a10 = r0[(size_t)ix[1] * C + c];
        const float a01 = r1[(size_t)ix[0] * C + c], a11 = r1[(size_t)ix[1] * C + c];
        const float top = a00 + fu * (a10 - a00), bot = a01 + fu * (a11 - a01);
        S += g[c] * (top + fv * (bot - top));
        DU += g[c] * ((1.0f - fv) * (a10 - a00) + fv * (a11 - a01));
        DV += g[c] * (bot - top);
    }
    *s = S;
    *du = DU * (float)w;
    *dv = DV * (float)h;
}

// d level / d da of tm_level; false (and zeros) where the level is clamped.  level = 1/2 log2(major), major = (A + B)/2 + sqrt((A - B)^2/4 + C^2).
// At an exactly isotropic footprint the square root is not differentiable: its term is taken as zero (the mean of the one-sided
// derivatives), i.e. 1/2 log2((A + B)/2) is differentiated there.
MVE_TM_FN bool tg_level_grad(const float* da, int tw, int th, int max_level, float* dl) {
    dl[0] = dl[1] = dl[2] = dl[3] = 0.0f;
    const float dsdx = da[0] * (float)tw, dsdy = da[1] * (float)tw, dtdx = da[2] * (float)th, dtdy = da[3] * (float)th;
    const float A = dsdx * dsdx + dtdx * dtdx, B = dsdy * dsdy + dtdy * dtdy, C = dsdx * dsdy + dtdx * dtdy;
    const float root = sqrtf(0.25f * (A - B) * (A - B) + C * C);
    const float major = 0.5f * (A + B) + root;
    const float lvl = 0.5f * log2f(major);
    if (!(lvl > 0.0f) || !(lvl < (float)max_level)) return false;
    float mA = 0.5f, mB = 0.5f, mC = 0.0f;                       // d major / d (A, B, C)
    if (root > 0.0f) {
        const float q = 0.25f * (A - B) / root;
        mA += q; mB -= q; mC = C / root;
    }
    const float k = 0.5f / (major * 0.6931471805599453f);        // d level / d major
    dl[0] = k * (2.0f * mA * dsdx + mC * dsdy) * (float)tw;
    dl[1] = k * (2.0f * mB * dsdy + mC * dsdx) * (float)tw;
    dl[2] = k * (2.0f * mA * dtdx + mC * dtdy) * (float)th;
    dl[3] = k * (2.0f * mB * dtdy + mC * dtdx) * (float)th;
    return true;
}

// tex0: level 0 of the texture this pixel reads, mips: its level stack (levels 1.. as tm_mip_offset lays them out; unused without da).
// da == NULL: filter_mode='linear' (level 0 only, g_da untouched).  g [C] -> g_uv [2], g_da [4]
MVE_TM_FN void tg_texture_grad_uv(const float* tex0, const float* mips, int H, int W, int C, int max_level, float u, float v, const float* da,
                                  const float* g, float* g_uv, float* g_da) {
    float s0, du0, dv0;
    if (!da) {
        tg_fetch_grad(tex0, W, H, C, u, v, g, &s0, &du0, &dv0);
        g_uv[0] = du0; g_uv[1] = dv0;
        return;
    }
    const TmLevel L = tm_level(da, W, H, max_level);
    const float* p0 = L.l0 == 0 ? tex0 : mips + (size_t)tm_mip_offset(H, W, L.l0) * C;
    tg_fetch_grad(p0, tm_dim(W, L.l0), tm_dim(H, L.l0), C, u, v, g, &s0, &du0, &dv0);
    g_da[0] = g_da[1] = g_da[2] = g_da[3] = 0.0f;
    if (!(L.f > 0.0f)) {                                         // one level read: clamped, or exactly on a level
        g_uv[0] = du0; g_uv[1] = dv0;
        return;
    }
    float s1, du1, dv1;
    const float* p1 = mips + (size_t)tm_mip_offset(H, W, L.l1) * C;
    tg_fetch_grad(p1, tm_dim(W, L.l1), tm_dim(H, L.l1), C, u, v, g, &s1, &du1, &dv1);
    g_uv[0] = (1.0f - L.f) * du0 + L.f * du1;
    g_uv[1] = (1.0f - L.f) * dv0 + L.f * dv1;
    float dl[4];
    if (tg_level_grad(da, W, H, max_level, dl)) {
        const float gl = s1 - s0;                                // d out / d level = fetch(l1) - fetch(l0)
        g_da[0] = gl * dl[0]; g_da[1] = gl * dl[1]; g_da[2] = gl * dl[2]; g_da[3] = gl * dl[3];
    }
}

// one attribute channel: (gx, gy) = gradient of (dA/dX, dA/dY).  g_db [4] is ADDED to; ga [3] = gradient of (a0, a1, a2)
MVE_TM_FN void tg_attr_da_bwd(float a0, float a1, float a2, const float* db, float gx, float gy, float* g_db, float* ga) {
    const float dsdu = a0 - a2, dsdv = a1 - a2;
    g_db[0] += gx * dsdu; g_db[1] += gy * dsdu; g_db[2] += gx * dsdv; g_db[3] += gy * dsdv;
    const float gu = gx * db[0] + gy * db[1], gv = gx * db[2] + gy * db[3];
    ga[0] = gu; ga[1] = gv; ga[2] = -(gu + gv);
}

// g [4] = gradient of tm_rast_db's output -> gp [3][3] = gradient of (x, y, w) of p0, p1, p2 (the direct dependence; z carries none),
// gb [2] = gradient of the stored (b0, b1)
MVE_TM_FN void tg_rast_db_bwd(const float* p0, const float* p1, const float* p2, float b0, float b1, int px, int py, int W, int H, const float* g,
                              float* gp, float* gb) {
    const float xs = 2.0f / (float)W, ys = 2.0f / (float)H, xo = 1.0f / (float)W - 1.0f, yo = 1.0f / (float)H - 1.0f;
    const float fx = xs * (float)px + xo, fy = ys * (float)py + yo;
    const float x[3] = {p0[0], p1[0], p2[0]}, y[3] = {p0[1], p1[1], p2[1]}, w[3] = {p0[3], p1[3], p2[3]};
    float qx[3], qy[3];
    for (int k = 0; k < 3; ++k) { qx[k] = x[k] - fx * w[k]; qy[k] = y[k] - fy * w[k]; }
    const float a0 = qx[1] * qy[2] - qy[1] * qx[2], a1 = qx[2] * qy[0] - qy[2] * qx[0], a2 = qx[0] * qy[1] - qy[0] * qx[1];
    const float iw = 1.0f / (a0 + a1 + a2);
    const float dfxdx = xs * iw, dfydy = ys * iw;
    float dadx[3], dady[3];
    for (int k = 0; k < 3; ++k) {
        const int i1 = (k + 1) % 3, i2 = (k + 2) % 3;
        dadx[k] = y[i2] * w[i1] - y[i1] * w[i2];
        dady[k] = x[i1] * w[i2] - x[i2] * w[i1];
    }
    const float datdx = dadx[0] + dadx[1] + dadx[2], datdy = dady[0] + dady[1] + dady[2];
    const float t0 = b0 * datdx - dadx[0], t1 = b0 * datdy - dady[0], t2 = b1 * datdx - dadx[1], t3 = b1 * datdy - dady[1];
    const float g_t0 = g[0] * dfxdx, g_t1 = g[1] * dfydy, g_t2 = g[2] * dfxdx, g_t3 = g[3] * dfydy;
    gb[0] = g_t0 * datdx + g_t1 * datdy;
    gb[1] = g_t2 * datdx + g_t3 * datdy;
    const float g_datdx = g_t0 * b0 + g_t2 * b1, g_datdy = g_t1 * b0 + g_t3 * b1;
    const float g_dadx[3] = {g_datdx - g_t0, g_datdx - g_t2, g_datdx}, g_dady[3] = {g_datdy - g_t1, g_datdy - g_t3, g_datdy};
    const float g_iw = xs * (g[0] * t0 + g[2] * t2) + ys * (g[1] * t1 + g[3] * t3);
    const float g_sum = -g_iw * iw * iw;                          // gradient of a0 + a1 + a2
    float gx[3] = {0.0f, 0.0f, 0.0f}, gy[3] = {0.0f, 0.0f, 0.0f}, gw[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3; ++k) {
        const int i1 = (k + 1) % 3, i2 = (k + 2) % 3;
        gy[i2] += g_dadx[k] * w[i1]; gw[i1] += g_dadx[k] * y[i2];
        gy[i1] -= g_dadx[k] * w[i2]; gw[i2] -= g_dadx[k] * y[i1];
        gx[i1] += g_dady[k] * w[i2]; gw[i2] += g_dady[k] * x[i1];
        gx[i2] -= g_dady[k] * w[i1]; gw[i1] -= g_dady[k] * x[i2];
        // a_k = qx[i1] qy[i2] - qy[i1] qx[i2], q = (x - fx w, y - fy w)
        const float hx1 = g_sum * qy[i2], hy2 = g_sum * qx[i1], hy1 = -g_sum * qx[i2], hx2 = -g_sum * qy[i1];
        gx[i1] += hx1; gw[i1] -= fx * hx1;
        gy[i2] += hy2; gw[i2] -= fy * hy2;
        gy[i1] += hy1; gw[i1] -= fy * hy1;
        gx[i2] += hx2; gw[i2] -= fx * hx2;
    }
    for (int k = 0; k < 3; ++k) { gp[3 * k] = gx[k]; gp[3 * k + 1] = gy[k]; gp[3 * k + 2] = gw[k]; }
}
