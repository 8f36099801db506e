"""mvedit_amd/csrc/texgrad_core.h -- the per-pixel reverse-mode arithmetic of mve_texture_grad_uv, mve_interpolate_da_backward and
mve_rasterize_db_backward -- compiled for the HOST (tests/texgrad_host.cpp, fp32, sequential) against float64 torch autograd over the oracle
pieces (oracle/texture_mip_oracle.py), per function.  No GPU: the device arithmetic itself is checked here; what is left for the GPU tests is
the launch geometry and the atomics.

Bar (the convention of test_mesh_ops.py::test_mip_texture_kernels_vs_oracle): float64 evaluation of the same formulas is the truth; the fp32
source may be no further from it than a few times the fp32 TORCH evaluation is:  e_host <= 4 e_f32 + 1e-6 scale  (max-abs)."""
import math

import numpy as np
import pytest
import torch

import nvdr_chain as NC
from oracle import texture_mip_oracle as TM


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return NC.build_texgrad_host(tmp_path_factory.mktemp('texgrad_host'))


def _bar(name, got, want64, f32):
    scale = want64.abs().max().item()
    e_host, e_f32 = (got.double() - want64).abs().max().item(), (f32.double() - want64).abs().max().item()
    print(f'{name}: e_host {e_host:.3e}  e_f32 {e_f32:.3e}  scale {scale:.3e}')
    assert scale > 0 and np.isfinite(e_host) and e_host <= 4 * e_f32 + 1e-6 * scale, (name, e_host, e_f32, scale)


def _texture_inputs(bt, n=2, S=48, T=64, C=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    tex = torch.rand(bt, T, T, C, generator=g)
    uv = torch.rand(n, S, S, 2, generator=g) * 3 - 1                             # wraps on both sides
    # footprints from well inside one texel (magnification: level clamped to 0) to beyond the whole texture (clamped to the top level)
    s = torch.exp(torch.rand(n, S, S, 1, generator=g) * (math.log(200.0) - math.log(0.1)) + math.log(0.1)) / T
    uv_da = torch.randn(n, S, S, 4, generator=g) * s
    return tex, uv, uv_da, torch.randn(n, S, S, C, generator=g)


def _texture_autograd(tex, uv, uv_da, g, dtype, filt):
    u = uv.detach().to(dtype).clone().requires_grad_(True)
    d = uv_da.detach().to(dtype).clone().requires_grad_(True) if filt == 'linear-mipmap-linear' else None
    out = TM.texture(tex.to(dtype), u, d, filter_mode=filt)
    (out * g.to(dtype)).sum().backward()
    return u.grad, None if d is None else d.grad


@pytest.mark.parametrize('bt', [1, 2])
@pytest.mark.parametrize('filt', ['linear', 'linear-mipmap-linear'])
def test_texture_grad_uv_vs_float64_autograd(host, filt, bt):
    tex, uv, uv_da, g = _texture_inputs(bt)
    mip = filt == 'linear-mipmap-linear'
    T = tex.shape[1]
    maxl = NC.mip_levels(T, T)
    ex = NC.excused(uv, uv_da, T, T, maxl, mip)
    share = ex.float().mean().item()
    print(f'excused {share:.4f}')
    assert share <= 0.02
    g = g * (~ex)[..., None]
    if mip:                  # the cases are all there: clamped below, clamped above, and between
        lvl = NC.unclamped_level(uv_da.double(), T, T)
        assert (lvl <= 0).float().mean() > 0.05 and (lvl >= maxl).float().mean() > 0.02 and ((lvl > 0) & (lvl < maxl)).float().mean() > 0.5
    want_uv, want_da = _texture_autograd(tex, uv, uv_da, g, torch.float64, filt)
    f32_uv, f32_da = _texture_autograd(tex, uv, uv_da, g, torch.float32, filt)
    got_uv, got_da = NC.host_texture_grad_uv(host, tex, uv, uv_da if mip else None, g)
    _bar('d/d uv', got_uv, want_uv, f32_uv)
    if mip:
        assert torch.isfinite(got_da).all()
        _bar('d/d uv_da', got_da, want_da, f32_da)
        clamped = (lvl <= 0) | (lvl >= maxl)
        assert (got_da[clamped] == 0).all() and (want_da[clamped] == 0).all()        # no dependence on uv_da where the level is clamped


def test_texture_grad_uv_at_the_isotropic_footprint(host):
    """uv_da = (s, 0, 0, s): (A - B)^2/4 + C^2 = 0 and the square root is not differentiable (torch autograd over the oracle returns NaN
    there).  The rule: its term is zero, i.e. 1/2 log2((A + B)/2) is differentiated: d level / d uv_da = (1, 0, 0, 1) / (2 s ln 2).  Compared with
    that closed form (fetch difference from the oracle in float64), and finite."""
    g_ = torch.Generator().manual_seed(5)
    T, C, n, S = 64, 3, 1, 32
    tex = torch.rand(1, T, T, C, generator=g_)
    uv = torch.rand(n, S, S, 2, generator=g_)
    s = torch.exp(torch.rand(n, S, S, generator=g_) * math.log(16.0)) * 1.5 / T            # levels log2(1.5) .. log2(24): all unclamped
    uv_da = torch.stack([s, torch.zeros_like(s), torch.zeros_like(s), s], dim=-1)
    g = torch.randn(n, S, S, C, generator=g_)
    maxl = NC.mip_levels(T, T)
    ex = NC.excused(uv, uv_da, T, T, maxl, True)
    assert ex.float().mean().item() <= 0.02
    g = g * (~ex)[..., None]
    # autograd really is NaN here
    d = uv_da.double().requires_grad_(True)
    (TM.texture(tex.double(), uv.double(), d) * g.double()).sum().backward()
    assert torch.isnan(d.grad).any()

    def closed_form(dtype):
        levels = TM.build_mips(tex.to(dtype))
        l0, l1, fr = TM.mip_level(uv_da.to(dtype).reshape(-1, 4), T, T, maxl)
        bsel = torch.zeros(l0.numel(), dtype=torch.long)
        f0, f1 = torch.zeros(l0.numel(), C, dtype=dtype), torch.zeros(l0.numel(), C, dtype=dtype)
        for l in range(maxl + 1):
            if (l0 == l).any():
                f0[l0 == l] = TM._bilinear_wrap(levels[l], bsel[l0 == l], uv.to(dtype).reshape(-1, 2)[l0 == l])
            if (l1 == l).any():
                f1[l1 == l] = TM._bilinear_wrap(levels[l], bsel[l1 == l], uv.to(dtype).reshape(-1, 2)[l1 == l])
        gl = ((f1 - f0) * g.to(dtype).reshape(-1, C)).sum(-1).reshape(n, S, S)
        k = gl / (2 * s.to(dtype) * math.log(2.0))
        return torch.stack([k, torch.zeros_like(k), torch.zeros_like(k), k], dim=-1)
    got_uv, got_da = NC.host_texture_grad_uv(host, tex, uv, uv_da, g)
    assert torch.isfinite(got_da).all() and torch.isfinite(got_uv).all()
    _bar('isotropic d/d uv_da', got_da, closed_form(torch.float64), closed_form(torch.float32))


def _raster_scene(H=24, W=32):
    from oracle import raster as RO
    from scene import face_atlas, icosphere
    v, f = icosphere(2, 0.6)
    vt, ft = face_atlas(f)
    pos = NC.clip_views(v)
    tri = torch.from_numpy(f.astype(np.int32))
    rast = torch.from_numpy(np.asarray(RO.rasterize(pos.numpy(), f, (H, W))))
    assert (rast[..., 3] > 0).sum() > 200
    return pos, tri, torch.from_numpy(vt)[None], torch.from_numpy(ft.astype(np.int32)), rast


@pytest.mark.parametrize('per_view', [False, True])
def test_interpolate_da_backward_vs_float64_autograd(host, per_view):
    pos, tri, vt, ft, rast = _raster_scene()
    g_ = torch.Generator().manual_seed(1)
    db = TM.rasterize_db(pos, tri, rast)
    attr = torch.cat([vt, torch.randn(1, vt.shape[1], 1, generator=g_)], dim=-1)            # the atlas coordinates and one more channel
    if per_view:
        attr = attr.expand(pos.shape[0], -1, -1) + 0.1 * torch.randn(pos.shape[0], vt.shape[1], 3, generator=g_)
    g_da = torch.randn(*rast.shape[:3], 6, generator=g_)

    def autograd(dtype):
        a, d = attr.detach().to(dtype).clone().requires_grad_(True), db.detach().to(dtype).clone().requires_grad_(True)
        (TM.interpolate_da(a, rast.to(dtype), d, ft) * g_da.to(dtype)).sum().backward()
        return d.grad, a.grad
    want_db, want_attr = autograd(torch.float64)
    f32_db, f32_attr = autograd(torch.float32)
    got_db, got_attr = NC.host_interpolate_da_backward(host, attr, rast, db, ft, g_da)
    _bar('d/d rast_db', got_db, want_db, f32_db)
    _bar('d/d attr', got_attr, want_attr, f32_attr)
    assert (got_db[rast[..., 3] == 0] == 0).all()


def test_rasterize_db_backward_vs_float64_autograd(host):
    pos, tri, vt, ft, rast = _raster_scene()
    g_db = torch.randn(rast.shape, generator=torch.Generator().manual_seed(2))

    def autograd(dtype):
        p, r = pos.detach().to(dtype).clone().requires_grad_(True), rast.detach().to(dtype).clone().requires_grad_(True)
        (TM.rasterize_db(p, tri, r) * g_db.to(dtype)).sum().backward()
        return p.grad, r.grad
    want_pos, want_rast = autograd(torch.float64)
    f32_pos, f32_rast = autograd(torch.float32)
    got_pos, got_rast = NC.host_rasterize_db_backward(host, pos, tri, rast, g_db)
    assert (want_rast[..., 2:] == 0).all() and (got_rast[..., 2:] == 0).all()
    _bar('d/d (b0, b1)', got_rast, want_rast, f32_rast)
    _bar('d/d pos (direct)', got_pos, want_pos, f32_pos)
    assert (got_pos[..., 2] == 0).all()                                                     # clip z does not enter rast_db
