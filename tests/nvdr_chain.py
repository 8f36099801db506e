"""Test helpers of the nvdiffrast.torch facade (tests/test_nvdr_*.py): the float64 reference chain, the excusal mask, the scenes and the host
build of mvedit_amd/csrc/texgrad_core.h.

"The gradient" of the facade is the derivative of this repository's own forward formulas as torch autograd computes it over the committed
oracle, with every pixel's triangle held fixed:

    u, v (pos)                oracle/raster_grad_oracle.py::rast_continuous
    rast_db (pos, u, v)       oracle/texture_mip_oracle.py::rasterize_db
    interpolate               u a0 + v a1 + (1 - u - v) a2
    attr_da (attr, rast_db)   oracle/texture_mip_oracle.py::interpolate_da
    texture (tex, uv, uv_da)  oracle/texture_mip_oracle.py::texture

The rasteriser snaps vertices to 1/256 pixel, so the stored (u, v) differ from the continuous model by up to 2e-2; the chain is evaluated at
the STORED values with the continuous model's gradient: u = u_stored + (u_cont - u_cont.detach())."""
import ctypes
import math
import os
import subprocess

import numpy as np
import torch

from oracle import raster_grad_oracle as R
from oracle import texture_mip_oracle as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ scenes
def clip_views(v, angles=(0.3, 1.1)):
    """The clip transforms of test_mesh_grad._scene for vertices v [V,3] -> pos [len(angles), V, 4] float32."""
    pos = torch.from_numpy(np.asarray(v)).float()

    def clip(ang):
        c, s = math.cos(ang), math.sin(ang)
        rot = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float32)
        p = pos @ rot.T
        z = p[:, 2] + 2.5
        return torch.stack([p[:, 0] * 2.0, p[:, 1] * 2.0, (z - 2.5) * 0.5, z], dim=-1)
    return torch.stack([clip(a) for a in angles])


def sphere_scene(S, atlas, subdiv=3, channels=3, seed=0):
    """icosphere(subdiv, 0.6) with face_atlas, two views, a random texture and a random g_out -> dict of CPU float32 / int32 tensors."""
    from scene import face_atlas, icosphere
    v, f = icosphere(subdiv, 0.6)
    vt, ft = face_atlas(f)
    g = torch.Generator().manual_seed(seed)
    pos = clip_views(v)
    return dict(pos=pos, tri=torch.from_numpy(f.astype(np.int32)), vt=torch.from_numpy(vt)[None], ft=torch.from_numpy(ft.astype(np.int32)),
                tex=torch.rand(1, atlas, atlas, channels, generator=g), g_out=torch.randn(pos.shape[0], S, S, channels, generator=g), S=S)


# ------------------------------------------------------------------------------------------------------------------ the chain
def interpolate(attr, rast, tri):
    """u a0 + v a1 + (1 - u - v) a2; attr [1 or B, V, A]; zeros on empty pixels."""
    B, H, W, _ = rast.shape
    ids = rast[..., 3].long() - 1
    t = tri.long()[ids.clamp(min=0)]
    at = attr.expand(B, -1, -1)
    bi = torch.arange(B)[:, None, None, None].expand(-1, H, W, 3)
    a = at[bi, t]                                                              # [B,H,W,3,A]
    u, v = rast[..., 0:1], rast[..., 1:2]
    out = u * a[..., 0, :] + v * a[..., 1, :] + (1 - u - v) * a[..., 2, :]
    return torch.where((ids >= 0)[..., None], out, torch.zeros_like(out))


def rast_with_continuous_gradient(pos, tri, rast_stored):
    """rast [B,H,W,4] holding the stored (u, v, z/w, id + 1) as values and the continuous model's dependence on pos as gradient."""
    B, H, W, _ = rast_stored.shape
    rs = rast_stored.to(pos.dtype)
    ids = rs[..., 3].long() - 1
    b, yy, xx = torch.nonzero(ids >= 0, as_tuple=True)
    uc, vc, zc = R.rast_continuous(pos, tri, b, ids[b, yy, xx], xx, yy, H, W)
    cols = [rs[b, yy, xx, 0] + (uc - uc.detach()), rs[b, yy, xx, 1] + (vc - vc.detach()), rs[b, yy, xx, 2] + (zc - zc.detach()), rs[b, yy, xx, 3]]
    rast = torch.zeros(B, H, W, 4, dtype=pos.dtype)
    return rast.index_put((b, yy, xx), torch.stack(cols, dim=-1))


def chain(pos, tri, vt, ft, tex, rast_stored, filter_mode):
    """pos, vt, tex (any float dtype, may require grad) -> dict(out [B,H,W,C], rast, rast_db, uv, uv_da) of the whole reference chain."""
    rast = rast_with_continuous_gradient(pos, tri, rast_stored)
    db = TM.rasterize_db(pos, tri, rast)
    uv = interpolate(vt, rast, ft)
    da = TM.interpolate_da(vt, rast, db, ft)
    mip = filter_mode == 'linear-mipmap-linear'
    out = TM.texture(tex, uv, da if mip else None, filter_mode=filter_mode)
    return dict(out=out, rast=rast, rast_db=db, uv=uv, uv_da=da)


def chain_gradients(sc, rast_stored, filter_mode, g_out, dtype):
    """d <chain, g_out> / d (pos, vt, tex) by torch autograd in `dtype` -> (grads dict, forward dict)."""
    pos, vt, tex = (sc[k].detach().to(dtype).clone().requires_grad_(True) for k in ('pos', 'vt', 'tex'))
    fw = chain(pos, sc['tri'], vt, sc['ft'], tex, rast_stored, filter_mode)
    (fw['out'] * g_out.to(dtype)).sum().backward()
    return dict(pos=pos.grad, vt=vt.grad, tex=tex.grad), {k: v.detach() for k, v in fw.items()}


# ------------------------------------------------------------------------------------------------------------------ excusal
def unclamped_level(uv_da, tex_h, tex_w):
    dsdx, dsdy, dtdx, dtdy = uv_da[..., 0] * tex_w, uv_da[..., 1] * tex_w, uv_da[..., 2] * tex_h, uv_da[..., 3] * tex_h
    A, B, C = dsdx * dsdx + dtdx * dtdx, dsdy * dsdy + dtdy * dtdy, dsdx * dsdy + dtdx * dtdy
    return 0.5 * torch.log2(0.5 * (A + B) + torch.sqrt(0.25 * (A - B) * (A - B) + C * C))


def excused(uv, uv_da, tex_h, tex_w, max_level, mip, tol=1e-3):
    """The derivative jumps where a bilinear tap index or the level pair changes.  A pixel is excused when, in the float64 forward,
    frac(u) w_l - 1/2 or frac(v) h_l - 1/2 is within `tol` of an integer at either level it reads, or its unclamped level is within `tol` of an
    integer in [0, max_level].  uv [..., 2], uv_da [..., 4] float64 -> bool [...]"""
    uv, uv_da = uv.double(), None if uv_da is None else uv_da.double()
    near = lambda x: (x - torch.round(x)).abs() < tol
    fu, fv = uv[..., 0] - torch.floor(uv[..., 0]), uv[..., 1] - torch.floor(uv[..., 1])
    taps = lambda l: near(fu * max(tex_w >> l, 1) - 0.5) | near(fv * max(tex_h >> l, 1) - 0.5)
    if not mip:
        return taps(0)
    lvl = unclamped_level(uv_da, tex_h, tex_w)
    l0, l1, fr = TM.mip_level(uv_da, tex_h, tex_w, max_level)
    ex = near(lvl) & (lvl > -tol) & (lvl < max_level + tol)
    for l in range(max_level + 1):
        ex = ex | (((l0 == l) | ((l1 == l) & (fr > 0))) & taps(l))
    return ex


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def mip_levels(H, W):
    l = 0
    while (max(H >> l, 1) | max(W >> l, 1)) > 1:
        l += 1
    return l


# ------------------------------------------------------------------------------------------------------------------ host build of the core header
_F, _I, _P = ctypes.c_float, ctypes.c_int, ctypes.c_void_p


def build_texgrad_host(tmp_dir):
    """g++ build of tests/texgrad_host.cpp (the product's texgrad_core.h, fp32, no contraction) -> ctypes library."""
    so = os.path.join(str(tmp_dir), 'libtexgrad_host.so')
    cmd = ['g++', '-O2', '-ffp-contract=off', '-std=c++17', '-shared', '-fPIC', '-I' + os.path.join(ROOT, 'mvedit_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'texgrad_host.cpp'), '-o', so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.th_texture_grad_uv.argtypes = [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _I, _I, _P, _P]
    lib.th_interpolate_da_backward.argtypes = [_P, _I, _I, _I, _P, _P, _I, _I, _P, _I, _P, _P, _P]
    lib.th_rasterize_db_backward.argtypes = [_P, _I, _I, _P, _I, _P, _I, _I, _P, _P, _P]
    for f in (lib.th_texture_grad_uv, lib.th_interpolate_da_backward, lib.th_rasterize_db_backward):
        f.restype = None
    return lib


def _np(t, dt=np.float32):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dt)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_P)


def flat_mips(tex):
    """levels 1.. of oracle build_mips in the layout of mve_mip_build: [Bt, mip_texels * C] float32 (computed in float32)."""
    lv = TM.build_mips(tex.float())
    if len(lv) == 1:
        return None, 0
    return torch.cat([l.reshape(tex.shape[0], -1) for l in lv[1:]], dim=1).contiguous(), len(lv) - 1


def host_texture_grad_uv(lib, tex, uv, uv_da, g):
    """tex [Bt,H,W,C], uv [n,h,w,2], uv_da [n,h,w,4] or None, g [n,h,w,C] -> (g_uv, g_da or None) float32 tensors."""
    Bt, H, W, C = tex.shape
    n, h, w, _ = uv.shape
    mips, lv = flat_mips(tex) if uv_da is not None else (None, 0)
    a = [_np(tex), _np(mips), _np(uv), _np(uv_da), _np(g)]
    g_uv, g_da = np.zeros((n, h, w, 2), np.float32), (np.zeros((n, h, w, 4), np.float32) if uv_da is not None else None)
    lib.th_texture_grad_uv(_ptr(a[0]), _ptr(a[1]), Bt, H, W, C, lv, _ptr(a[2]), _ptr(a[3]), _ptr(a[4]), n, h * w, _ptr(g_uv), _ptr(g_da))
    return torch.from_numpy(g_uv), None if g_da is None else torch.from_numpy(g_da)


def host_interpolate_da_backward(lib, attr, rast, rast_db, tri, g_da):
    Ba, V, C = attr.shape
    B, H, W, _ = rast.shape
    a = [_np(attr), _np(rast), _np(rast_db), _np(tri, np.int32), _np(g_da)]
    g_db, g_attr = np.zeros((B, H, W, 4), np.float32), np.zeros((Ba, V, C), np.float32)
    lib.th_interpolate_da_backward(_ptr(a[0]), Ba, V, C, _ptr(a[1]), _ptr(a[2]), B, H * W, _ptr(a[3]), a[3].shape[0], _ptr(a[4]), _ptr(g_db), _ptr(g_attr))
    return torch.from_numpy(g_db), torch.from_numpy(g_attr)


def host_rasterize_db_backward(lib, pos, tri, rast, g_db):
    B, V, _ = pos.shape
    _, H, W, _ = rast.shape
    a = [_np(pos), _np(tri, np.int32), _np(rast), _np(g_db)]
    g_pos, g_rast = np.zeros((B, V, 4), np.float32), np.zeros((B, H, W, 4), np.float32)
    lib.th_rasterize_db_backward(_ptr(a[0]), B, V, _ptr(a[1]), a[1].shape[0], _ptr(a[2]), H, W, _ptr(a[3]), _ptr(g_pos), _ptr(g_rast))
    return torch.from_numpy(g_pos), torch.from_numpy(g_rast)
