"""Times the texture path's geometry gradient behind mvedit_amd.nvdiffrast.torch (csrc/texture_grad.hip) at a size the mesh optimisation runs:
32 views at 512 x 512 of the subdivision-6 icosphere (40 962 vertices, 81 920 faces), one chart per face in a 1024 x 1024 RGB atlas,
filter_mode='linear-mipmap-linear'.

  * the chain pos, vt, tex -> rasterize -> interpolate(rast_db, 'all') -> texture -> <., g_out>: forward, and forward + backward through the
    facade with every gradient (pos, vt, tex)
  * the same with uv / uv_da detached through mesh_ops (what the engine could do before: no gradient from the fetch back to the geometry)
  * each of the three new kernels alone, with the bytes it must move (streams per pixel, the vertex arrays read and added to once, the
    texture and its level stack once) over its time

Device-event times, mean of K launches after warm-up; repeated R times to show the spread.  python tools/nvdr_grad_bench.py [K] [R]"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from scene import face_atlas, icosphere  # noqa: E402
from mvedit_amd import _lib, mesh_ops  # noqa: E402
import mvedit_amd.nvdiffrast.torch as dr  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
R = int(sys.argv[2]) if len(sys.argv) > 2 else 3
B, S, T, C, SUBDIV = 32, 512, 1024, 3, 6
dev = torch.device('cuda:0')
torch.cuda.set_device(dev)
g = torch.Generator().manual_seed(3)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(R):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(K):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / K)
    return out


def fmt(ts):
    return f'{min(ts):8.3f} ms  (runs: {", ".join(f"{t:.3f}" for t in ts)})'


v, f = icosphere(SUBDIV, 0.6)
vt_np, ft_np = face_atlas(f)
p = torch.from_numpy(v)
views = []
for i in range(B):
    ang, tilt = 2 * math.pi * i / B, 0.4 * math.sin(3.0 * i)
    ca, sa, ct, st = math.cos(ang), math.sin(ang), math.cos(tilt), math.sin(tilt)
    rot = torch.tensor([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ torch.tensor([[1, 0, 0], [0, ct, -st], [0, st, ct]])
    q = p @ rot.T.float()
    z = q[:, 2] + 2.5
    views.append(torch.stack([q[:, 0] * 2.0, q[:, 1] * 2.0, (z - 2.5) * 0.5, z], dim=-1))
pos0 = torch.stack(views).to(dev)
tri, ft = torch.from_numpy(f.astype(np.int32)).to(dev), torch.from_numpy(ft_np.astype(np.int32)).to(dev)
vt0 = torch.from_numpy(vt_np)[None].to(dev)
tex0 = torch.rand(1, T, T, C, generator=g).to(dev)
g_out = torch.randn(B, S, S, C, generator=g).to(dev)
ctx = dr.RasterizeCudaContext()
V, F, Vt = pos0.shape[1], tri.shape[0], vt0.shape[1]


def facade(grad):
    pos, vt, tex = (x.detach().requires_grad_(grad) for x in (pos0, vt0, tex0))
    rast, db = dr.rasterize(ctx, pos, tri, (S, S))
    uv, da = dr.interpolate(vt, rast, ft, rast_db=db, diff_attrs='all')
    out = dr.texture(tex, uv, uv_da=da)
    if grad:
        (out * g_out).sum().backward()
    return out


def detached_uv():
    # nothing reaches pos or vt from the fetch: the backward is the texture's alone
    tex = tex0.detach().requires_grad_(True)
    rast = mesh_ops.rasterize(pos0, tri, (S, S))
    uv = mesh_ops.interpolate(vt0, rast, ft)
    da = mesh_ops.interpolate_da(vt0, rast, mesh_ops.rasterize_db(pos0, tri, rast), ft)
    out = mesh_ops.texture(tex, uv, uv_da=da, filter_mode='linear-mipmap-linear')
    (out * g_out).sum().backward()
    return out


with torch.no_grad():
    rast, db = dr.rasterize(ctx, pos0, tri, (S, S))
    uv, da = dr.interpolate(vt0, rast, ft, rast_db=db, diff_attrs='all')
    mips, lv = mesh_ops.build_mips(tex0)
cover = (rast[..., 3] > 0).float().mean().item()
npix = B * S * S
print(f'{B} views {S} x {S}, {V} vertices, {F} faces, atlas {T} x {T} x {C} ({lv} levels above 0), coverage {cover:.3f}; K = {K}, R = {R}', flush=True)
print('chain rasterize -> interpolate(rast_db, all) -> texture (linear-mipmap-linear):', flush=True)
print(f'  forward (facade, no grad)                          {fmt(timed(lambda: facade(False)))}', flush=True)
print(f'  forward + backward, facade: pos, vt, tex           {fmt(timed(lambda: facade(True)))}', flush=True)
print(f'  forward + backward, mesh_ops, uv detached: tex     {fmt(timed(detached_uv))}', flush=True)

sp = _lib.stream_ptr(dev)
g_uv, g_da, g_db, via = torch.empty_like(uv), torch.randn(da.shape, generator=g).to(dev), torch.randn(db.shape, generator=g).to(dev), torch.empty_like(rast)
g_da_out, g_db_out = torch.empty_like(da), torch.empty_like(db)
g_vt, g_pos = torch.zeros_like(vt0), torch.zeros_like(pos0)
kernels = [
    ('mve_texture_grad_uv', lambda: _lib.call('mve_texture_grad_uv', _lib.ptr(tex0), _lib.ptr(mips), 1, T, T, C, lv, _lib.ptr(uv), _lib.ptr(da), _lib.ptr(g_out),
                                              B, S, S, _lib.ptr(g_uv), _lib.ptr(g_da_out), sp),
     npix * (8 + 16 + 4 * C + 8 + 16) + 4 * C * (T * T + int(mips.numel() // C))),
    ('mve_interpolate_da_backward', lambda: _lib.call('mve_interpolate_da_backward', _lib.ptr(vt0), 1, Vt, 2, _lib.ptr(rast), _lib.ptr(db), B, S * S, _lib.ptr(ft), F,
                                                      _lib.ptr(g_da), _lib.ptr(g_db_out), _lib.ptr(g_vt), sp),
     npix * (16 + 16 + 16 + 16) + 4 * (3 * F + 3 * Vt * 2)),
    ('mve_rasterize_db_backward', lambda: _lib.call('mve_rasterize_db_backward', _lib.ptr(pos0), B, V, _lib.ptr(tri), F, _lib.ptr(rast), S, S, _lib.ptr(g_db),
                                                    _lib.ptr(g_pos), _lib.ptr(via), sp),
     npix * (16 + 16 + 16) + 4 * (3 * F + 3 * B * V * 4)),
]
print('the new kernels alone (bytes that must move / time):', flush=True)
for name, fn, nbytes in kernels:
    ts = timed(fn)
    print(f'  {name:30s} {fmt(ts)}   {nbytes / 1e6:8.1f} MB -> {nbytes / min(ts) / 1e6:7.1f} GB/s', flush=True)
