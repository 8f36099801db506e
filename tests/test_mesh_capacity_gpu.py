"""Capacity (host-read-free) form of the mesh optimisation iteration on an MI355X: DMTet(capacity=) -> Mesh(live=).auto_normal ->
MeshRenderer.forward -> mesh_optim_loss + mesh_regularizers(live=) -> backward -> adam_step_n, with the vertex / face buffers sized by
the caller and the live counts in device memory (rules: mvedit_amd/csrc/mesh_capacity_core.h).

References: tests/golden/dmtet_ref.npz (the reference's DMTet class executed, values and autograd gradients), mesh_normals_ref.npz and
mesh_reg_ref.npz (the reference's auto_normal and regularisers executed) at the bars tests/test_dmtet.py and tests/test_mesh_reg.py hold
the exact path to; and the exact path itself, which the capacity form must reproduce bit for bit wherever no float atomic is involved.
Every case fails on a tree without `capacity=` / `live=`."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import dmtet_oracle as DO
from scene import blob_sdf, icosphere, tet_grid

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(__file__)
GD = np.load(os.path.join(HERE, 'golden', 'dmtet_ref.npz'))
GN = np.load(os.path.join(HERE, 'golden', 'mesh_normals_ref.npz'))
GR = np.load(os.path.join(HERE, 'golden', 'mesh_reg_ref.npz'))
S, NV = 32, 2


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-12))


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def grown(n, factor):
    return max(int(np.ceil(n * factor)), n + 1)


def pad_rows(t, rows, value=0):
    out = torch.full((rows,) + tuple(t.shape[1:]), value, dtype=t.dtype, device=t.device)
    out[:t.shape[0]] = t
    return out


def live_of(nv, nf):
    return torch.tensor([nv, nf], dtype=torch.int32).cuda()


@functools.lru_cache(maxsize=None)
def grid(n, seed):
    pos, tets = tet_grid(n)
    return cu(pos), cu(blob_sdf(pos, seed)), cu(tets)


@functools.lru_cache(maxsize=None)
def cameras():
    gold = np.load(os.path.join(HERE, 'golden', 'reference_py.npz'))
    poses = cu(gold['poses'][:NV, :3].astype(np.float32))
    fl = S / (2 * np.tan(np.deg2rad(15)))
    intr = torch.tensor([[fl, fl, S / 2, S / 2]], dtype=torch.float32).repeat(NV, 1).cuda()
    return poses, intr, fl


def check_tail(v, f, e, nv, nf):
    assert (v[nv:] == 0).all() and (f[nf:] == 0).all() and (e is None or (e[nv:] == 0).all())


# ================================================================================================ 1. extraction
@pytest.mark.parametrize('factor', [1.0, 1.5])
@pytest.mark.parametrize('n,seed', [(10, 0), (16, 1)])
def test_extraction_matches_the_reference_output_on_the_live_rows(lib, n, seed, factor):
    from mvedit_amd.mesh_ops import DMTet
    pos, sdf, tets = grid(n, seed)
    gv, gf = GD[f'verts_{n}'], GD[f'faces_{n}']
    nv, nf = gv.shape[0], gf.shape[0]
    cap = (nv, nf) if factor == 1.0 else (grown(nv, factor), grown(nf, factor))
    dm = DMTet('cuda')
    v, f = dm(pos, sdf, tets, capacity=cap)
    assert v.shape == (cap[0], 3) and f.shape == (cap[1], 3) and f.dtype == torch.int64 and v.dtype == torch.float32
    assert dm.counts.tolist() == [nv, nf] and dm.live.tolist() == [nv, nf] and dm.overflow.tolist() == [0]
    assert all(t.is_cuda and t.dtype == torch.int32 for t in (dm.counts, dm.live, dm.overflow))
    assert (v[:nv].cpu().numpy() == gv).all() and (f[:nf].cpu().numpy() == gf).all()          # the golden is the reference class executed
    ve, fe, ee, _ = dm._extract_n(pos, sdf, dm._tets32, *cap)
    vx, fx, ex = dm._extract(pos, sdf, dm._tets32, want_edges=True)                            # the exact path's edges
    assert torch.equal(ve[:nv], vx) and torch.equal(fe[:nf], fx) and torch.equal(ee[:nv], ex)
    check_tail(ve, fe, ee, nv, nf)
    check_tail(v, f, None, nv, nf)
    first = dm.live
    dm(pos, sdf, tets, capacity=cap)
    assert dm.live is not first and dm.live.data_ptr() != first.data_ptr()                     # fresh device tensors on every call


def test_extraction_single_tetrahedron_patterns_and_empty_meshes(lib):
    from mvedit_amd.mesh_ops import DMTet
    dm = DMTet('cuda')
    p4 = torch.tensor([[0., 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]).cuda()
    t4 = torch.tensor([[0, 1, 2, 3]]).cuda()
    for code in range(16):
        s = torch.tensor([1.0 if (code >> k) & 1 else -1.0 for k in range(4)]) * torch.tensor([0.3, 0.5, 0.7, 0.9])
        vo, fo = DO.dmtet(p4.cpu().numpy(), s.numpy(), t4.cpu().numpy())
        v, f = dm(p4, s.cuda(), t4, capacity=(6, 3))
        nv, nf = vo.shape[0], fo.shape[0]
        assert dm.counts.tolist() == [nv, nf] and dm.live.tolist() == [nv, nf] and dm.overflow.item() == 0, code
        assert (v[:nv].cpu().numpy() == vo).all() and (f[:nf].cpu().numpy() == fo).all(), code
        check_tail(v, f, None, nv, nf)
    pos, _, tets = grid(10, 0)
    for fill in (1.0, -1.0):                                           # nothing crosses: live is (0, 0), every row is padding
        v, f = dm(pos, torch.full((pos.shape[0],), fill).cuda(), tets, capacity=(7, 5))
        assert dm.counts.tolist() == [0, 0] and dm.live.tolist() == [0, 0] and dm.overflow.item() == 0
        check_tail(v, f, None, 0, 0)


# ================================================================================================ 2. DMTet backward
@pytest.mark.parametrize('n,seed', [(10, 0), (16, 1)])
def test_backward_matches_reference_autograd_with_half_the_rows_padding(lib, n, seed):
    from mvedit_amd.mesh_ops import DMTet
    pos, sdf, tets = grid(n, seed)
    tp, ts = pos.clone().requires_grad_(True), sdf.clone().requires_grad_(True)
    nv, nf = GD[f'verts_{n}'].shape[0], GD[f'faces_{n}'].shape[0]
    v, f = DMTet('cuda')(tp, ts, tets, capacity=(2 * nv, 2 * nf))
    assert v.requires_grad and not f.requires_grad and (v[:nv].detach().cpu().numpy() == GD[f'verts_{n}']).all()
    R = np.random.default_rng(7).standard_normal((nv, 3)).astype(np.float32)                   # the golden's cotangent on the live rows,
    R = np.concatenate([R, 1e3 * np.random.default_rng(8).standard_normal((nv, 3)).astype(np.float32)])       # anything on the padded ones
    (v * cu(R)).sum().backward()
    for got, want, name in ((tp.grad, GD[f'grad_pos_{n}'], 'pos'), (ts.grad, GD[f'grad_sdf_{n}'], 'sdf')):
        assert torch.isfinite(got).all(), name                                                  # a padded (0, 0) edge would divide by s_a - s_b = 0
        want_t = torch.from_numpy(want)
        scale = want_t.abs().max().item()
        err = (got.cpu() - want_t).abs().max().item()
        print(f'dmtet backward_n n={n} d{name}: max err {err:.3e} of scale {scale:.3e}')
        assert scale > 0 and err <= 1e-5 * scale, name                                          # float atomics: summation order only
    v2, _ = DMTet('cuda')(pos, sdf, tets, capacity=(2 * nv, 2 * nf))
    assert not v2.requires_grad


# ================================================================================================ 3. normals and regularisers
def _padded(verts, faces, factor=1.3, vert_fill=float('nan')):
    """-> padded verts (the padding NaN: a kernel that reads a padded vertex shows), padded faces (0, 0, 0), live"""
    V, F = verts.shape[0], faces.shape[0]
    return pad_rows(verts, grown(V, factor), vert_fill), pad_rows(faces, grown(F, factor), 0), live_of(V, F)


@pytest.mark.parametrize('i', range(int(GN['n_cases'])))
def test_auto_normal_on_a_padded_mesh_vs_reference_method(lib, i):
    from mvedit_amd.mesh_ops import Mesh
    c = lambda k: GN[f'c{i}_{k}']
    V, F = c('verts').shape[0], c('faces').shape[0]
    vp, fp, live = _padded(cu(c('verts'), torch.float32), cu(c('faces')))
    vp.requires_grad_(True)
    m = Mesh(vp, fp, live=live)
    m.auto_normal()
    vn, fn = m.vn.detach().cpu().numpy(), m.face_normals.detach().cpu().numpy()
    assert rel(vn[:V], c('vn')) < 1e-6 and rel(fn[:F], c('face_normals')) < 1e-6
    assert (vn[V:] == 0).all() and (fn[F:] == 0).all() and m.fn.dtype == torch.int32
    g_vn = pad_rows(cu(c('g_vn'), torch.float32), vp.shape[0], 7.0)                             # cotangents on padded rows must not leak
    g_fn = pad_rows(cu(c('g_fn'), torch.float32), fp.shape[0], -5.0)
    g_v, = torch.autograd.grad((m.vn * g_vn).sum() + (m.face_normals * g_fn).sum(), vp)
    assert rel(g_v[:V].cpu().numpy(), c('g_verts')) < 3e-6
    assert (g_v[V:] == 0).all()                                                                # padded rows receive zero gradient


@pytest.mark.parametrize('i', range(int(GR['n_cases'])))
def test_regularisers_on_a_padded_mesh_are_the_exact_call_bit_for_bit(lib, i):
    from mvedit_amd.mesh_ops import mesh_regularizers
    c = lambda k: GR[f'c{i}_{k}']
    v, f, fn = cu(c('verts'), torch.float32), cu(c('faces')), cu(c('face_normals'), torch.float32)
    V, F = v.shape[0], f.shape[0]
    lap_x, nc_x = mesh_regularizers(v, f, fn)
    vp, fp, live = _padded(v, f)
    fnp = pad_rows(fn, fp.shape[0], float('nan'))
    vp.requires_grad_(True), fnp.requires_grad_(True)
    lap, nc = mesh_regularizers(vp, fp, fnp, live=live)
    assert torch.equal(lap.detach(), lap_x) and torch.equal(nc.detach(), nc_x), (lap.item(), lap_x.item(), nc.item(), nc_x.item())
    lap_f, nc_f = float(lap.detach()), float(nc.detach())
    assert abs(lap_f - float(c('lap'))) < 2e-6 * float(c('lap')) and abs(nc_f - float(c('nc'))) < 2e-6 * float(c('nc'))
    g_v, g_fn = torch.autograd.grad(0.25 * lap - 3.0 * nc, (vp, fnp))
    assert rel(g_v[:V].cpu().numpy(), 0.25 * c('g_verts')) < 3e-6 and rel(g_fn[:F].cpu().numpy(), -3.0 * c('g_fn')) < 2e-6
    assert (g_v[V:] == 0).all() and (g_fn[F:] == 0).all()


def test_zero_live_rows_give_zeros_not_nan(lib):
    from mvedit_amd.mesh_ops import Mesh, edge_opposites, mesh_regularizers
    v = torch.zeros(9, 3, device='cuda', requires_grad=True)
    f = torch.zeros(5, 3, dtype=torch.int64, device='cuda')
    live = live_of(0, 0)
    m = Mesh(v, f, live=live)
    m.auto_normal()
    assert (m.vn == 0).all() and (m.face_normals == 0).all()
    lap, nc = mesh_regularizers(v, f, m.face_normals, live=live)
    assert float(lap) == 0.0 and float(nc) == 0.0
    g, = torch.autograd.grad(lap + nc + m.vn.sum() + m.face_normals.sum(), v)
    assert (g == 0).all()
    assert (edge_opposites(f, live) == -1).all()
    # live vertices without a live face (a count pair no extraction produces, but the kernels must hold): still zeros
    lap, nc = mesh_regularizers(v, f, m.face_normals, live=live_of(4, 0))
    assert float(lap) == 0.0 and float(nc) == 0.0


# ================================================================================================ 4. opposites
@pytest.mark.parametrize('which', ['dmtet_10', 'dmtet_16', 'reg_0', 'reg_1'])
def test_opposites_take_live_faces_only(lib, which):
    from mvedit_amd.mesh_ops import edge_opposites
    kind, k = which.split('_')
    f = cu(GD[f'faces_{k}'] if kind == 'dmtet' else GR[f'c{k}_faces'])
    F = f.shape[0]
    want = edge_opposites(f)
    fp = pad_rows(f, grown(F, 1.3), 0)
    got = edge_opposites(fp, live_of(int(f.max()) + 1, F))
    assert got.dtype == torch.int32 and torch.equal(got[:F], want) and (got[F:] == -1).all()
    assert int((want >= 0).sum()) > F                                                          # the comparison is not about an empty table


# ================================================================================================ 5. render
def _vc(v):
    return torch.cat([torch.full_like(v, 0.7), torch.ones_like(v[:, :1])], -1)


def test_render_of_the_padded_mesh_is_the_exact_render_bit_for_bit(lib):
    from mvedit_amd.mesh_ops import Mesh, MeshRenderer
    poses, intr, _ = cameras()
    v, f = cu(GD['verts_10']), cu(GD['faces_10'])
    V, F = v.shape[0], f.shape[0]
    mx = Mesh(v, f, vc=_vc(v))
    mx.auto_normal()
    vp, fp, live = _padded(v, f, vert_fill=0.0)
    # one set of vertex normals for both meshes (auto_normal sums with float atomics; it has its own test above): this case is the renderer's
    mp = Mesh(vp, fp, vn=pad_rows(mx.vn, vp.shape[0], 0.0), fn=fp.to(torch.int32), vc=_vc(vp), live=live)
    mr = MeshRenderer(near=0.01, far=100)
    with torch.no_grad():
        ox = mr([mx], poses[None], intr[None], S, S)
        op = mr([mp], poses[None], intr[None], S, S)
        gx = mr.render_geometry(v, f.to(torch.int32), mx.vn, mx.fn, poses, intr, S, S)
        gp = mr.render_geometry(vp, fp.to(torch.int32), mp.vn, mp.fn, poses, intr, S, S, host_read_free=True)
    assert torch.equal(gx['rast'], gp['rast'])
    cover = float((gx['rast'][..., 3] > 0).float().mean())
    assert 0.05 < cover < 0.95, cover
    for k in ('rgba', 'normal', 'depth'):
        assert ox[k].shape == op[k].shape and torch.equal(ox[k], op[k]), k


# ================================================================================================ 6. whole iteration
@functools.lru_cache(maxsize=None)
def targets():
    """what the loop fits: the render of a slightly larger sphere (exact path, once)"""
    from mvedit_amd.mesh_ops import Mesh, MeshRenderer
    poses, intr, fl = cameras()
    v0, f0 = icosphere(2, 0.7)
    v0, f0 = cu(v0), cu(f0)
    m = Mesh(v0, f0, vc=_vc(v0))
    mr = MeshRenderer(near=0.01, far=100)
    with torch.no_grad():
        m.auto_normal()
        out = mr([m], poses[None], intr[None], S, S)
    rgba, normal = out['rgba'][0], out['normal'][0]
    tgt_m = rgba[..., 3:].contiguous()
    tgt_rgb = (rgba[..., :3] / tgt_m.clamp(min=1e-3)).contiguous()
    erode = -torch.nn.functional.max_pool2d(-tgt_m.permute(0, 3, 1, 2), 5, stride=1, padding=2).permute(0, 2, 3, 1).contiguous()
    ys, xs = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing='ij')
    dirs = torch.stack([(xs + 0.5 - S / 2) / fl, (ys + 0.5 - S / 2) / fl, torch.ones_like(xs)], -1)[None].repeat(NV, 1, 1, 1).cuda()
    return dict(rgb=tgt_rgb, erode=erode, m=tgt_m, dirs=dirs.contiguous(), normal=normal.contiguous(), view_w=torch.ones(NV, device='cuda'), mr=mr)


def iteration(dm, sdf, deform, state, capacity, lr=1e-3):
    """one mesh_optim iteration (mvedit_3d_pipeline.py:745-847 with the DMTet call of :828); capacity=None is the exact form"""
    from mvedit_amd.mesh_ops import Mesh, adam_step_n, mesh_regularizers
    from mvedit_amd.recon_loss import mesh_optim_loss
    pos, _, tets = grid(10, 0)
    poses, intr, _ = cameras()
    t = targets()
    sdf.grad = deform.grad = None
    if capacity is None:
        v, f = dm(pos + deform, sdf, tets)
        live, skip = None, None
    else:
        v, f = dm(pos + deform, sdf, tets, capacity=capacity)
        live, skip = dm.live, dm.overflow
    m = Mesh(v, f, vc=_vc(v), live=live)
    m.auto_normal()
    out = t['mr']([m], poses[None], intr[None], S, S)
    res = mesh_optim_loss(out['rgba'][0], out['normal'][0], out['depth'][0].detach(), t['rgb'], t['erode'], t['m'], t['dirs'], t['view_w'],
                          target_n=t['normal'], normal_reg_weight=1.0)
    lap, nc = mesh_regularizers(v, f, m.face_normals, live=live)
    (res['loss'] + 5.0 * (lap + nc)).backward()
    adam_step_n([sdf, deform], [sdf.grad, deform.grad], state, lr=lr, skip_if=skip)
    return res['loss'].detach(), lap.detach(), nc.detach(), out


def _start():
    pos, sdf, _ = grid(10, 0)
    return sdf.clone().requires_grad_(True), torch.zeros_like(pos).requires_grad_(True), {}


def test_adam_step_n_is_torch_adam(lib):
    from mvedit_amd.mesh_ops import adam_step_n
    g = torch.Generator().manual_seed(5)
    ps = [torch.randn(37, generator=g).cuda(), torch.randn(11, 3, generator=g).cuda()]
    qs = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.Adam(qs, lr=1e-3)
    state = {}
    for _ in range(3):
        grads = [torch.randn(p.shape, generator=g).cuda() for p in ps]
        for q, gr in zip(qs, grads):
            q.grad = gr.clone()
        opt.step()
        adam_step_n(ps, grads, state, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    assert state['step'].tolist() == [3]
    for p, q in zip(ps, qs):
        # three steps, each rounded once into the parameter (an ulp is 1.2e-7 of its value) and of size <= lr with ~1e-6 of relative error
        assert (p - q.detach()).abs().max().item() <= 3 * 1.2e-7 * q.detach().abs().max().item() + 3 * 1e-3 * 2e-6


def test_whole_iteration_capacity_form_vs_exact_form(lib):
    from mvedit_amd.mesh_ops import DMTet
    nv, nf = GD['verts_10'].shape[0], GD['faces_10'].shape[0]
    cap = (grown(nv, 1.5), grown(nf, 1.5))
    sx, dx, stx = _start()
    sc, dc, stc = _start()
    lx = iteration(DMTet('cuda'), sx, dx, stx, None)
    lc = iteration(DMTet('cuda'), sc, dc, stc, cap)
    for name, a, b in zip(('loss', 'laplacian', 'normal consistency'), lx[:3], lc[:3]):
        print(f'iteration 1 {name}: exact {float(a)!r} capacity {float(b)!r}')
    for name, a, b in (('sdf', sx, sc), ('deform', dx, dc)):
        scale = a.detach().abs().max().item()
        err = (a.detach() - b.detach()).abs().max().item()
        print(f'after the step, {name}: max |exact - capacity| = {err:.3e}, scale {scale:.3e}')
    for name, a, b in zip(('loss', 'laplacian', 'normal consistency'), lx[:3], lc[:3]):
        assert torch.isfinite(a) and torch.equal(a, b), (name, float(a), float(b))
    assert stx['step'].tolist() == [1] and stc['step'].tolist() == [1]
    moved = 0.0
    for name, a, b, a0 in (('sdf', sx, sc, grid(10, 0)[1]), ('deform', dx, dc, torch.zeros_like(dx))):
        scale = a.detach().abs().max().item()
        assert (a.detach() - b.detach()).abs().max().item() <= 1e-5 * scale, name             # gradients pass through float atomics
        moved += (a.detach() - a0).abs().max().item()
    assert moved > 1e-4                                                                        # the step was a step


def test_capacity_iterations_never_read_on_the_host(lib):
    from mvedit_amd.mesh_ops import DMTet
    nv, nf = GD['verts_10'].shape[0], GD['faces_10'].shape[0]
    cap = (grown(nv, 1.5), grown(nf, 1.5))
    sdf, deform, state = _start()
    dm = DMTet('cuda')
    targets()
    iteration(dm, sdf, deform, state, cap)                               # warm-up outside the guard: allocator, lazy module loads
    torch.cuda.synchronize()
    flags = []
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for _ in range(4):
            iteration(dm, sdf, deform, state, cap)
            flags.append(dm.overflow)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert state['step'].tolist() == [5] and [int(f) for f in flags] == [0, 0, 0, 0]
    assert torch.isfinite(sdf).all() and torch.isfinite(deform).all() and dm.counts.tolist() == dm.live.tolist()


# ================================================================================================ 7. overflow
@pytest.mark.parametrize('short', ['verts', 'faces'])
def test_overflow_is_the_empty_mesh_and_skips_the_step(lib, short):
    from mvedit_amd.mesh_ops import DMTet, Mesh, MeshRenderer, adam_step_n
    pos, sdf0, tets = grid(10, 0)
    poses, intr, _ = cameras()
    nv, nf = GD['verts_10'].shape[0], GD['faces_10'].shape[0]
    cap = (nv - 1, nf) if short == 'verts' else (nv, nf - 1)
    dm = DMTet('cuda')
    v, f = dm(pos, sdf0, tets, capacity=cap)
    assert dm.overflow.tolist() == [1] and dm.counts.tolist() == [nv, nf] and dm.live.tolist() == [0, 0]
    check_tail(v, f, None, 0, 0)                                         # never a truncated mesh with dangling indices
    m = Mesh(v, f, vc=_vc(v), live=dm.live)
    m.auto_normal()
    with torch.no_grad():
        out = MeshRenderer(near=0.01, far=100)([m], poses[None], intr[None], S, S)
    assert (out['rgba'][..., 3] == 0).all() and (out['rgba'] == 0).all() and (out['depth'] == 0).all()
    # an optimiser with history (one real step), then a step under the raised flag: nothing moves
    g = torch.Generator().manual_seed(3)
    params = [sdf0.clone(), torch.zeros_like(pos)]
    state = {}
    adam_step_n(params, [torch.randn(p.shape, generator=g).cuda() for p in params], state, lr=1e-3)
    keep = [p.clone() for p in params] + [t.clone() for mm in state['moments'] for t in mm] + [state['step'].clone()]
    adam_step_n(params, [torch.randn(p.shape, generator=g).cuda() for p in params], state, lr=1e-3, skip_if=dm.overflow)
    now = params + [t for mm in state['moments'] for t in mm] + [state['step']]
    assert state['step'].tolist() == [1] and all(torch.equal(a, b) for a, b in zip(keep, now))
    # grow from the true totals, at a point where the loop synchronises anyway
    v, f = dm(pos, sdf0, tets, capacity=tuple(dm.counts.tolist()))
    assert dm.overflow.tolist() == [0] and dm.live.tolist() == [nv, nf]
    assert (v.cpu().numpy() == GD['verts_10']).all() and (f.cpu().numpy() == GD['faces_10']).all()
