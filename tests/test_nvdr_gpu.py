"""`mvedit_amd.nvdiffrast.torch` on the GPU: forwards against `mesh_ops` (same kernels, bit for bit), gradients against float64 torch autograd
over the oracle chain (tests/nvdr_chain.py) -- per op on identical float32 inputs and end to end pos, vt, tex -> rasterize -> interpolate ->
texture -- the reference's own forward composed from `dr.*` calls against its recorded output, `visibility_grad`, a fit that only the new
uv path can do, and the first-order-only / grad_db / pos_gradient_boost contracts.

Bars.  Per-pixel gradients (uv, uv_da, rast, rast_db): e_kernel <= 4 e_f32 + 1e-6 scale (max-abs; float64 is the truth, e_f32 the distance of
the float32 TORCH evaluation of the same formulas from it -- the convention of test_mesh_ops.py::test_mip_texture_kernels_vs_oracle).
Atomically summed gradients (attr, pos, tex): rel-L2 <= 1e-3, the project's per-kernel bar (README "Parity").  Pixels at which the derivative
jumps are excused as nvdr_chain.excused defines, at most 2 % of them."""
import os

import numpy as np
import pytest
import torch

import nvdr_chain as NC
from oracle import texture_mip_oracle as TM

pytestmark = pytest.mark.gpu
FILTERS = ['linear', 'linear-mipmap-linear']


def _dr():
    import mvedit_amd.nvdiffrast.torch as dr
    return dr


def _per_pixel_bar(name, got, want64, f32):
    scale = want64.abs().max().item()
    e_ker, e_f32 = (got.cpu().double() - want64).abs().max().item(), (f32.double() - want64).abs().max().item()
    print(f'{name}: e_kernel {e_ker:.3e}  e_f32 {e_f32:.3e}  scale {scale:.3e}')
    assert scale > 0 and np.isfinite(e_ker) and e_ker <= 4 * e_f32 + 1e-6 * scale, (name, e_ker, e_f32, scale)


def _summed_bar(name, got, want64, f32):
    r_ker, r_f32 = NC.rel_l2(got.cpu(), want64), NC.rel_l2(f32, want64)
    print(f'{name}: rel-L2 kernel {r_ker:.3e}  float32 torch {r_f32:.3e}')
    assert np.isfinite(r_ker) and r_ker <= 1e-3, (name, r_ker, r_f32)


def _facade_forward(sc, filt, grad=False):
    """The chain of test 8 through the facade on the GPU -> dict of GPU tensors (leaves pos, vt, tex require grad when `grad`)."""
    dr = _dr()
    pos, vt, tex = (sc[k].cuda().requires_grad_(grad) for k in ('pos', 'vt', 'tex'))
    tri, ft = sc['tri'].cuda(), sc['ft'].cuda()
    rast, db = dr.rasterize(dr.RasterizeCudaContext(), pos, tri, (sc['S'], sc['S']))
    uv, da = dr.interpolate(vt, rast, ft, rast_db=db, diff_attrs='all')
    out = dr.texture(tex, uv, uv_da=da, filter_mode=filt)
    return dict(pos=pos, vt=vt, tex=tex, rast=rast, rast_db=db, uv=uv, uv_da=da, out=out)


def _excusal(uv64, da64, rast, atlas, mip):
    """-> (excused [B,H,W] bool, share of the covered pixels)"""
    ex = NC.excused(uv64, da64, atlas, atlas, NC.mip_levels(atlas, atlas), mip)
    fg = rast[..., 3] > 0
    share = (ex & fg).float().sum().item() / fg.float().sum().item()
    print(f'excused {share:.4f} of {int(fg.sum())} covered pixels')
    assert share <= 0.02, share
    return ex


# ------------------------------------------------------------------------------------------------ 6. forward
def test_forward_equals_mesh_ops_bit_for_bit(lib):
    from mvedit_amd import mesh_ops
    from mvedit_amd.mesh_ops import MeshRenderer
    from test_mesh_ops import _mip_scene
    dr = _dr()
    S, T = 64, 256
    v, f, vn, vt, ft, tex, poses, intr = _mip_scene(S, T)
    t = lambda a: torch.from_numpy(a).cuda()
    _, v_clip, _ = MeshRenderer(near=0.01, far=100).project(t(v), t(poses), t(intr), S, S)
    tri, ftc, vtc, tx = t(f), t(ft), t(vt)[None], t(tex[..., :3].copy())[None]
    rast, db = dr.rasterize(dr.RasterizeCudaContext(), v_clip, tri, (S, S))
    rast_m = mesh_ops.rasterize(v_clip, tri, (S, S))
    assert torch.equal(rast, rast_m) and torch.equal(db, mesh_ops.rasterize_db(v_clip, tri, rast_m))
    r2, db2 = dr.rasterize(dr.RasterizeGLContext(output_db=False), v_clip, tri.long(), [S, S])
    assert torch.equal(r2, rast) and tuple(db2.shape) == (3, S, S, 0)
    assert torch.equal(dr.rasterize(dr.RasterizeGLContext(), v_clip, tri, (S, S))[1], db)
    fg = rast[..., 3] > 0
    assert 0.05 < fg.float().mean().item() < 0.8
    uv, da = dr.interpolate(vtc, rast, ftc, rast_db=db, diff_attrs='all')
    assert torch.equal(uv, mesh_ops.interpolate(vtc, rast, ftc)) and torch.equal(da, mesh_ops.interpolate_da(vtc, rast, db, ftc))
    uv1, da1 = dr.interpolate(vtc, rast, ftc, rast_db=db, diff_attrs=[1])
    assert torch.equal(uv1, uv) and torch.equal(da1, da[..., 2:4])
    for extra in (dict(), dict(rast_db=db)):                               # no rast_db or no diff_attrs: an empty second output
        o, d = dr.interpolate(vtc, rast, ftc, **extra)
        assert torch.equal(o, uv) and tuple(d.shape) == (3, S, S, 0)
    zero_uv, zero_da = torch.zeros(1, 1, 1, 2, dtype=torch.float64), torch.zeros(1, 1, 1, 4, dtype=torch.float64)
    for filt in FILTERS:
        out = dr.texture(tx, uv, uv_da=da, filter_mode=filt)
        ref = mesh_ops.texture(tx, uv, rast, uv_da=da, filter_mode=filt)
        assert torch.equal(out[fg], ref[fg]) and (ref[~fg] == 0).all()
        # empty pixels fetch at their uv = (0, 0) with an empty footprint, as nvdiffrast does: the mean of the four corner texels
        at0 = TM.texture(tx.cpu().double(), zero_uv, zero_da, filter_mode=filt)[0, 0, 0]
        assert (out[~fg].cpu().double() - at0).abs().max().item() < 1e-6
    assert torch.equal(dr.texture(tx, uv, uv_da=da), dr.texture(tx, uv, uv_da=da, filter_mode='linear-mipmap-linear'))      # 'auto'
    assert torch.equal(dr.texture(tx, uv), dr.texture(tx, uv, filter_mode='linear'))
    color = torch.rand(3, S, S, 5, generator=torch.Generator().manual_seed(4)).cuda()
    aa = dr.antialias(color, rast, v_clip, tri)
    assert torch.equal(aa, mesh_ops.antialias(color, rast, v_clip, tri)) and not torch.equal(aa, color)
    assert torch.equal(aa, dr.antialias(color, rast, v_clip, tri, topology_hash=dr.antialias_construct_topology_hash(tri)))


# ------------------------------------------------------------------------------------------------ 7. per-op gradients
@pytest.mark.parametrize('filt', FILTERS)
def test_texture_gradients_vs_float64_oracle(lib, filt):
    dr = _dr()
    S, atlas = 64, 256
    sc = NC.sphere_scene(S, atlas)
    mip = filt == 'linear-mipmap-linear'
    fw = _facade_forward(sc, filt)
    uv32, da32, tex32 = fw['uv'].detach().cpu(), fw['uv_da'].detach().cpu(), sc['tex']
    ex = _excusal(uv32.double(), da32.double(), fw['rast'].cpu(), atlas, mip)
    g = sc['g_out'] * (~ex)[..., None]
    uv, da, tex = (x.cuda().requires_grad_(True) for x in (uv32, da32, tex32))
    (dr.texture(tex, uv, uv_da=da if mip else None, filter_mode=filt) * g.cuda()).sum().backward()

    def oracle(dtype):
        u, d, t = (x.detach().to(dtype).clone().requires_grad_(True) for x in (uv32, da32, tex32))
        (TM.texture(t, u, d if mip else None, filter_mode=filt) * g.to(dtype)).sum().backward()
        return u.grad, d.grad, t.grad
    w_uv, w_da, w_tex = oracle(torch.float64)
    f_uv, f_da, f_tex = oracle(torch.float32)
    _per_pixel_bar('texture -> uv', uv.grad, w_uv, f_uv)
    if mip:
        # an empty footprint (uv_da = 0 on the empty pixels): level = -inf, clamped to 0 -- the derivative is zero by the clamping rule and the
        # kernel writes zero; torch autograd over the oracle multiplies 0 by inf there and returns NaN, so those pixels are compared with the rule
        empty = (da32 == 0).all(-1)
        assert empty.any() and torch.isfinite(da.grad).all() and (da.grad.cpu()[empty] == 0).all() and torch.isnan(w_da[empty]).all()
        _per_pixel_bar('texture -> uv_da', da.grad.cpu()[~empty], w_da[~empty], f_da[~empty])
    else:
        assert da.grad is None
    _summed_bar('texture -> tex', tex.grad, w_tex, f_tex)


def test_interpolate_gradients_vs_float64_oracle(lib):
    dr = _dr()
    sc = NC.sphere_scene(64, 256)
    fw = _facade_forward(sc, 'linear')
    gen = torch.Generator().manual_seed(11)
    rast32, db32 = fw['rast'].detach().cpu(), fw['rast_db'].detach().cpu()
    attr32 = torch.cat([sc['vt'], torch.randn(1, sc['vt'].shape[1], 1, generator=gen)], dim=-1)
    g_out, g_da = torch.randn(*rast32.shape[:3], 3, generator=gen), torch.randn(*rast32.shape[:3], 6, generator=gen)
    attr, rast, db = (x.cuda().requires_grad_(True) for x in (attr32, rast32, db32))
    out, da = dr.interpolate(attr, rast, sc['ft'].cuda(), rast_db=db, diff_attrs='all')
    ((out * g_out.cuda()).sum() + (da * g_da.cuda()).sum()).backward()

    def oracle(dtype):
        a, r, d = (x.detach().to(dtype).clone().requires_grad_(True) for x in (attr32, rast32, db32))
        o = NC.interpolate(a, r, sc['ft'])
        o_da = TM.interpolate_da(a, r, d, sc['ft'])
        ((o * g_out.to(dtype)).sum() + (o_da * g_da.to(dtype)).sum()).backward()
        return a.grad, r.grad, d.grad
    w_a, w_r, w_d = oracle(torch.float64)
    f_a, f_r, f_d = oracle(torch.float32)
    _per_pixel_bar('interpolate -> rast', rast.grad, w_r, f_r)
    _per_pixel_bar('interpolate -> rast_db', db.grad, w_d, f_d)
    _summed_bar('interpolate -> attr', attr.grad, w_a, f_a)
    # a subset of the attributes: the gradient of the others' differentials is absent, not garbage
    attr2, db2 = attr32.cuda().requires_grad_(True), db32.cuda().requires_grad_(True)
    _, da_sub = dr.interpolate(attr2, rast32.cuda(), sc['ft'].cuda(), rast_db=db2, diff_attrs=[2, 0])
    (da_sub * g_da[..., :4].cuda()).sum().backward()
    a, d = attr32.double().requires_grad_(True), db32.double().requires_grad_(True)
    full = TM.interpolate_da(a, rast32.double(), d, sc['ft']).reshape(*rast32.shape[:3], 3, 2)[..., [2, 0], :].reshape(*rast32.shape[:3], 4)
    (full * g_da[..., :4].double()).sum().backward()
    assert NC.rel_l2(db2.grad.cpu(), d.grad) <= 1e-5 and NC.rel_l2(attr2.grad.cpu(), a.grad) <= 1e-3


def test_rasterize_gradient_from_rast_and_rast_db_vs_float64_oracle(lib):
    dr = _dr()
    S = 64
    sc = NC.sphere_scene(S, 256)
    gen = torch.Generator().manual_seed(12)
    g_rast, g_db = torch.randn(2, S, S, 4, generator=gen), torch.randn(2, S, S, 4, generator=gen)
    g_rast[..., 3] = 0
    pos = sc['pos'].cuda().requires_grad_(True)
    rast, db = dr.rasterize(dr.RasterizeCudaContext(), pos, sc['tri'].cuda(), (S, S))
    ((rast * g_rast.cuda()).sum() + (db * g_db.cuda()).sum()).backward()
    stored = rast.detach().cpu()

    def oracle(dtype):
        p = sc['pos'].detach().to(dtype).clone().requires_grad_(True)
        r = NC.rast_with_continuous_gradient(p, sc['tri'], stored)
        d = TM.rasterize_db(p, sc['tri'], r)
        ((r * g_rast.to(dtype)).sum() + (d * g_db.to(dtype)).sum()).backward()
        return p.grad
    _summed_bar('rasterize -> pos (g_rast and g_db)', pos.grad, oracle(torch.float64), oracle(torch.float32))
    # and each alone
    for name, use_db in (('g_rast alone', False), ('g_db alone', True)):
        p = sc['pos'].cuda().requires_grad_(True)
        r, d = dr.rasterize(dr.RasterizeCudaContext(), p, sc['tri'].cuda(), (S, S))
        ((d * g_db.cuda()).sum() if use_db else (r * g_rast.cuda()).sum()).backward()
        p64 = sc['pos'].double().requires_grad_(True)
        r64 = NC.rast_with_continuous_gradient(p64, sc['tri'], stored)
        ((TM.rasterize_db(p64, sc['tri'], r64) * g_db.double()).sum() if use_db else (r64 * g_rast.double()).sum()).backward()
        print(name, 'rel-L2', NC.rel_l2(p.grad.cpu(), p64.grad))
        assert NC.rel_l2(p.grad.cpu(), p64.grad) <= 1e-3


# ------------------------------------------------------------------------------------------------ 8. the whole chain
@pytest.mark.parametrize('S,atlas', [(64, 256), (64, 1024), (128, 64)])
@pytest.mark.parametrize('filt', FILTERS)
def test_whole_chain_gradients_vs_float64_oracle(lib, filt, S, atlas):
    """pos, vt, tex -> rasterize -> interpolate(rast_db, 'all') -> texture -> <., g_out> through the facade against the float64 chain evaluated
    at the rasteriser's stored (u, v)."""
    sc = NC.sphere_scene(S, atlas)
    fw = _facade_forward(sc, filt, grad=True)
    stored = fw['rast'].detach().cpu()
    with torch.no_grad():
        f64 = NC.chain(sc['pos'].double(), sc['tri'], sc['vt'].double(), sc['ft'], sc['tex'].double(), stored, filt)
    assert (fw['out'].detach().cpu().double() - f64['out']).abs().max().item() < 1e-3                # the same forward up to fp32
    ex = _excusal(f64['uv'], f64['uv_da'], stored, atlas, filt == 'linear-mipmap-linear')
    g = sc['g_out'] * (~ex)[..., None]
    (fw['out'] * g.cuda()).sum().backward()
    want, _ = NC.chain_gradients(sc, stored, filt, g, torch.float64)
    f32, _ = NC.chain_gradients(sc, stored, filt, g, torch.float32)
    for k in ('pos', 'vt', 'tex'):
        assert want[k].abs().max().item() > 0
        _summed_bar(f'chain -> {k}', fw[k].grad, want[k], f32[k])


# ------------------------------------------------------------------------------------------------ 9. the reference's forward
@pytest.mark.parametrize('tag,filt', [('tex_aa', 'linear'), ('texmip_aa', None)])
def test_reference_forward_composed_from_dr_calls_vs_golden(lib, tag, filt):
    """The steps of the reference's MeshRenderer.forward for a textured mesh (rasterize; interpolate vt with rast_db; texture; albedo[~fg] = 0;
    alpha; antialias), composed here from `dr.*` calls on the recorded v_clip, against the output of the reference's own forward
    (tests/golden/mesh_forward_ref.npz).  Criterion of test_mesh_ops.py::test_mesh_renderer_forward_mip_mapped_vs_reference_golden."""
    import importlib.util
    dr = _dr()
    here = os.path.dirname(__file__)
    G = np.load(os.path.join(here, 'golden', 'mesh_forward_ref.npz'))
    spec = importlib.util.spec_from_file_location('make_mesh_forward_golden', os.path.join(here, 'golden', 'make_mesh_forward_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    v, f, vn, vt, ft, tex, vcol, poses, intr, S = mod.scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    albedo_map = t(tex if tag == 'tex_aa' else G['tex_big'])
    v_clip, tri = t(G[f'{tag}_v_clip']), t(f)
    glctx = dr.RasterizeCudaContext()
    rast, rast_db = dr.rasterize(glctx, v_clip, tri, (S, S), grad_db=torch.is_grad_enabled())
    fg = rast[..., 3] > 0
    texc, texc_db = dr.interpolate(t(vt).unsqueeze(0).contiguous(), rast, t(ft), rast_db=rast_db, diff_attrs='all')
    kw = dict(filter_mode=filt) if filt is not None else dict()                  # texmip: the default filter ('auto' with uv_da)
    albedo = dr.texture(albedo_map.unsqueeze(0)[..., :3].contiguous(), texc, uv_da=texc_db, **kw)
    albedo[~fg] = 0
    rgba = torch.cat([albedo, fg.float().unsqueeze(-1)], dim=-1)
    rgba = dr.antialias(rgba, rast, v_clip, tri)
    bad = (np.abs(rgba.cpu().numpy() - G[f'{tag}_rgba']).max(-1) > 1e-4)
    print(tag, 'pixels off by more than 1e-4:', bad.mean())
    assert bad.mean() < 2e-3, bad.mean()


# ------------------------------------------------------------------------------------------------ 10. visibility_grad
def test_visibility_grad_as_the_reference_computes_it(lib):
    """base_mesh_renderer.py:470-475: autograd.grad(dr.texture(ones, texc, uv_da=texc_db).sum(), ones)."""
    dr = _dr()
    S, T = 64, 128
    sc = NC.sphere_scene(S, T)
    fw = _facade_forward(sc, 'linear-mipmap-linear')
    texc, texc_db = fw['uv'].detach(), fw['uv_da'].detach()
    with torch.enable_grad():
        dummy = torch.ones(2, T, T, 1, device='cuda').requires_grad_(True)
        albedo = dr.texture(dummy, texc, uv_da=texc_db, filter_mode='linear-mipmap-linear')
        vis = torch.autograd.grad(albedo.sum(), dummy, create_graph=False)[0]
    ones = torch.ones(2, T, T, 1, dtype=torch.float64).requires_grad_(True)
    want = torch.autograd.grad(TM.texture(ones, texc.cpu().double(), texc_db.cpu().double()).sum(), ones)[0]
    err, scale = (vis.cpu().double() - want).abs().max().item(), want.abs().max().item()
    print('visibility_grad: max-abs error', err, 'scale', scale)
    assert vis.shape == (2, T, T, 1) and err < 2e-5 * scale + 1e-6                   # the bar of the texture gradient in test_mesh_ops.py
    assert abs(vis.double().sum().item() - 2 * S * S) < 1e-4 * 2 * S * S             # every pixel's weights sum to one


# ------------------------------------------------------------------------------------------------ 11. a fit that needs d out / d uv
def _smooth_atlas(T):
    """A few low-frequency sinusoids with whole periods over the atlas: the wrap is seamless and a shift of the coordinates is smooth."""
    y, x = torch.meshgrid((torch.arange(T) + 0.5) / T, (torch.arange(T) + 0.5) / T, indexing='ij')
    ch = [0.5 + 0.2 * torch.sin(2 * np.pi * (1 * x + 2 * y) + 0.3) + 0.2 * torch.cos(2 * np.pi * (3 * x - 1 * y)),
          0.5 + 0.3 * torch.sin(2 * np.pi * (2 * x + 1 * y) + 1.1) + 0.1 * torch.cos(2 * np.pi * (1 * x + 3 * y)),
          0.5 + 0.25 * torch.cos(2 * np.pi * (2 * x - 2 * y) + 0.7) + 0.15 * torch.sin(2 * np.pi * (3 * y))]
    return torch.stack(ch, dim=-1)[None].float()


def test_texture_coordinate_offset_fit_needs_the_uv_gradient(lib):
    """A textured sphere from 4 views, target = the same mesh with every vt shifted by a common offset of about one texel; the unknown is that
    offset (vertices fixed), Adam through rasterize -> interpolate -> texture.  With uv detached delta receives no gradient at all; through the
    full path the loss falls and delta ends closer to the true offset than it started.
    Measured on an MI355X (120 Adam steps, lr 5e-4, true offset (1, -0.75) texels of the 256^2 atlas): loss 4.564e-04 -> 5.868e-10 (ratio
    1.3e-06), offset error 1.250 -> 0.001 texels.  Only the fall of the loss and the approach are asserted."""
    from scene import face_atlas, icosphere
    dr = _dr()
    S, T = 64, 256
    v, f = icosphere(3, 0.6)
    vt, ft = face_atlas(f)
    pos = NC.clip_views(v, angles=(0.3, 1.1, 2.4, 4.0)).cuda()
    tri, ftc, vtc = torch.from_numpy(f.astype(np.int32)).cuda(), torch.from_numpy(ft.astype(np.int32)).cuda(), torch.from_numpy(vt)[None].cuda()
    tex = _smooth_atlas(T).cuda()
    true = torch.tensor([1.0 / T, -0.75 / T], device='cuda')
    ctx = dr.RasterizeCudaContext()
    rast, db = dr.rasterize(ctx, pos, tri, (S, S))
    fg = (rast[..., 3:] > 0).float()

    def render(coords, detach_uv=False):
        uv, da = dr.interpolate(coords, rast, ftc, rast_db=db, diff_attrs='all')
        if detach_uv:
            uv, da = uv.detach(), da.detach()
        return dr.texture(tex, uv, uv_da=da) * fg
    with torch.no_grad():
        target = render(vtc + true)
    delta = torch.zeros(2, device='cuda', requires_grad=True)
    loss = ((render(vtc + delta, detach_uv=True) - target) ** 2).sum() / fg.sum()
    assert not loss.requires_grad                                   # uv detached: nothing reaches delta, nothing would move
    opt = torch.optim.Adam([delta], lr=5e-4)
    losses = []
    for _ in range(120):
        loss = ((render(vtc + delta) - target) ** 2).sum() / fg.sum()
        opt.zero_grad()
        loss.backward()
        assert torch.isfinite(delta.grad).all() and (len(losses) > 0 or delta.grad.abs().max().item() > 0)
        opt.step()
        losses.append(loss.item())
    err0, err1 = true.norm().item(), (delta.detach() - true).norm().item()
    print(f'offset fit: loss {losses[0]:.3e} -> {losses[-1]:.3e} (ratio {losses[-1] / losses[0]:.3e}); offset error {err0 * T:.3f} -> {err1 * T:.3f} texels')
    assert losses[-1] < losses[0] and err1 < err0


# ------------------------------------------------------------------------------------------------ 12. contracts
def test_first_order_only_grad_db_and_pos_gradient_boost(lib):
    dr = _dr()
    S = 32
    sc = NC.sphere_scene(S, 64)
    tri, ft = sc['tri'].cuda(), sc['ft'].cuda()
    ctx = dr.RasterizeCudaContext()
    # create_graph=True: the first-order gradients are there, differentiating them raises
    pos, vt, tex = (sc[k].cuda().requires_grad_(True) for k in ('pos', 'vt', 'tex'))
    rast, db = dr.rasterize(ctx, pos, tri, (S, S))
    uv, da = dr.interpolate(vt, rast, ft, rast_db=db, diff_attrs='all')
    out = dr.antialias(dr.texture(tex, uv, uv_da=da), rast, pos, tri)
    grads = torch.autograd.grad((out ** 2).sum(), [pos, vt, tex], create_graph=True)
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 and g.requires_grad for g in grads)
    for g in grads:
        with pytest.raises(RuntimeError, match='second-order'):
            torch.autograd.grad(g.sum(), [pos, vt, tex], retain_graph=True, allow_unused=True)
    # grad_db=False: rast_db is detached, rast still carries the gradient
    p = sc['pos'].cuda().requires_grad_(True)
    r, d = dr.rasterize(ctx, p, tri, (S, S), grad_db=False)
    assert d.grad_fn is None and not d.requires_grad and r.grad_fn is not None
    r2, d2 = dr.rasterize(ctx, p, tri, (S, S))
    assert d2.grad_fn is not None and torch.equal(d2, d)
    r3, d3 = dr.rasterize(ctx, p.detach(), tri, (S, S))
    assert r3.grad_fn is None and d3.grad_fn is None
    # pos_gradient_boost scales the silhouette gradient linearly (and nothing else)
    color = torch.rand(2, S, S, 3, generator=torch.Generator().manual_seed(3)).cuda()
    g_out = torch.randn(2, S, S, 3, generator=torch.Generator().manual_seed(4)).cuda()
    got = {}
    for boost in (1.0, 2.5):
        p, c = sc['pos'].cuda().requires_grad_(True), color.clone().requires_grad_(True)
        (dr.antialias(c, rast.detach(), p, tri, pos_gradient_boost=boost) * g_out).sum().backward()
        got[boost] = (p.grad, c.grad)
    assert got[1.0][0].abs().sum() > 0 and torch.equal(got[2.5][1], got[1.0][1])
    assert NC.rel_l2(got[2.5][0], 2.5 * got[1.0][0]) <= 1e-5             # (float atomics: the summation order differs from run to run)
