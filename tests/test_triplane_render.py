"""Rendering tri-plane scenes: mve_triplane_render_rays behind TriPlaneDecoder.render_rays, the NeRFRenderer.render seam and
TriPlaneVolumeRenderer, against the CPU statement tests/triplane_render_rule.py (the oracle's eval loop / training forward with the pinned
decode rules receiving the marched directions).

Scene (shared): the golden weights of the dir-net cases `ssd` / `stable` / `wide` (tests/golden/triplane_dirnet_ref.npz) and of the
default-topology case `plain` (tests/golden/triplane_ref.npz), seeded code planes of the goldens' shapes, the bitfield of
sphere_density_grid(64, 0.55) packed at 0.5, rays scene_rays(2, 24).  DENSITY_BIAS is added to density_net.0.bias so that the rule alone
meets the conditioning of test_scene_conditioning_under_the_rule (rays that saturate AND rays that leave the box unsaturated).

Bars: ws / image / depth of the fused render 1e-4 absolute (test_nerf.py's bar for the same compositing over a decode held to 2e-5); the seam,
the training forward and the gradients carry the bars of the iNGP tests they mirror (test_gpu_nerf_render_seam, test_gpu_train_branch_forward,
test_triplane.py's gradient bar)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_triplane as TT  # noqa: E402
import test_triplane_dirnet as TD  # noqa: E402
import triplane_render_rule as RR  # noqa: E402
from oracle import nerf_oracle as NO  # noqa: E402
from oracle import raymarching as ORM  # noqa: E402
from oracle import triplane_oracle as TO  # noqa: E402
from scene import camera_rays as scene_rays, sphere_density_grid  # noqa: E402

GRID = 64
T_THRESH = 1e-2
DIRNET = ('ssd', 'stable', 'wide')
CASES = DIRNET + ('plain',)
DT_GAMMAS = (0.0, 1.0 / 256)
# added to density_net.0.bias, chosen on the rule alone: without it no ray of the sphere saturates (the goldens' densities are O(1)), with
# 0.5 more fewer than a quarter of the hit rays stay unsaturated
DENSITY_BIAS = dict(ssd=1.5, stable=2.0, wide=2.0, plain=2.0)
_cache = {}


def bits():
    if 'bits' not in _cache:
        _cache['bits'] = ORM.packbits(sphere_density_grid(GRID, radius=0.55), 0.5)
    return _cache['bits']


def rays():
    if 'rays' not in _cache:
        _cache['rays'] = scene_rays(2, 24)
    return _cache['rays']


def code_planes(tag):
    shape = (TD.G if tag in DIRNET else TT.G)[f'{tag}_code'].shape                  # [1, 3, C, h, w]
    return torch.randn(*shape, generator=torch.Generator().manual_seed(17 + CASES.index(tag))) * 0.7


def rule_weights(tag, dtype=torch.float32, zero_dir_net=False):
    if tag in DIRNET:
        w = TD.weights(tag, dtype)
        w['density_net.0.bias'] = w['density_net.0.bias'] + DENSITY_BIAS[tag]
        if zero_dir_net:
            w['dir_net.0.weight'], w['dir_net.0.bias'] = torch.zeros_like(w['dir_net.0.weight']), torch.zeros_like(w['dir_net.0.bias'])
    else:
        w = TT.weights(tag, dtype)
        w['dens_b'] = w['dens_b'] + DENSITY_BIAS[tag]
    return w


def rule_decode_torch(tag, xyz, dirs, code, w, table=None):
    """the pinned decode rule of the case's topology on torch tensors (differentiable w.r.t. code and w)"""
    if tag in DIRNET:
        return TD.rule(tag, xyz, dirs, code, w, table)
    c = TT.CASES[tag]
    hash_ = dict(TT.HASH, table=TT.G[f'{tag}_table'] if table is None else table) if c['ingp'] else None
    return TO.point_decode(xyz, dirs, code, w, c['plane_cfg'], c['flip_z'], c['activation'], hash=hash_)


def rule_decode(tag, code=None, w=None, colour_dirs=None):
    """decode(xyzs, dirs) for the rule's loops; colour_dirs(dirs) replaces the directions the colour sees"""
    code = code_planes(tag)[0] if code is None else code
    w = rule_weights(tag) if w is None else w

    def decode(xyzs, dirs):
        d = dirs if colour_dirs is None else colour_dirs(dirs)
        with torch.no_grad():
            sig, rgb = rule_decode_torch(tag, torch.from_numpy(np.ascontiguousarray(xyzs)), torch.from_numpy(np.ascontiguousarray(d)), code, w)
        return sig.numpy(), rgb.numpy()
    return decode


def rule_render(tag, dt_gamma):
    """the rule's eval render of the shared scene, computed once per (case, dt_gamma) -> (ws, depth, image, n_samples, trace)"""
    key = ('render', tag, dt_gamma)
    if key not in _cache:
        o, d = rays()
        _cache[key] = RR.render_rays_eval(o, d, bits(), GRID, rule_decode(tag), dt_gamma=dt_gamma, max_steps=512, T_thresh=T_THRESH, trace=True)
    return _cache[key]


def engine(tag, device='cuda', zero_dir_net=False, **kw):
    from mvedit_amd.triplane import TriPlaneDecoder, TriPlaneiNGPDecoder
    if tag in DIRNET:
        c, sd = TD.CASES[tag], TD.state_dict(tag)
        if zero_dir_net:
            sd['dir_net.0.weight'], sd['dir_net.0.bias'] = torch.zeros_like(sd['dir_net.0.weight']), torch.zeros_like(sd['dir_net.0.bias'])
    else:
        c, G = TT.CASES[tag], TT.G
        sd = {'base_net.0.weight': G[f'{tag}_base_w'], 'base_net.0.bias': G[f'{tag}_base_b'], 'density_net.0.weight': G[f'{tag}_dens_w'],
              'density_net.0.bias': G[f'{tag}_dens_b'], 'color_net.0.weight': G[f'{tag}_col1_w'], 'color_net.0.bias': G[f'{tag}_col1_b'],
              'color_net.2.weight': G[f'{tag}_col2_w'], 'color_net.2.bias': G[f'{tag}_col2_b']}
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)).clone() for k, v in sd.items()}
    sd['density_net.0.bias'] = sd['density_net.0.bias'] + DENSITY_BIAS[tag]
    kw = dict(dict(plane_cfg=c['plane_cfg'], activation=c['activation'], flip_z=c['flip_z'], device=device, max_steps=512), **kw)
    eng = TriPlaneiNGPDecoder(n_levels=12, max_resolution=320, log2_hashmap_size=12, **kw) if c['ingp'] else TriPlaneDecoder(**kw)
    return eng.load_state_dict(sd)


# ---- CPU: the rule -----------------------------------------------------------------------------------------------------------------------
def test_new_loop_equals_the_oracle_loop_for_a_direction_blind_decode():
    """with a decode that ignores dirs, RR.render_rays_eval returns NO.render_rays_eval(..., decode=...) bit for bit"""
    o, d = rays()
    dec = rule_decode('ssd', colour_dirs=lambda dirs: np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (dirs.shape[0], 1)))
    blind = lambda xyzs: dec(xyzs, np.zeros_like(xyzs))
    for dt_gamma in DT_GAMMAS:
        a = RR.render_rays_eval(o, d, bits(), GRID, dec, dt_gamma=dt_gamma, max_steps=512, T_thresh=T_THRESH)
        b = NO.render_rays_eval(o, d, bits(), GRID, None, dt_gamma=dt_gamma, max_steps=512, T_thresh=T_THRESH, decode=blind)
        assert a[3] == b[3] and a[3] > 1000
        for x, y in zip(a[:3], b[:3]):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize('dt_gamma', DT_GAMMAS)
@pytest.mark.parametrize('tag', CASES)
def test_scene_conditioning_under_the_rule(tag, dt_gamma):
    ws, depth, image, n_samples, tr = rule_render(tag, dt_gamma)
    hit = tr['counts'] > 0
    near = tr['margin'] < 1e-4
    stats = dict(hit=hit.mean(), stopped=tr['stopped'][hit].mean(), unsaturated=(ws[hit] < 0.99).mean(), median=np.median(tr['counts'][hit]),
                 near_threshold=near.mean(), n_samples=n_samples)
    print(tag, dt_gamma, {k: round(float(v), 4) for k, v in stats.items()})
    assert stats['hit'] > 0.10
    assert stats['stopped'] >= 0.25 and stats['unsaturated'] >= 0.25
    assert stats['median'] >= 4
    assert stats['near_threshold'] <= 0.01
    assert (ws[~hit] == 0).all() and (image[~hit] == 0).all()
    # rgb along a ray depends on the direction: the colour seeing the OTHER view's directions moves the image
    half = rays()[1].shape[0] // 2
    o, d = rays()
    lut = {v.tobytes(): d[(i + half) % (2 * half)] for i, v in enumerate(d)}
    swap = lambda dirs: np.stack([lut[v.tobytes()] if v.any() else v for v in dirs]).astype(np.float32)
    _, _, image2, _ = RR.render_rays_eval(o, d, bits(), GRID, rule_decode(tag, colour_dirs=swap), dt_gamma=dt_gamma, max_steps=512, T_thresh=T_THRESH)
    assert np.abs(image2 - image).max() > 1e-2


# ---- CPU: the Python surface ---------------------------------------------------------------------------------------------------------------
def test_from_config_reads_max_steps_and_min_near():
    pytest.importorskip('mvedit_amd._lib')
    from mvedit_amd.triplane import TriPlaneDecoder
    base = TD.CFGS['configs']['paper_cfgs/ssdnerf_cars_uncond.py']
    dec = TriPlaneDecoder.from_config(dict(base, max_steps=1024, min_near=0.05), device='cpu')
    assert dec.max_steps == 1024 and dec.min_near == 0.05
    plain = TriPlaneDecoder.from_config({k: v for k, v in base.items() if k not in ('max_steps', 'min_near')}, device='cpu')
    assert plain.max_steps == 256 and plain.min_near == 0.2                             # VolumeRenderer's defaults
    assert TriPlaneDecoder(device='cpu', max_steps=64, min_near=0.1).max_steps == 64


def test_nerf_renderer_routes_on_the_decoder_type(monkeypatch):
    pytest.importorskip('mvedit_amd._lib')
    from mvedit_amd import nerf
    from mvedit_amd.triplane import TriPlaneDecoder
    seen = {}
    n = 2 * 4 * 4
    out = (torch.zeros(n), torch.zeros(n), torch.zeros(n, 3))
    monkeypatch.setattr(nerf, 'camera_rays', lambda intr, pose, h, w: (torch.zeros(n, 3), torch.ones(n, 3), torch.ones(2, h, w)))

    class Tri(TriPlaneDecoder):
        def render_rays(self, rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma=0.0, **kw):
            seen['tri'] = (code, density_bitfield.shape, grid_size, dt_gamma)
            return out

    class INGP:
        def render_rays(self, rays_o, rays_d, density_bitfield, grid_size, dt_gamma=0.0, **kw):
            seen['ingp'] = (density_bitfield.shape, grid_size, dt_gamma)
            return out

    code = torch.zeros(1, 3, 2, 4, 4)
    intr, poses = torch.tensor([[[8.0, 8.0, 2.0, 2.0]] * 2]), torch.eye(4)[None, None, :3].repeat(1, 2, 1, 1)
    nr = nerf.NeRFRenderer(grid_size=8)
    bf = torch.zeros(1, 64, dtype=torch.uint8)
    img, depth = nr.render(Tri(device='cpu'), code, bf, 4, 4, intr, poses, cfg=dict(dt_gamma_scale=1.0))
    assert seen['tri'][0] is code and seen['tri'][1:] == (torch.Size([64]), 8, 0.125) and img.shape == (1, 2, 4, 4, 3) and 'ingp' not in seen
    nr.render(INGP(), code, bf, 4, 4, intr, poses, cfg=dict(dt_gamma_scale=1.0))
    assert seen['ingp'] == (torch.Size([64]), 8, 0.125)


def test_refusals_raise_before_any_launch():
    pytest.importorskip('mvedit_amd._lib')
    from mvedit_amd.triplane import TriPlaneVolumeRenderer
    dec = engine('ssd', device='cpu')
    code = code_planes('ssd')
    o, d = (torch.from_numpy(a) for a in rays())
    bf = torch.from_numpy(bits())
    with pytest.raises(NotImplementedError, match='pre_gamma'):
        TriPlaneVolumeRenderer(dec, pre_gamma=2.2)
    with pytest.raises(NotImplementedError, match='post_gamma'):
        TriPlaneVolumeRenderer(dec, post_gamma=2.2)
    vr = TriPlaneVolumeRenderer(dec)
    assert (vr.min_near, vr.max_steps, vr.bound) == (dec.min_near, 512, 1.0)
    vr.training = True
    with pytest.raises(NotImplementedError, match='capacity'):
        vr.forward(o, d, code, bf, GRID, capacity=4096)
    with pytest.raises(NotImplementedError, match='compute_normal'):
        vr.forward(o, d, code, bf, GRID, compute_normal=True)
    for training in (True, False):
        vr.training = training
        with pytest.raises(NotImplementedError, match='code'):
            vr.forward(o, d, torch.cat([code, code]), bf, GRID)
        with pytest.raises(NotImplementedError, match='rays_o'):
            vr.forward(torch.stack([o, o]), torch.stack([d, d]), code, bf, GRID)
    with pytest.raises(NotImplementedError, match='code'):
        vr.update_extra_state(torch.cat([code, code]), torch.zeros(1, 512), torch.zeros(1, 64, dtype=torch.uint8), 0)
    with pytest.raises(NotImplementedError, match='forward only'):
        dec.render_rays(o, d, code.clone().requires_grad_(True), bf, GRID)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize('dt_gamma', DT_GAMMAS)
@pytest.mark.parametrize('tag', CASES)
def test_gpu_fused_render_matches_the_rule(lib, tag, dt_gamma):
    """| case, dt_gamma | measured max |d| ws / image / depth | bar 1e-4 |: printed by the test (run with -s)."""
    ws_o, dep_o, img_o, n_rule, tr = rule_render(tag, dt_gamma)
    o, d = rays()
    eng = engine(tag)
    render = lambda *a, **k: eng.render_rays(*a, fused=True, **k)          # the kernel under test, whatever the default picks
    ws, dep, img, cnt = render(_t(o), _t(d), code_planes(tag).cuda(), _t(bits()), GRID, dt_gamma, T_thresh=T_THRESH, return_counts=True)
    keep = ~(tr['margin'] < 1e-4)
    assert (~keep).mean() <= 0.01
    errs = {}
    for name, got, want in (('ws', ws, ws_o), ('image', img, img_o), ('depth', dep, dep_o)):
        errs[name] = float(np.abs(got.cpu().numpy() - want)[keep].max())
    print(f'{tag} dt_gamma {dt_gamma:.5f}: max |d| ws {errs["ws"]:.2e} image {errs["image"]:.2e} depth {errs["depth"]:.2e} (bar 1e-4), '
          f'excluded {(~keep).sum()} of {keep.size} rays, samples {int(cnt.sum())} / rule {n_rule}')
    for name, e in errs.items():
        assert e <= 1e-4, (tag, dt_gamma, name, e)
    cnt = cnt.cpu().numpy()
    assert 0.9 * n_rule <= int(cnt.sum()) <= n_rule
    assert (cnt[tr['counts'] == 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('tag', CASES)
def test_gpu_fused_render_properties(lib, tag):
    o, d = rays()
    eng = engine(tag)
    render = lambda *a, **k: eng.render_rays(*a, fused=True, **k)          # the kernel under test, whatever the default picks
    code, bf, o, d = code_planes(tag).cuda(), _t(bits()), _t(o), _t(d)
    dt_gamma = 1.0 / 256
    ws, dep, img, cnt = render(o, d, code, bf, GRID, dt_gamma, return_counts=True)
    again = render(o, d, code, bf, GRID, dt_gamma)
    assert len(again) == 3 and torch.equal(ws, again[0]) and torch.equal(dep, again[1]) and torch.equal(img, again[2])      # deterministic; counts optional
    N = o.shape[0]
    # (1152 rays are 18 whole waves) a subset in another order, 301 = 4 waves and a partial one
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:301].cuda()
    a = render(o[idx].contiguous(), d[idx].contiguous(), code, bf, GRID, dt_gamma)
    assert torch.equal(a[0], ws[idx]) and torch.equal(a[1], dep[idx]) and torch.equal(a[2], img[idx])
    hit = int(torch.nonzero(cnt > 0)[0])
    one = render(o[hit:hit + 1], d[hit:hit + 1], code, bf, GRID, dt_gamma, return_counts=True)           # N = 1
    assert torch.equal(one[0], ws[hit:hit + 1]) and torch.equal(one[2], img[hit:hit + 1]) and torch.equal(one[3], cnt[hit:hit + 1])
    e = render(o[:0], d[:0], code, bf, GRID, dt_gamma, return_counts=True)                              # N = 0
    assert [tuple(t.shape) for t in e] == [(0,), (0,), (0, 3), (0,)]
    z = render(o, d, code, torch.zeros_like(bf), GRID, dt_gamma, return_counts=True)                    # nothing occupied
    assert all(float(t.abs().sum()) == 0 for t in z)
    if tag in DIRNET:
        # with dir_net zeroed the image no longer depends on the direction: the rule marched along the same rays with another colour direction
        eng0 = engine(tag, zero_dir_net=True)
        img0 = eng0.render_rays(o, d, code, bf, GRID, dt_gamma, fused=True)[2].cpu().numpy()
        on, dn = rays()
        w0 = rule_weights(tag, zero_dir_net=True)
        other = lambda dirs: np.roll(dirs, 1, axis=1)
        for colour_dirs in (None, other):
            ref = RR.render_rays_eval(on, dn, bits(), GRID, rule_decode(tag, w=w0, colour_dirs=colour_dirs), dt_gamma=dt_gamma, max_steps=512,
                                      T_thresh=T_THRESH, trace=True)
            keep = ~(ref[4]['margin'] < 1e-4)
            assert np.abs(img0 - ref[2])[keep].max() <= 1e-4
        assert np.abs(img0 - img.cpu().numpy()).max() > 1e-2


def _tri_nerf_render(tag, bitfield, h, w, intrinsics, poses, dt_gamma_scale, normal_bg=(0.5, 0.5, 1.0)):
    """NO.nerf_render with the tri-plane decode"""
    b = intrinsics.shape[0]
    dt_gamma = float(dt_gamma_scale * 2 / (intrinsics[:, 0] + intrinsics[:, 1]).mean())
    directions = NO.get_ray_directions(h, w, intrinsics)
    rays_o, rays_d = NO.get_rays(directions, poses, norm=True)
    ws, depth, image, _ = RR.render_rays_eval(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3), bitfield, GRID, rule_decode(tag), dt_gamma=dt_gamma,
                                              max_steps=512, T_thresh=T_THRESH)
    rgba = np.concatenate([image, ws[:, None]], -1).reshape(b, h, w, 4)
    depth = depth.reshape(b, h, w) * np.linalg.norm(directions, axis=-1)
    normal_fg = NO.depth_to_normal(depth / np.maximum(rgba[..., 3], np.float32(1e-6)), directions)
    normal = normal_fg * rgba[..., 3:] + np.asarray(normal_bg, np.float32) * (1 - rgba[..., 3:])
    return rgba.astype(np.float32), depth.astype(np.float32), normal.astype(np.float32)


@pytest.mark.gpu
def test_gpu_nerf_render_seam(lib):
    """NeRFRenderer.render(decoder, code, ...) with a tri-plane decoder, 3 surround views at 24^2, cfg=dict(dt_gamma_scale=1.0) (what
    Adapter3DRunner's preview passes), both return_rgba forms and compute_normal; bars as test_nerf.py::test_gpu_nerf_render_seam.  An
    INGPDecoderParams call returns the bits of its own render_rays, as before."""
    from mvedit_amd import nerf
    tag = 'stable'
    eng = engine(tag)
    g = np.load(os.path.join(HERE, 'golden', 'reference_py.npz'))
    S = 24
    f = S / (2 * np.tan(np.deg2rad(15)))
    intr = np.tile(np.array([[f, f, S / 2, S / 2]], np.float32), (3, 1))
    poses = g['poses'][:6:2, :3]
    rgba_o, depth_o, normal_o = _tri_nerf_render(tag, bits(), S, S, intr, poses, 1.0)
    nr = nerf.NeRFRenderer(grid_size=GRID)
    code, bf = code_planes(tag).cuda(), _t(bits())[None]
    args = (S, S, _t(intr)[None], _t(poses)[None])
    rgba, depth, normal, nfg = nr.render(eng, code, bf, *args, cfg=dict(return_rgba=True, compute_normal=True, dt_gamma_scale=1.0))
    assert rgba.shape == (1, 3, S, S, 4) and depth.shape == (1, 3, S, S) and normal.shape == (1, 3, S, S, 3)
    rgb, depth2 = nr.render(eng, code, bf, *args, cfg=dict(dt_gamma_scale=1.0))
    assert rgb.shape == (1, 3, S, S, 3) and torch.equal(depth2, depth)
    rgb_o = rgba_o[..., :3] + 1.0 * (1 - rgba_o[..., 3:])
    for got, ref, name in ((rgba, rgba_o, 'rgba'), (rgb, rgb_o, 'rgb'), (depth, depth_o, 'depth'), (normal, normal_o, 'normal')):
        err = np.abs(got[0].cpu().numpy() - ref)
        assert (err < 1e-3).mean() > 0.995 and err.mean() < 1e-4, (name, err.max(), err.mean())
    assert (rgba_o[..., 3] > 0.5).mean() > 0.05
    # an iNGP decoder takes exactly the path it took: `code` is not read
    import test_nerf as TN
    _, ingp = TN._decoder(12, 320, table_scale=2.0)
    ingp.max_steps = 512
    out = nr.render(ingp, None, bf, *args, cfg=dict(return_rgba=True, dt_gamma_scale=1.0))
    ro, rd, dn = nerf.camera_rays(_t(intr), _t(poses), S, S)
    dt_gamma = float(1.0 * 2 / (_t(intr)[:, 0] + _t(intr)[:, 1]).mean())
    ws, dep, img = ingp.render_rays(ro, rd, bf.reshape(-1), GRID, dt_gamma)
    assert torch.equal(out[0], torch.cat([img, ws[:, None]], -1).view(1, 3, S, S, 4)) and torch.equal(out[1], (dep.view(3, S, S) * dn)[None])


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['stable', 'plain'])
def test_gpu_training_forward(lib, tag):
    """TriPlaneVolumeRenderer.forward, training branch, against the rule's train_forward on given noises (bars of test_gpu_train_branch_forward)"""
    from mvedit_amd.triplane import TriPlaneVolumeRenderer
    o, d = scene_rays(1, 32)
    noises = np.random.default_rng(2).random(o.shape[0]).astype(np.float32)
    ref = RR.train_forward(o, d, bits(), GRID, rule_decode(tag), noises, dt_gamma=1 / 256, max_steps=256)
    vr = TriPlaneVolumeRenderer(engine(tag, max_steps=256))
    vr.training = True
    out = vr.forward(_t(o), _t(d), code_planes(tag).cuda(), _t(bits()), GRID, dt_gamma=1 / 256, noises=_t(noises))
    M_o, M_h = ref['ts'].shape[0], out['ts'][0].shape[0]
    assert M_o > 1000 and abs(M_o - M_h) <= 3, (M_o, M_h)
    assert set(out) == {'weights', 'weights_sum', 'depth', 'image', 'rays', 'normal', 'ts'} and out['normal'] is None
    for k in ('weights_sum', 'depth', 'image'):
        a, b = out[k][0].cpu().numpy(), ref[k]
        print(tag, k, np.abs(a - b).max(), np.abs(a - b).mean())
        assert np.abs(a - b).max() < 1.5e-3 and np.abs(a - b).mean() < 1e-5, k
    assert (ref['weights_sum'] > 0.5).mean() > 0.1
    vr.training = False                                       # eval: the fused render, in the reference's result dict
    ev = vr.forward(_t(o), _t(d), code_planes(tag).cuda(), _t(bits()), GRID, dt_gamma=1 / 256)
    assert ev['weights'] is None and ev['ts'] is None and ev['image'][0].shape == (o.shape[0], 3)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['stable', 'plain'])
def test_gpu_training_forward_gradients(lib, tag):
    """loss = sum(image G) + sum(ws g) through the training forward, `code` and every parameter requiring grad, against torch autograd over
    the float64 rule (decode rule + composite_rays_train_torch) on the samples the engine kept.  Bar: 2e-4 of each tensor's magnitude + 1e-6
    (test_triplane.py's); the hash table by that file's directional finite difference; Linear gradients bit-identical run to run."""
    from mvedit_amd.triplane import TriPlaneVolumeRenderer
    o, d = scene_rays(1, 32)
    noises = np.random.default_rng(2).random(o.shape[0]).astype(np.float32)
    rng = np.random.default_rng(5)
    Gi, gw = rng.standard_normal((o.shape[0], 3)).astype(np.float32), rng.standard_normal(o.shape[0]).astype(np.float32)
    eng = engine(tag, max_steps=256)
    vr = TriPlaneVolumeRenderer(eng)
    vr.training = True
    code = code_planes(tag)

    def run():
        for p in eng.parameters().values():
            p.requires_grad_(True)
            p.grad = None
        code_d = code.cuda().requires_grad_(True)
        out = vr.forward(_t(o), _t(d), code_d, _t(bits()), GRID, dt_gamma=1 / 256, noises=_t(noises))
        loss = (out['image'][0] * _t(Gi)).sum() + (out['weights_sum'][0] * _t(gw)).sum()
        loss.backward()
        return out, code_d.grad, {k: p.grad.clone() for k, p in eng.parameters().items()}

    out, g_code, grads = run()
    ts, rays_k = out['ts'][0].cpu().numpy(), out['rays'][0].cpu().numpy()
    # the samples the engine kept: positions from (o, d, t) are not returned, so march + cull again on the engine's own tensors
    from mvedit_amd import raymarching as rm
    with torch.no_grad():
        nears, fars = rm.near_far_from_aabb(_t(o), _t(d), eng.aabb, eng.min_near)
        xyzs, dirs, ts0, rays0 = rm.march_rays_train(_t(o), _t(d), 1.0, _t(bits()), 1, GRID, nears, fars, dt_gamma=1 / 256, max_steps=256, noises=_t(noises))
        sig0, _ = eng.point_density_decode([xyzs], code.cuda())
        w0, _, _, _ = rm.batch_composite_rays_train(sig0, sig0.new_zeros(sig0.shape[0], 3), [ts0], [rays0], [ts0.shape[0]])
        xyzs, dirs, ts1, rays1 = rm.cull_samples(w0, vr.weight_culling_th, xyzs, dirs, ts0, rays0)
    assert torch.equal(ts1, out['ts'][0]) and torch.equal(rays1, out['rays'][0])
    xyz64, dir64 = xyzs.cpu().double(), dirs.cpu().double()
    table = (TD.G if tag in DIRNET else TT.G)[f'{tag}_table'] if eng.hash is not None else None

    def rule_loss(w64, code64, tab):
        sig, rgb = rule_decode_torch(tag, xyz64, dir64, code64, w64, tab)
        _, ws, _, image = RR.composite_rays_train_torch(sig, rgb, ts, rays_k)
        return (image * torch.from_numpy(Gi).double()).sum() + (ws * torch.from_numpy(gw).double()).sum()

    w64 = {k: v.clone().requires_grad_(True) for k, v in rule_weights(tag, torch.float64).items()}
    code64 = code[0].double().clone().requires_grad_(True)
    rule_loss(w64, code64, table).backward()

    def close(got, want, what):
        want = want.float()
        scale = want.abs().max().item()
        err = (got.cpu() - want).abs().max().item()
        print(f'{tag} {what}: max |d| {err:.3e}, magnitude {scale:.3e}')
        assert scale > 0 and err <= 2e-4 * scale + 1e-6, f'{tag} {what}: max |d| {err:.3e} against a gradient of magnitude {scale:.3e}'

    close(g_code[0], code64.grad, 'code planes')
    for name, gr in grads.items():
        if name == 'encoder.params':
            continue
        key = name if tag in DIRNET else TT._ONAME[name]
        close(gr.reshape(w64[key].shape), w64[key].grad, name)
    if table is not None:
        gt = grads['encoder.params'].cpu().reshape(-1, 2)
        D = np.random.default_rng(3).standard_normal(table.shape).astype(np.float32)
        eps = 1e-2
        w0_ = {k: v.detach() for k, v in w64.items()}
        with torch.no_grad():
            fd = (rule_loss(w0_, code64.detach(), table + eps * D) - rule_loss(w0_, code64.detach(), table - eps * D)).item() / (2 * eps)
        an = float((gt.double() * torch.from_numpy(D).double()).sum())
        assert abs(fd - an) <= 2e-3 * max(abs(fd), abs(an)) + 1e-4, (fd, an)
    _, _, again = run()
    for name, gr in grads.items():
        if name != 'encoder.params':
            assert torch.equal(gr, again[name]), name


@pytest.mark.gpu
def test_gpu_update_extra_state(lib):
    """update_extra_state(code, ...): a full update (iter_density < 16) with torch's generator seeded, against the rule's density_grid_update fed
    the engine's own jitter (as test_nerf.py::test_gpu_update_extra_state); the bitfield is packbits of the grid."""
    from mvedit_amd.triplane import TriPlaneVolumeRenderer
    tag = 'stable'
    eng = engine(tag)
    vr = TriPlaneVolumeRenderer(eng)
    H = 16
    n = H ** 3
    code = code_planes(tag)
    grid = torch.zeros(1, n, device='cuda')
    bitfield = torch.zeros(1, n // 8, dtype=torch.uint8, device='cuda')
    torch.manual_seed(0)
    it, th = vr.update_extra_state(code.cuda(), grid, bitfield, 0)
    torch.manual_seed(0)
    noise = torch.rand(n, 3, dtype=torch.float32, device='cuda').cpu().numpy()              # the draw update_extra_state made
    cc = np.stack(np.meshgrid(*[np.arange(H)] * 3, indexing='ij'), -1).reshape(-1, 3)
    x_o, idx_o = NO.density_grid_points(cc, noise, H)
    sig_o, _ = rule_decode(tag)(x_o, np.tile(np.array([[0, 0, 1]], np.float32), (n, 1)))
    g_o, mean_o = NO.density_grid_update(np.zeros(n, np.float32), sig_o, idx_o, 0.9)
    assert it == 1 and th == pytest.approx(min(float(mean_o), 0.01), rel=1e-5)
    np.testing.assert_allclose(grid[0].cpu().numpy(), g_o, rtol=3e-5, atol=1e-7)          # sigma: 2e-5 relative (+ a jitter ulp through the planes)
    assert (bitfield.cpu().numpy() == ORM.packbits(grid[0].cpu().numpy(), th)).all()
