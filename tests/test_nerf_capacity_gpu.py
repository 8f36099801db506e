"""Capacity (host-read-free) form of the NeRF training iteration on the GPU: sample tensors sized by a caller-chosen capacity, the live
count on the device (mve_*_n entry points, VolumeRenderer.forward(capacity=...), nerf_optim_loss(n_samples=...), adam_step(skip_if=...)).

The reference of every comparison is the existing exact entry point or path on M = count samples, or the CPU oracle -- never another
`_n` call.  Index arithmetic, the decoded head, the MLP gradients (fixed-order reduction over the same 256-row blocks), the image-space
loss and the first Adam step are the same arithmetic in the same order, so they are compared bit for bit; the table gradient is accumulated
with float atomics and is held to the project's own bounds (2e-4 of the gradient's scale against autograd, 4e-4 between two atomic runs,
tests/test_nerf.py).  Later Adam steps take their bias corrections from the device's powf instead of the host's: the moments stay
bit-equal, the parameters are held to the rounding of the two powf.

One case deviates from its specification on purpose: with weight culling on, a capacity equal to the KEPT count is below the marched
total, and the clamp step defines exactly that as an overflow.  That case therefore asserts the overflow contract (flag set, true
marched total reported, everything finite) instead of equality; every capacity at or above the marched total asserts equality."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as NO
from oracle import raymarching as ORM
from scene import camera_rays as scene_rays, sphere_density_grid
from test_nerf import _decoder

pytestmark = pytest.mark.gpu

BLOCK, XTY_ROWS = 256, 256          # decode block size (NB) and rows per partial block of the gradient reduction, csrc/nerf.hip
SIZES = sorted({0, 1, BLOCK - 1, BLOCK, BLOCK + 1, XTY_ROWS - 1, XTY_ROWS, XTY_ROWS + 1, 6000})
MLP = ('w1', 'b1', 'w2', 'b2')


def capacities(M):
    return (M, M + 1, 2 * M + 513)


def dev_count(n):
    return torch.full((1,), n, dtype=torch.int32, device='cuda')


_cache = {}


def points():
    """6000 + tail points, incoming gradients and the autograd reference of the table gradient at M = 6000 (computed once)"""
    if 'pts' not in _cache:
        p, _ = _decoder(12, 320, table_scale=0.1)
        rng = np.random.default_rng(2)
        x = rng.uniform(-1, 1, (6000, 3)).astype(np.float32)
        gs = rng.normal(size=6000).astype(np.float32) * 0.3
        gr = rng.normal(size=(6000, 3)).astype(np.float32)
        _cache['pts'] = (x, gs, gr, NO.decoder_grads_torch(x, p, gs, gr)['table'])
    return _cache['pts']


def padded(a, M, cap, fill):
    """rows [0, M) of a, then cap - M rows of `fill` (what a kernel must never load)"""
    t = torch.full((cap,) + a.shape[1:], fill, dtype=torch.float32)
    t[:M] = torch.from_numpy(a[:M])
    return t.cuda()


@pytest.mark.parametrize('M', SIZES)
def test_decode_and_backward_with_the_count_on_the_device(lib, M):
    _, dec = _decoder(12, 320, table_scale=0.1)
    x, gs, gr, table_ref = points()
    t = lambda a: torch.from_numpy(a[:M]).cuda()
    s_e, c_e = dec.point_decode(t(x))
    g_e = dec.point_decode_backward(t(x), t(gs), t(gr))
    for cap in capacities(M):
        n = dev_count(M)
        xc = padded(x, M, cap, float('nan'))                              # a tail row that were decoded would give NaN, not 0
        s, c = dec.point_decode_n(xc, n)
        assert s.shape == (cap,) and c.shape == (cap, 3)
        assert torch.equal(s[:M], s_e) and torch.equal(c[:M], c_e), (M, cap)
        assert (s[M:] == 0).all() and (c[M:] == 0).all(), (M, cap)
        s_d, none = dec.point_decode_n(xc, n, density_only=True)
        assert none is None and torch.equal(s_d, s)
        g = dec.point_decode_backward_n(xc, n, padded(gs, M, cap, float('nan')), padded(gr, M, cap, float('nan')))
        for k in MLP:
            assert torch.equal(g[k], g_e[k]), (k, M, cap)
        assert torch.isfinite(g['table']).all()
        scale = float(g_e['table'].abs().max())
        assert float((g['table'] - g_e['table']).abs().max()) <= 4e-4 * scale, (M, cap)      # two atomically accumulated results
        if M == 6000:
            ref_scale = np.abs(table_ref).max()
            np.testing.assert_allclose(g['table'].cpu().numpy(), table_ref, rtol=0, atol=2e-4 * ref_scale)
    # a count above the capacity is clamped to it, a negative one to zero: never a row outside the buffers
    if M:
        s, c = dec.point_decode_n(t(x), dev_count(M + 1000))
        assert torch.equal(s, s_e) and torch.equal(c, c_e)
        s, c = dec.point_decode_n(t(x), dev_count(-3))
        assert (s == 0).all() and (c == 0).all()


@pytest.mark.parametrize('M', SIZES)
def test_cull_with_the_count_on_the_device(lib, M):
    from mvedit_amd import raymarching as rm
    rng = np.random.default_rng(5 + M)
    cnt = []
    while sum(cnt) < M:
        c = int(rng.integers(0, 40)) if rng.random() > 0.2 else 0
        cnt.append(min(c, M - sum(cnt)))
    cnt += [0, 0, 0]                                                      # rays that meet nothing, also past the last sample
    cnt = np.asarray(cnt, np.int32)
    off = (np.cumsum(cnt) - cnt).astype(np.int32)
    rays = np.stack([off, cnt], -1).astype(np.int32)
    w = rng.random(M).astype(np.float32) * 4e-3
    w[rng.random(M) < 0.05] = 1e-3                                        # exactly at the threshold: strict '>' drops them
    xyzs, dirs = rng.normal(size=(M, 3)).astype(np.float32), rng.normal(size=(M, 3)).astype(np.float32)
    ts = rng.random((M, 2)).astype(np.float32)
    xo, do, to, ro, _ = NO.cull_samples(w, 1e-3, xyzs, dirs, ts, rays)
    kept = xo.shape[0]
    for cap in capacities(M):
        n = dev_count(M)
        wc = padded(w, M, cap, 1.0)                                       # tail weights far above the threshold: kept if they were read
        xh, dh, th, rh, n_out = rm.cull_samples_n(wc, 1e-3, padded(xyzs, M, cap, 7.0), padded(dirs, M, cap, 7.0), padded(ts, M, cap, 7.0),
                                                  torch.from_numpy(rays).cuda(), n)
        assert int(n_out) == kept and int(n) == M, (M, cap)
        assert (rh.cpu().numpy() == ro).all(), (M, cap)
        for a, b in ((xh, xo), (dh, do), (th, to)):
            assert a.shape[0] == cap and (a[:kept].cpu().numpy() == b).all() and (a[kept:] == 0).all(), (M, cap)


# --------------------------------------------------------------------------------------------------------------------------------
def inputs():
    """the training tests' scene: 64^3 grid with a sphere of radius 0.6, 2 patches of 32 x 32 rays, one noise per ray"""
    if 'inputs' not in _cache:
        H, P, ps = 64, 2, 32
        bits = torch.from_numpy(ORM.packbits(sphere_density_grid(H, radius=0.6), 0.5)).cuda()
        o, d = scene_rays(P, ps, seed=5)
        noises = np.random.default_rng(2).random(o.shape[0]).astype(np.float32)
        _cache['inputs'] = dict(H=H, P=P, ps=ps, bits=bits, o=torch.from_numpy(o).cuda(), d=torch.from_numpy(d).cuda(),
                                noises=torch.from_numpy(noises).cuda())
    return _cache['inputs']


def renderer(requires_grad=False):
    """a fresh copy of the same initial parameters: 12-level decoder, 256 steps, training mode"""
    from mvedit_amd.nerf import VolumeRenderer
    _, dec = _decoder(12, 320, table_scale=0.1)
    dec.max_steps = 256
    for t in dec.parameters().values():
        t.requires_grad_(requires_grad)
    vr = VolumeRenderer(dec)
    vr.training = True
    return vr, dec


def forward(vr, capacity, cull=True):
    i = inputs()
    vr.weight_culling_th = 1e-3 if cull else 0
    return vr.forward(i['o'], i['d'], i['bits'], i['H'], dt_gamma=0.0, noises=i['noises'], capacity=capacity)


def setup():
    """targets of the loss and the exact forward (culling on / off), computed once and left unchanged"""
    if 'scene' not in _cache:
        from mvedit_amd.tonemapping import Tonemapping
        P, ps = inputs()['P'], inputs()['ps']
        fl = ps / (2 * np.tan(np.deg2rad(15)))
        ys, xs = torch.meshgrid(torch.arange(ps, dtype=torch.float32), torch.arange(ps, dtype=torch.float32), indexing='ij')
        dirs = torch.stack([(xs + 0.5 - ps / 2) / fl, (ys + 0.5 - ps / 2) / fl, torch.ones_like(xs)], -1)[None].repeat(P, 1, 1, 1).cuda()
        vr, _ = renderer()
        with torch.no_grad():
            exact = {cull: forward(vr, None, cull) for cull in (True, False)}
        target_m = (exact[True]['weights_sum'].reshape(P, ps, ps, 1) > 0.0).float()
        target_rgbs = torch.tensor([0.8, 0.3, 0.2], device='cuda').expand(P, ps, ps, 3) * target_m + (1 - target_m)
        lights = torch.nn.functional.normalize(torch.tensor([[0.3, -0.5, -1.0]] * P, device='cuda'), dim=-1)
        _cache['scene'] = dict(dirs=dirs, target_m=target_m, target_rgbs=target_rgbs, lights=lights, patch_w=torch.ones(P, device='cuda'),
                               tm=Tonemapping(device='cuda'), exact=exact, marched=exact[False]['ts'][0].shape[0],
                               kept=exact[True]['ts'][0].shape[0])
    return _cache['scene']


def loss_of(out, n_samples=None):
    from mvedit_amd.recon_loss import nerf_optim_loss
    s = setup()
    return nerf_optim_loss(out['image'], out['weights_sum'], out['depth'], out['weights'], out['ts'][0], s['target_rgbs'], s['target_m'], s['dirs'],
                           s['patch_w'], s['lights'], tonemapping=s['tm'], shaded=True, normal_reg_weight=0.5, entropy_weight=0.2,
                           n_samples=n_samples)


def assert_same_forward(out, ref, marched, kept):
    M = ref['ts'][0].shape[0]
    assert out['n_samples'].tolist() == [marched, kept] and int(out['overflow']) == 0
    for k in ('weights_sum', 'depth', 'image'):
        assert torch.equal(out[k], ref[k]), k
    assert torch.equal(out['rays'][0], ref['rays'][0])
    assert torch.equal(out['weights'][:M], ref['weights']) and (out['weights'][M:] == 0).all()
    assert torch.equal(out['ts'][0][:M], ref['ts'][0]) and (out['ts'][0][M:] == 0).all()


@pytest.mark.parametrize('cull', (True, False))
def test_forward_capacity_equals_the_exact_forward(lib, cull):
    s = setup()
    ref, marched = s['exact'][cull], s['marched']
    kept = s['kept'] if cull else marched
    assert marched > 5000 and 0 < s['kept'] < marched
    vr, _ = renderer()
    with torch.no_grad():
        for C in (kept, marched, 2 * marched):
            out = forward(vr, C, cull)
            assert out['weights'].shape == (C,) and out['ts'][0].shape == (C, 2)
            if C >= marched:
                assert_same_forward(out, ref, marched, kept)
            else:                                                          # (culling on, C = kept count < marched total: an overflow by definition)
                assert int(out['overflow']) == 1 and int(out['n_samples'][0]) == marched and int(out['n_samples'][1]) <= C
                assert all(torch.isfinite(out[k]).all() for k in ('weights', 'weights_sum', 'depth', 'image'))


@pytest.mark.parametrize('cull', (True, False))
def test_overflow_forward_renders_exactly_the_rays_that_fit(lib, cull):
    """capacity = half the marched total: a ray whose samples fit renders as in the exact forward, bit for bit; any other ray is empty
    (with culling: re-indexed to (kept, 0); without: skipped by the composite kernels, `offset + count > capacity`)"""
    s = setup()
    ref, marched = s['exact'][cull], s['marched']
    C = marched // 2
    table = s['exact'][False]['rays'][0].long()                             # the march's own table: (offset, count) per ray
    ends = table[:, 0] + table[:, 1]
    fits = ends <= C
    live = int(ends[fits].max())
    assert 0 < live <= C and bool(fits.any()) and not bool(fits.all())
    vr, _ = renderer()
    with torch.no_grad():
        out = forward(vr, C, cull)
    assert int(out['overflow']) == 1 and int(out['n_samples'][0]) == marched
    kept = int(out['n_samples'][1])
    rays = out['rays'][0]
    assert torch.equal(rays[fits], ref['rays'][0][fits])
    if cull:
        assert kept == int((ref['rays'][0][fits][:, 1]).sum()) and kept <= live
        assert (rays[~fits, 0] == kept).all() and (rays[~fits, 1] == 0).all()
    else:
        assert kept == live and torch.equal(rays, ref['rays'][0])           # the table is the march's; the kernels skip what does not fit
    for k in ('weights_sum', 'depth', 'image'):
        got, want = out[k].reshape(fits.shape[0], -1), ref[k].reshape(fits.shape[0], -1)      # one row per ray
        assert torch.equal(got[fits], want[fits]), k
        assert (got[~fits] == 0).all(), k
    assert torch.equal(out['weights'][:kept], ref['weights'][:kept]) and (out['weights'][kept:] == 0).all()
    assert torch.equal(out['ts'][0][:kept], ref['ts'][0][:kept]) and (out['ts'][0][kept:] == 0).all()


def test_adam_on_a_device_step_counter_follows_the_host_counted_step(lib):
    """Four steps on the same gradients, host-counted against device-counted.  The moments do not see the bias corrections: bit-equal.
    The corrections are 1 - powf(beta, step) from two libraries (host, device), each within 1 ulp of beta^step < 1, i.e. within
    2 * 2^-24 of each other; so the step's update u = lr * (m / bc1) / sqrt(v / bc2) differs by at most
    |u| * 2^-23 * (1 / bc1 + 0.5 / bc2) plus a few roundings of the parameter, summed over the steps.  Step 1 is exact (beta^1)."""
    _, dec_e = renderer()
    _, dec_c = renderer()
    lr, (b1, b2) = 1e-2, (0.9, 0.999)
    st_e, st_c = {}, dec_c.adam_state()
    go = torch.zeros(1, dtype=torch.int32, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(9)
    bound = {k: torch.zeros_like(t) for k, t in dec_e.parameters().items()}
    for step in range(1, 5):
        grads = {k: torch.randn(t.shape, generator=g, device='cuda') * 1e-2 for k, t in dec_e.parameters().items()}
        before = {k: t.detach().clone() for k, t in dec_e.parameters().items()}
        dec_e.adam_step(grads, st_e, lr=lr, betas=(b1, b2))
        dec_c.adam_step(grads, st_c, lr=lr, betas=(b1, b2), skip_if=go)
        for k, t in dec_e.parameters().items():
            assert torch.equal(st_c[k][0], st_e[k][0]) and torch.equal(st_c[k][1], st_e[k][1]), (k, step)
            if step == 1:
                assert torch.equal(dec_c.parameters()[k], t), k
            else:
                u = (t.detach() - before[k]).abs()
                bound[k] += u * 2.0 ** -23 * (1 / (1 - b1 ** step) + 0.5 / (1 - b2 ** step)) + 4 * 2.0 ** -24 * t.detach().abs()
            diff = (dec_c.parameters()[k].detach() - t.detach()).abs()
            print(f'adam step {step} {k}: max diff {float(diff.max()):.3e}, max bound {float(bound[k].max()):.3e}')
            assert (diff <= bound[k]).all(), (k, step)
    assert int(st_c['step']) == 4 and st_e['step'] == 4


def iteration(vr, dec, state, capacity, lr=1e-2):
    """forward -> nerf_optim_loss -> backward through composite and the hash grid -> native Adam"""
    for t in dec.parameters().values():
        t.grad = None
    out = forward(vr, capacity)
    res = loss_of(out, None if capacity is None else out['n_samples'])
    res['loss'].backward()
    grads = {k: t.grad for k, t in dec.parameters().items()}
    dec.adam_step(grads, state, lr=lr, skip_if=None if capacity is None else out['overflow'])
    return out, res, grads


def test_whole_iteration_exact_against_capacity(lib):
    from mvedit_amd.recon_loss import PARTS
    s = setup()
    vr_e, dec_e = renderer(True)
    vr_c, dec_c = renderer(True)
    out_e, res_e, g_e = iteration(vr_e, dec_e, {}, None)
    out_c, res_c, g_c = iteration(vr_c, dec_c, dec_c.adam_state(), s['marched'] + s['marched'] // 4)
    assert_same_forward(out_c, out_e, s['marched'], s['kept'])
    for k in PARTS:
        assert torch.isfinite(res_c[k]) and torch.equal(res_c[k], res_e[k]), (k, float(res_c[k]), float(res_e[k]))
    assert float(res_e['entropy_loss']) != 0
    assert torch.equal(res_c['out_rgbs'], res_e['out_rgbs']) and torch.equal(res_c['out_normals'], res_e['out_normals'])
    initial = renderer()[1].parameters()
    for k in MLP:
        assert torch.equal(g_c[k], g_e[k]), k
        assert torch.equal(dec_c.parameters()[k], dec_e.parameters()[k]), k
        assert not torch.equal(dec_c.parameters()[k], initial[k]), k          # the step did move it
    scale = float(g_e['table'].abs().max())
    assert scale > 0 and float((g_c['table'] - g_e['table']).abs().max()) <= 4e-4 * scale


def test_capacity_iterations_never_read_on_the_host(lib):
    s = setup()
    vr, dec = renderer(True)
    state = dec.adam_state()
    C = 2 * s['marched']
    iteration(vr, dec, state, C)                                            # lazy initialisation happens outside the checked region
    vr_e, dec_e = renderer(True)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        for _ in range(3):
            iteration(vr, dec, state, C)
        with pytest.raises(RuntimeError):                                   # the check can fail: the exact path reads its counts
            iteration(vr_e, dec_e, {}, None)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert int(state['step']) == 4


def test_overflow_is_a_flag_and_skips_the_step(lib):
    s = setup()
    vr, dec = renderer(True)
    state = dec.adam_state()
    g = torch.Generator(device='cuda').manual_seed(3)
    for k in dec.parameters():                                              # a state in mid-training: non-trivial moments, step 5
        for m in state[k]:
            m.copy_(torch.rand(m.shape, generator=g, device='cuda') * 1e-3)
    state['step'].fill_(5)
    before = {k: t.detach().clone() for k, t in dec.parameters().items()}
    moments = {k: (state[k][0].clone(), state[k][1].clone()) for k in dec.parameters()}
    out, res, grads = iteration(vr, dec, state, s['marched'] // 2)
    assert int(out['overflow']) != 0 and int(out['n_samples'][0]) == s['marched']
    assert int(out['n_samples'][1]) <= s['marched'] // 2
    for k in ('weights', 'weights_sum', 'depth', 'image'):
        assert torch.isfinite(out[k]).all(), k
    assert all(torch.isfinite(v).all() for v in res.values()) and all(torch.isfinite(v).all() for v in grads.values())
    assert int(state['step']) == 5
    for k, t in dec.parameters().items():
        assert torch.equal(t.detach(), before[k]), k
        assert torch.equal(state[k][0], moments[k][0]) and torch.equal(state[k][1], moments[k][1]), k
    # the caller grows the capacity to the reported total and continues: the exact result
    with torch.no_grad():
        assert_same_forward(forward(vr, int(out['n_samples'][0])), s['exact'][True], s['marched'], s['kept'])

