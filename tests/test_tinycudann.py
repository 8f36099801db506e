"""mvedit_amd.tinycudann.Encoding: the `tcnn.Encoding` the reference's hash-grid decoders build (lib/models/decoders/ingp_decoder.py:62-74,
triplane_ingp_decoder.py:102-114), on csrc/hashgrid_encode.hip.

not gpu : C-ABI argument checks, construction for the reference's two configs (level table == nerf.grid_meta), unsupported configs, the
          drop-in seeding `tinycudann`; with the reference tree present, its own iNGPDecoder.__init__ / init_weights run on the facade.
gpu     : forward against oracle.nerf_oracle.hashgrid_encode (F = 2, Smoothstep) and a numpy restatement (F = 1, 4, 8, Linear); d params
          against torch autograd over the oracle's decoder restatement (random and ray-ordered batches); d x against float64 autograd;
          facade + nn.Linear MLP against decoder_ref.npz (the reference's point_decode) and the fused decoder; a torch.optim.Adam fit;
          edge cases.  Table gradients come from float atomics (order-dependent rounding): 2e-4 of the gradient's scale.
"""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as NO

REF = '/root/reference/lib/models/decoders/ingp_decoder.py'
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'decoder_ref.npz')


def ref_config(n_levels, max_res, bound=1.0, base=16):
    """the encoding_config of iNGPDecoder.__init__ (ingp_decoder.py:62-74)"""
    return {"otype": "HashGrid", "n_levels": n_levels, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": base,
            "interpolation": "Smoothstep", "per_level_scale": np.exp2(np.log2(max_res * bound / base) / (n_levels - 1))}


def level_arrays(meta):
    L = len(meta)
    return ((ctypes.c_float * L)(*[m[0] for m in meta]), (ctypes.c_uint32 * L)(*[m[1] for m in meta]),
            (ctypes.c_uint32 * L)(*[m[2] for m in meta]), (ctypes.c_uint32 * L)(*[m[3] for m in meta]))


# ------------------------------------------------------------------------------------------------ restatements
def _hashed(res, size):
    stride = 1
    for _ in range(3):
        if stride > size:
            break
        stride *= res
    return size < stride


def encode_np(x01, table, meta, smooth=True, fma=True):
    """numpy float32 restatement for any F: x01 [M,3], table [rows, F] -> [M, L*F].  fma: the cell position is fmaf(scale, x, 0.5) with one
    rounding, as tiny-cuda-nn and the kernels compute it (the product of two floats is exact in float64); fma=False rounds scale * x first, as
    oracle.nerf_oracle.hashgrid_encode does -- positions then differ by up to half an ulp of scale * x (1.5e-5 at a 320 grid)."""
    x01 = np.ascontiguousarray(x01, np.float32)
    M, F = x01.shape[0], table.shape[1]
    out = np.zeros((M, len(meta) * F), np.float32)
    for lvl, (scale, res, off, size) in enumerate(meta):
        if fma:
            pos = (x01.astype(np.float64) * np.float64(np.float32(scale)) + 0.5).astype(np.float32)
        else:
            pos = (np.float32(scale) * x01 + np.float32(0.5)).astype(np.float32)
        cf = np.floor(pos)
        fr = (pos - cf).astype(np.float32)
        cell = cf.astype(np.int64).astype(np.uint32)
        w = (fr * fr * (np.float32(3) - np.float32(2) * fr)).astype(np.float32) if smooth else fr
        acc = np.zeros((M, F), np.float32)
        for corner in range(8):
            wt = np.ones(M, np.float32)
            c = []
            for d in range(3):
                up = bool(corner & (1 << d))
                wt = wt * (w[:, d] if up else np.float32(1) - w[:, d])
                c.append(cell[:, d] + np.uint32(up))
            if _hashed(res, size):
                idx = (c[0] * np.uint32(1)) ^ (c[1] * np.uint32(2654435761)) ^ (c[2] * np.uint32(805459861))
            else:
                idx = c[0] + c[1] * np.uint32(res) + c[2] * np.uint32(res * res)
            idx = idx % np.uint32(size)
            acc = acc + wt[:, None] * table[off + idx.astype(np.int64)]
        out[:, lvl * F:(lvl + 1) * F] = acc
    return out


def encode_torch(x01, table, meta, smooth=True):
    """torch restatement, differentiable in x01 and table [rows, F] (any float dtype)"""
    M32 = 0xFFFFFFFF
    feats = []
    for (scale, res, off, size) in meta:
        pos = x01 * float(np.float32(scale)) + 0.5
        cf = torch.floor(pos).detach()
        fr = pos - cf
        w = fr * fr * (3.0 - 2.0 * fr) if smooth else fr
        cell = cf.to(torch.int64) & M32
        acc = 0
        for corner in range(8):
            wt = 1.0
            c = []
            for d in range(3):
                up = bool(corner & (1 << d))
                wt = wt * (w[:, d] if up else 1.0 - w[:, d])
                c.append((cell[:, d] + int(up)) & M32)
            if _hashed(res, size):
                idx = ((c[0] * 1) & M32) ^ ((c[1] * 2654435761) & M32) ^ ((c[2] * 805459861) & M32)
            else:
                idx = (c[0] + c[1] * res + c[2] * res * res) & M32
            acc = acc + wt[:, None] * table[off + idx % size]
        feats.append(acc)
    return torch.cat(feats, 1)


def test_restatements_agree_with_the_oracle():
    """the two restatements above against oracle.nerf_oracle.hashgrid_encode where it applies (F = 2, Smoothstep)"""
    meta, rows = NO.grid_meta(12, 16, 320)
    p = NO.make_nerf_params(12, 320, seed=3, table_scale=0.5)
    x = np.random.default_rng(0).uniform(0, 1, (500, 3)).astype(np.float32)
    ref = NO.hashgrid_encode(x, p['table'], 12, 320)
    np.testing.assert_allclose(encode_np(x, p['table'], meta, fma=False), ref, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(encode_torch(torch.from_numpy(x), torch.from_numpy(p['table']), meta).numpy(), ref, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ CPU: C ABI
def test_abi_rejects_bad_arguments(lib):
    fwd, bwd = lib.raw('mve_hashgrid_encode'), lib.raw('mve_hashgrid_encode_backward')
    meta, rows = NO.grid_meta(12, 16, 320)
    sc, rs, of, sz = level_arrays(meta)
    dev = ctypes.c_void_p(256)               # never dereferenced: every case below fails before a launch

    def f(**kw):
        a = dict(x=dev, N=100, table=dev, rows=rows, F=2, L=12, sc=sc, rs=rs, of=of, sz=sz, interp=1, out=dev)
        a.update(kw)
        return fwd(a['x'], a['N'], a['table'], a['rows'], a['F'], a['L'], a['sc'], a['rs'], a['of'], a['sz'], a['interp'], a['out'], None)

    assert f(F=3) == -1 and 'n_features must be 1, 2, 4 or 8' in lib.last_error()
    assert f(L=0) == -1 and 'n_levels must be in [1, 16]' in lib.last_error()
    assert f(L=17) == -1 and 'n_levels' in lib.last_error()
    assert f(interp=2) == -1 and 'interpolation' in lib.last_error()
    assert f(sc=None) == -1 and 'null level table' in lib.last_error()
    assert f(rows=rows - 1) == -1 and 'outside the' in lib.last_error()
    assert f(x=None) == -1 and 'null pointer' in lib.last_error()
    assert f(out=None) == -1 and 'null pointer' in lib.last_error()
    assert f(N=0, x=None, table=None, out=None) == 0                 # an empty batch launches nothing
    # a hashed level (100^3 > 1000 rows) whose row count is not a power of two
    h = level_arrays([(99.0, 100, 0, 1000)])
    assert f(L=1, sc=h[0], rs=h[1], of=h[2], sz=h[3], rows=1000) == -1 and 'not a power of two' in lib.last_error()
    z = level_arrays([(15.0, 16, 0, 0)])
    assert f(L=1, sc=z[0], rs=z[1], of=z[2], sz=z[3]) == -1 and 'empty level' in lib.last_error()
    rc = bwd(dev, 100, dev, rows, 8, 12, sc, rs, of, sz, 1, None, dev, None, None)
    assert rc == -1 and 'null pointer' in lib.last_error()
    rc = bwd(dev, 100, None, rows, 2, 12, sc, rs, of, sz, 1, dev, dev, dev, None)
    assert rc == -1 and 'needs the table' in lib.last_error()
    rc = bwd(dev, 100, dev, rows, 2, 12, sc, rs, of, sz, 0, dev, None, None, None)
    assert rc == -1 and 'null pointer' in lib.last_error()
    rc = bwd(dev, 100, dev, rows, 16, 12, sc, rs, of, sz, 1, dev, dev, None, None)
    assert rc == -1 and 'n_features' in lib.last_error()


# ------------------------------------------------------------------------------------------------ CPU: construction
@pytest.mark.parametrize('n_levels,max_res,rows,n_out', [(12, 320, 3593720, 24), (14, 512, 4594792, 28)])
def test_construction_for_the_reference_configs(lib, n_levels, max_res, rows, n_out):
    from mvedit_amd import nerf
    from mvedit_amd.tinycudann import Encoding
    enc = Encoding(n_input_dims=3, encoding_config=ref_config(n_levels, max_res), dtype=torch.float32)
    assert enc.n_input_dims == 3 and enc.n_output_dims == n_out and enc.dtype == torch.float32
    assert enc.params.shape == (rows * 2,) and enc.params.dtype == torch.float32 and enc.params.device.type == 'cpu'
    assert isinstance(enc.params, torch.nn.Parameter) and enc.params.requires_grad
    assert list(enc.state_dict()) == ['params'] and [n for n, _ in enc.named_parameters()] == ['params']
    assert float(enc.params.abs().max()) <= 1e-4 and float(enc.params.std()) > 1e-5
    meta, total = nerf.grid_meta(n_levels, 16, max_res, 1.0)
    assert enc.meta == meta and enc.n_rows == total == rows
    # the oracle's statement of the same table
    ometa, orows = NO.grid_meta(n_levels, 16, max_res)
    assert orows == rows and [(float(s), r, o, n) for s, r, o, n in ometa] == meta
    # the fused renderer reads a reference-built decoder's table as params.reshape(-1, 2)
    assert enc.params.reshape(-1, 2).shape == (rows, 2)
    # a module nested as the reference nests it: the checkpoint key
    m = torch.nn.Module()
    m.encoder = enc
    assert list(m.state_dict()) == ['encoder.params']
    # the same seed gives the same table, another seed another one
    e2 = Encoding(3, ref_config(n_levels, max_res), seed=1337, dtype=torch.float32)
    e3 = Encoding(3, ref_config(n_levels, max_res), seed=7, dtype=torch.float32)
    assert torch.equal(e2.params, enc.params) and not torch.equal(e3.params, enc.params)


def test_other_grid_spellings_and_defaults(lib):
    from mvedit_amd import nerf
    from mvedit_amd.tinycudann import Encoding
    e = Encoding(3, {"otype": "Grid", "type": "Hash", "n_levels": 4, "n_features_per_level": 8, "log2_hashmap_size": 15,
                     "base_resolution": 8, "per_level_scale": 1.5, "interpolation": "Linear"}, dtype=torch.float32)
    meta, rows = nerf.level_table(4, 8, 1.5, 15)
    assert e.n_output_dims == 32 and e.params.shape == (rows * 8,) and e.interpolation == 'Linear'
    d = Encoding(3, {"otype": "HashGrid"}, dtype=torch.float32)          # tiny-cuda-nn's defaults: 16 levels, 2 features, 2^19, 16, 2.0, Linear
    assert d.n_output_dims == 32 and d.interpolation == 'Linear' and d.meta == nerf.level_table(16, 16, 2.0, 19)[0]


@pytest.mark.parametrize('kw,word', [
    (dict(dtype=None), 'dtype'),
    (dict(dtype=torch.float16), 'dtype'),
    (dict(n_input_dims=2), 'n_input_dims'),
    (dict(config=dict(otype='Frequency')), 'otype'),
    (dict(config=dict(otype='Grid', type='Dense')), 'otype'),
    (dict(config=dict(interpolation='Nearest')), 'interpolation'),
    (dict(config=dict(n_features_per_level=3)), 'n_features_per_level'),
    (dict(config=dict(n_levels=17)), 'n_levels'),
    (dict(config=dict(hash='Prime')), 'hash'),
    (dict(config=dict(stochastic_interpolation=True)), 'stochastic_interpolation'),
])
def test_unsupported_configs_raise(lib, kw, word):
    from mvedit_amd.tinycudann import Encoding
    cfg = dict(ref_config(12, 320), **kw.get('config', {}))
    with pytest.raises(NotImplementedError, match=word):
        Encoding(kw.get('n_input_dims', 3), cfg, dtype=kw.get('dtype', torch.float32))


# ------------------------------------------------------------------------------------------------ CPU: drop-in
def test_dropin_seeds_tinycudann(lib):
    from mvedit_amd import dropin, tinycudann
    assert 'tinycudann' not in sys.modules
    dropin.install()
    try:
        import tinycudann as tcnn
        assert tcnn.Encoding is tinycudann.Encoding and tcnn.__all__ == ['Encoding']
        from tinycudann import Encoding  # noqa: F401
    finally:
        dropin.uninstall()
    assert 'tinycudann' not in sys.modules


def test_late_install_rebinds_tcnn_in_imported_decoders(lib, monkeypatch):
    """ingp_decoder.py:5-8 leaves `tcnn = None` when it was imported before install(): install() rebinds it, uninstall() restores it."""
    from mvedit_amd import dropin, tinycudann
    mods = {}
    for name in ('lib.models.decoders.ingp_decoder', 'lib.models.decoders.triplane_ingp_decoder'):
        mods[name] = types.ModuleType(name)
        mods[name].tcnn = None
        monkeypatch.setitem(sys.modules, name, mods[name])
    dropin.install()
    try:
        for m in mods.values():
            assert m.tcnn is sys.modules['tinycudann'] and m.tcnn.Encoding is tinycudann.Encoding
    finally:
        dropin.uninstall()
    assert all(m.tcnn is None for m in mods.values())


@pytest.mark.skipif(not os.path.exists(REF), reason='reference tree not present')
def test_reference_decoder_constructs_on_the_facade(lib):
    """The reference's own iNGPDecoder.__init__ / init_weights (and its MLP), cut out of ingp_decoder.py with `ast` and executed with
    `tcnn` bound to the seeded module.  Stubbed: VolumeRenderer (the base: only `bound`), xavier_init, constant_init, MODULES."""
    import ast
    import importlib.util
    import torch.nn as nn
    import torch.nn.functional as F
    from mvedit_amd import dropin
    sys.dont_write_bytecode = True
    tree = ast.parse(open(REF).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'iNGPDecoder')
    cls.body = [fn for fn in cls.body if isinstance(fn, ast.FunctionDef) and fn.name in ('__init__', 'init_weights')]
    mlp = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'MLP')

    class VolumeRenderer(nn.Module):
        def __init__(self, bound=1, **kwargs):
            super().__init__()
            self.bound = bound

    def xavier_init(m, distribution='normal'):
        assert distribution == 'uniform'
        nn.init.xavier_uniform_(m.weight)
        nn.init.zeros_(m.bias)

    registry = types.SimpleNamespace(register_module=lambda: (lambda c: c))
    spec = importlib.util.spec_from_file_location('ref_activation', '/root/reference/lib/ops/activation.py')
    act = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(act)
    dropin.install()
    try:
        import tinycudann
        ns = dict(torch=torch, nn=nn, F=F, np=np, tcnn=tinycudann, VolumeRenderer=VolumeRenderer, xavier_init=xavier_init,
                  constant_init=lambda *a, **k: None, MODULES=registry, TruncExp=act.TruncExp)
        exec(compile(ast.Module([mlp, cls], []), REF, 'exec'), ns)
        for kw, n_out in ((dict(), 24), (dict(n_levels=14, max_resolution=512), 28)):
            dec = ns['iNGPDecoder'](**kw)
            assert isinstance(dec.encoder, tinycudann.Encoding) and dec.encoder.n_output_dims == n_out
            assert dec.mlp.net[0].in_features == dec.encoder.n_output_dims
            assert 'encoder.params' in dec.state_dict()
            dec.encoder.params.data.fill_(5.0)
            dec.init_weights()
            assert float(dec.encoder.params.abs().max()) <= 1e-4
    finally:
        dropin.uninstall()


# ------------------------------------------------------------------------------------------------ GPU
def _enc(n_levels=12, max_res=320, table=None, config=None):
    from mvedit_amd.tinycudann import Encoding
    e = Encoding(3, config or ref_config(n_levels, max_res), dtype=torch.float32).cuda()
    if table is not None:
        with torch.no_grad():
            e.params.copy_(torch.from_numpy(np.ascontiguousarray(table)).reshape(-1))
    return e


def _corner_points(n, seed):
    x = np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)
    x[:8] = [[-1, -1, -1], [1, 1, 1], [0, 0, 0], [1, -1, 0.5], [0.999999, 0.3, -0.7], [-1, 1, 1], [0.25, 0.25, 0.25], [1, 0, 0]]
    return ((x + np.float32(1)) / np.float32(2)).astype(np.float32)          # point_decode's (x + bound) / (2 bound)


def _ray_ordered_points(res=32, seed=6):
    """samples of a march through the test scene, in ray order ([-1, 1]^3)"""
    sys.path.insert(0, os.path.dirname(__file__))
    from scene import camera_rays, sphere_density_grid
    from oracle import raymarching as ORM
    from mvedit_amd import raymarching as rm
    bits = torch.from_numpy(ORM.packbits(sphere_density_grid(64, radius=0.6), 0.5)).cuda()
    o, d = camera_rays(1, res, seed=seed)
    o, d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32, device='cuda')
    nears, fars = rm.near_far_from_aabb(o, d, aabb, 0.2)
    xyzs, _, _, _ = rm.march_rays_train(o, d, 1.0, bits, 1, 64, nears, fars, dt_gamma=0.0, max_steps=256)
    return xyzs


@pytest.mark.gpu
@pytest.mark.parametrize('n_levels,max_res', [(12, 320), (14, 512)])
def test_gpu_forward_reference_configs(lib, n_levels, max_res):
    p = NO.make_nerf_params(n_levels, max_res, seed=7, table_scale=0.5)
    e = _enc(n_levels, max_res, p['table'])
    x = _corner_points(20000, 1)
    got = e(torch.from_numpy(x).cuda()).detach()
    assert got.shape == (20000, 2 * n_levels) and got.dtype == torch.float32
    # the oracle rounds scale * x before adding 0.5 where tiny-cuda-nn and the kernels use one fmaf: up to 1.5e-5 apart in a fine level's
    # fractional position, ~5e-5 of the table's scale in the encoding
    want = NO.hashgrid_encode(x, p['table'], n_levels, max_res)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-5, atol=1e-4 * np.abs(p['table']).max())
    meta, _ = NO.grid_meta(n_levels, 16, max_res)
    np.testing.assert_allclose(got.cpu().numpy(), encode_np(x, p['table'], meta), rtol=2e-5, atol=1e-6 * np.abs(p['table']).max())


@pytest.mark.gpu
@pytest.mark.parametrize('F,interp', [(1, 'Smoothstep'), (4, 'Smoothstep'), (8, 'Linear'), (2, 'Linear'), (4, 'Linear')])
def test_gpu_forward_other_widths_and_linear(lib, F, interp):
    cfg = {"otype": "HashGrid", "n_levels": 16 if F < 8 else 10, "n_features_per_level": F, "log2_hashmap_size": 17, "base_resolution": 8,
           "per_level_scale": 1.45, "interpolation": interp}
    e = _enc(config=cfg)
    table = np.random.default_rng(F).uniform(-1, 1, (e.n_rows, F)).astype(np.float32)
    with torch.no_grad():
        e.params.copy_(torch.from_numpy(table).reshape(-1))
    x = np.random.default_rng(2).uniform(0, 1, (8000, 3)).astype(np.float32)
    x[:3] = [[0, 0, 0], [1, 1, 1], [0.5, 1, 0]]
    got = e(torch.from_numpy(x).cuda()).detach().cpu().numpy()
    want = encode_np(x, table, e.meta, smooth=interp == 'Smoothstep')
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-6 * np.abs(table).max())


def _trunc_exp():
    class TruncExp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.save_for_backward(x)
            return torch.exp(x)

        @staticmethod
        def backward(ctx, g):
            return g * torch.exp(ctx.saved_tensors[0]).clamp(min=1e-6, max=1e6)
    return TruncExp.apply


def _head(enc_fn, x, p, b1, b2, bound=1.0, blob_density=1.0, blob_radius=0.2, sat=0.001):
    """the reference's point_decode around the encoder (ingp_decoder.py:100-118), restated: MLP, density blob, truncated exp, saturated
    sigmoid.  x [M,3] in [-bound, bound]."""
    enc = enc_fn((x + bound) / (2 * bound))
    h = torch.relu(enc @ p['w1'].t() + b1) @ p['w2'].t() + b2
    d = (x ** 2).sum(-1).clamp(min=0.2)
    sigma = _trunc_exp()(h[:, 0] + blob_density * torch.exp(-d / (2 * blob_radius ** 2)))
    rgb = torch.sigmoid(h[:, 1:]) * (1 + sat * 2) - sat
    return sigma, rgb


@pytest.mark.gpu
def test_gpu_backward_params_vs_autograd(lib):
    """d params through the reference's decode head against torch autograd over oracle.nerf_oracle.decoder_grads_torch, on a random batch
    and on a ray-ordered one (many same-cell neighbours: the lane merge); a second backward accumulates into .grad."""
    p = NO.make_nerf_params(12, 320, seed=7, table_scale=0.5)
    p['b1'] = np.random.default_rng(7).normal(0, 0.1, 64).astype(np.float32)
    p['b2'] = np.array([1.5, 0.1, -0.2, 0.3], np.float32)
    e = _enc(12, 320, p['table'])
    tp = {k: torch.from_numpy(p[k]).cuda() for k in ('w1', 'w2')}
    rng = np.random.default_rng(2)
    for x in (rng.uniform(-1, 1, (6000, 3)).astype(np.float32), _ray_ordered_points().cpu().numpy()):
        M = x.shape[0]
        gs = rng.normal(size=M).astype(np.float32) * 0.3
        gr = rng.normal(size=(M, 3)).astype(np.float32)
        ref = NO.decoder_grads_torch(x, p, gs, gr)['table']
        e.params.grad = None
        xt = torch.from_numpy(x).cuda()
        for _ in range(2):
            sigma, rgb = _head(e, xt, tp, torch.from_numpy(p['b1']).cuda(), torch.from_numpy(p['b2']).cuda())
            ((torch.from_numpy(gs).cuda() * sigma).sum() + (torch.from_numpy(gr).cuda() * rgb).sum()).backward()
        scale = np.abs(ref).max()
        assert scale > 0 and (np.abs(ref).sum(1) > 0).mean() > 0.001
        np.testing.assert_allclose(e.params.grad.cpu().numpy().reshape(-1, 2), 2 * ref, rtol=0, atol=4e-4 * scale)
    assert M > 5000            # the ray-ordered batch


@pytest.mark.gpu
@pytest.mark.parametrize('F,interp,n_levels,max_res', [(2, 'Smoothstep', 12, 320), (4, 'Linear', 8, 128), (1, 'Smoothstep', 6, 64)])
def test_gpu_backward_x_vs_float64_autograd(lib, F, interp, n_levels, max_res):
    cfg = dict(ref_config(n_levels, max_res), n_features_per_level=F, interpolation=interp)
    e = _enc(config=cfg)
    table = np.random.default_rng(3).uniform(-1, 1, (e.n_rows, F)).astype(np.float32)
    with torch.no_grad():
        e.params.copy_(torch.from_numpy(table).reshape(-1))
    x = np.random.default_rng(4).uniform(0.02, 0.98, (6000, 3)).astype(np.float32)
    # keep every level's position away from cell faces, where float32 and float64 may pick different cells
    keep = np.ones(len(x), bool)
    for (scale, res, off, size) in e.meta:
        fr = (x.astype(np.float64) * np.float32(scale) + 0.5) % 1.0
        keep &= ((fr > 0.01) & (fr < 0.99)).all(1)
    x = x[keep]
    assert len(x) > 300
    g = np.random.default_rng(5).normal(size=(len(x), e.n_output_dims)).astype(np.float32)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    (e(xt) * torch.from_numpy(g).cuda()).sum().backward()
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    (encode_torch(x64, torch.from_numpy(table).double(), e.meta, smooth=interp == 'Smoothstep') * torch.from_numpy(g).double()).sum().backward()
    want = x64.grad.numpy()
    np.testing.assert_allclose(xt.grad.cpu().numpy(), want, rtol=1e-4, atol=1e-4 * np.abs(want).max())
    # d params through the same restatement (float32 on the CPU), for this width and interpolation
    t32 = torch.from_numpy(table).requires_grad_(True)
    (encode_torch(torch.from_numpy(x), t32, e.meta, smooth=interp == 'Smoothstep') * torch.from_numpy(g)).sum().backward()
    ref = t32.grad.numpy()
    np.testing.assert_allclose(e.params.grad.cpu().numpy().reshape(-1, F), ref, rtol=0, atol=2e-4 * np.abs(ref).max())


@pytest.mark.gpu
def test_gpu_end_to_end_reference_decode(lib):
    """facade + nn.Linear MLP + the reference's head reproduce decoder_ref.npz (written by executing the reference's point_decode, see
    tests/golden/make_decoder_golden.py) and the fused decoder on the same tensors."""
    from mvedit_amd.nerf import INGPDecoderParams
    g = np.load(GOLD)
    p = NO.make_nerf_params(seed=7, table_scale=0.5)
    p['b1'], p['b2'] = g['b1'], g['b2']
    gen = torch.Generator().manual_seed(5)                     # make_decoder_golden.points()
    x = torch.rand(3000, 3, generator=gen) * 2 - 1
    x[:200] *= 0.2
    e = _enc(12, 320, p['table'])
    assert float(ref_config(12, 320)['per_level_scale']) == float(g['per_level_scale'])
    l1, l2 = torch.nn.Linear(24, 64).cuda(), torch.nn.Linear(64, 4).cuda()
    with torch.no_grad():
        for lin, w, b in ((l1, 'w1', 'b1'), (l2, 'w2', 'b2')):
            lin.weight.copy_(torch.from_numpy(p[w]))
            lin.bias.copy_(torch.from_numpy(p[b]))
        xc = x.cuda()
        h = l2(torch.relu(l1(e((xc + 1.0) / 2.0))))
        d = (xc ** 2).sum(-1).clamp(min=0.2)
        sigma = torch.exp(h[:, 0] + 1.0 * torch.exp(-d / (2 * 0.2 ** 2)))
        rgb = torch.sigmoid(h[:, 1:]) * (1 + 0.001 * 2) - 0.001
    np.testing.assert_allclose(sigma.cpu().numpy(), g['sigmas'], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(rgb.cpu().numpy(), g['rgbs'], rtol=2e-5, atol=2e-5)
    dec = INGPDecoderParams(e.params.detach().reshape(-1, 2), p['w1'], p['b1'], p['w2'], p['b2'], 12, 320)
    s_f, c_f = dec.point_decode(xc)
    np.testing.assert_allclose(sigma.cpu().numpy(), s_f.cpu().numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(rgb.cpu().numpy(), c_f.cpu().numpy(), rtol=2e-5, atol=2e-5)


@pytest.mark.gpu
def test_gpu_training_with_torch_adam(lib):
    """Encoding.params + an nn.Linear MLP under a stock torch.optim.Adam: a fitting loss falls (the reconstruct step's shape)."""
    torch.manual_seed(0)
    e = _enc(12, 320)
    mlp = torch.nn.Sequential(torch.nn.Linear(24, 64), torch.nn.ReLU(), torch.nn.Linear(64, 3)).cuda()
    x = _ray_ordered_points()
    x01 = (x + 1) / 2
    target = 0.5 + 0.4 * torch.sin(6.0 * x) * torch.cos(4.0 * x[:, [1, 2, 0]])
    opt = torch.optim.Adam(list(e.parameters()) + list(mlp.parameters()), lr=1e-2, eps=1e-15)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = ((mlp(e(x01)) - target) ** 2).mean()
        loss.backward()
        assert e.params.grad is not None and torch.isfinite(e.params.grad).all()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < 0.3 * losses[0], (losses[0], losses[-1])
    # below what any constant output reaches: the fit goes through the encoding
    assert losses[-1] < 0.5 * float(target.var(0).mean()), (losses[-1], float(target.var(0).mean()))


@pytest.mark.gpu
def test_gpu_edge_cases(lib):
    p = NO.make_nerf_params(12, 320, seed=9, table_scale=0.5)
    e = _enc(12, 320, p['table'])
    # N = 0, forward and backward
    x0 = torch.zeros(0, 3, device='cuda', requires_grad=True)
    out0 = e(x0)
    assert out0.shape == (0, 24)
    out0.sum().backward()
    assert x0.grad.shape == (0, 3) and float(e.params.grad.abs().sum()) == 0
    # N not a multiple of 64 (nor of the 256-point block), points outside [0, 1]
    x = np.random.default_rng(3).uniform(-0.5, 1.5, (1000 + 37, 3)).astype(np.float32)
    got = e(torch.from_numpy(x).cuda()).detach()
    np.testing.assert_allclose(got.cpu().numpy(), encode_np(x, p['table'], e.meta), rtol=2e-5, atol=1e-6 * 0.5)
    # non-contiguous and float64 input: a contiguous float32 copy is encoded; the gradient comes back in the input's dtype
    xt = torch.from_numpy(x).cuda()
    nc = xt.t().contiguous().t()
    assert not nc.is_contiguous()
    assert torch.equal(e(nc), got)
    x64 = xt.double().requires_grad_(True)
    assert torch.equal(e(x64), got)
    e(x64).sum().backward()
    assert x64.grad.dtype == torch.float64 and torch.isfinite(x64.grad).all()
    # CPU input: no fallback
    with pytest.raises(RuntimeError, match='GPU only'):
        e(torch.from_numpy(x))
    # second order: the backward is once-differentiable
    xg = torch.from_numpy(x[:100]).cuda().requires_grad_(True)
    (gx,) = torch.autograd.grad(e(xg).sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError, match='second-order gradients'):
        gx.sum().backward()
