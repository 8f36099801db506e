"""The attention-processor table on real engines (mvedit_amd/attn_processors.py): every case compares two routes into the SAME native calls --
the table the reference would install against the engine's own switches (`set_ip_adapter`, `mode` / `ref_dict`, a context cut on the host) --
so the comparisons are `torch.equal`.  Processor classes are the stand-ins of tests/attn_standins.py.  SMALL config, fp16, 16 x 16 latent."""
import numpy as np
import pytest
import torch

import attn_standins as S
from oracle import unet_oracle as U
from test_unet import inputs

pytestmark = pytest.mark.gpu
CFG, DT, HW = U.SMALL, torch.float16, 16


def _q(sd):
    return {k: v.to(DT).float() for k, v in sd.items()}


@pytest.fixture(scope='module')
def unet_case():
    """Shared, read-only: weights, two sets of IP weights, inputs on the device."""
    sd = _q(U.make_state_dict(CFG, seed=8))
    ip, ip2 = _q(U.make_ip_state_dict(CFG)), _q(U.make_ip_state_dict(CFG, seed=99))
    x, ctx = inputs(CFG, 2, HW, seed=4, ctx_len=77 + 16)
    return dict(sd=sd, ip=ip, ip2=ip2, x=x.to(DT).cuda(), ctx=ctx.to(DT).cuda())


def _engine(sd, ip=None):
    from mvedit_amd.unet import UNet2DConditionEngine
    return UNet2DConditionEngine.from_state_dict(dict(sd, **(ip or {})), CFG, DT)


def _run(eng, c, ctx=None, **cak):
    return eng(c['x'], 250, c['ctx'] if ctx is None else ctx, cross_attention_kwargs=cak or None)[0]


@pytest.mark.parametrize('n_img', [1, 2])
def test_ip_adapter_through_the_processor_table(lib, unet_case, n_img):
    from mvedit_amd.attn_processors import attn_processor_names
    c = unet_case
    names = attn_processor_names(CFG)
    cak = dict(num_cross_attn_imgs=n_img) if n_img > 1 else {}
    a = _engine(c['sd'], c['ip'])
    a.set_ip_adapter(16, 0.6)
    want = _run(a, c, **cak)
    b = _engine(c['sd'])
    wrap = S.CrossImageAttnProcWrapper if n_img > 1 else None
    b.set_attn_processor(S.ip_table(CFG, names, num_tokens=16, scale=1.0, wrap=wrap))
    if n_img > 1:                                                                 # joint_attn.py:40-45 wraps whatever is installed
        inner = torch.nn.ModuleList(p.base_attn_proc for p in b.attn_processors.values())
    else:
        inner = torch.nn.ModuleList(b.attn_processors.values())                  # ip_adapter.py:61-62
    inner.load_state_dict(S.ip_checkpoint(c['ip'], names))
    ips = [p for p in inner if isinstance(p, S.IPAttnProcessor)]
    for p in ips:
        p.scale = 0.6                                                             # IPAdapter.set_scale
    got = _run(b, c, **cak)
    assert torch.equal(got, want)
    if n_img > 1:
        return
    plain = _run(_engine(c['sd']), c, ctx=c['ctx'][:, :77].contiguous())
    assert not torch.equal(want, plain)                                           # the image branch matters here
    for p in ips:
        p.scale = 0.3
    a.set_ip_adapter(16, 0.3)
    assert torch.equal(_run(b, c), _run(a, c))
    inner.load_state_dict(S.ip_checkpoint(c['ip2'], names))                       # other adapter weights, loaded in place
    got2 = _run(b, c)
    a2 = _engine(c['sd'], c['ip2'])
    a2.set_ip_adapter(16, 0.3)
    assert not torch.equal(got2, _run(a, c)) and torch.equal(got2, _run(a2, c))
    b.set_attn_processor(S.AttnProcessor2_0())                                    # unload_ip_adapter
    assert torch.equal(_run(b, c, ctx=c['ctx'][:, :77].contiguous()), plain)


def test_reference_only_through_the_processor_table(lib, unet_case):
    from mvedit_amd.attn_processors import attn_processor_names
    sd = unet_case['sd']
    names = attn_processor_names(CFG)
    x, ctx = inputs(CFG, 3, HW, seed=6)
    xr, _ = inputs(CFG, 3, HW, seed=7)
    x, xr, ctx = x.to(DT).cuda(), xr.to(DT).cuda(), ctx.to(DT).cuda()

    def two_passes(eng):
        d = {}
        eng(xr, 300, ctx, cross_attention_kwargs=dict(mode='w', ref_dict=d, is_cfg_guidance=True))
        assert len(d) == 1
        out = eng(x, 300, ctx, cross_attention_kwargs=dict(mode='r', ref_dict=d, is_cfg_guidance=True))[0]
        assert len(d) == 0
        return out
    want = two_passes(_engine(sd))
    b = _engine(sd)
    b.set_attn_processor({n: S.ReferenceOnlyAttnProc(S.AttnProcessor2_0(), enabled=n.endswith('attn1.processor'), name=n) for n in names})
    got = two_passes(b)
    assert torch.equal(got, want) and not torch.equal(got, b(x, 300, ctx)[0])
    b.set_attn_processor(S.AttnProcessor2_0())
    d = {}
    with pytest.raises(ValueError, match="mode='w'"):
        b(xr, 300, ctx, cross_attention_kwargs=dict(mode='w', ref_dict=d))
    assert d == {}                                                                # refused before the store was made, before any launch


def _cn_case(seed):
    sd = _q(U.make_controlnet_state_dict(CFG, seed=seed))
    g = torch.Generator().manual_seed(seed + 100)
    return sd, torch.rand(2, 3, 8 * HW, 8 * HW, generator=g).to(DT).cuda()


def test_controlnet_ignores_the_image_tokens(lib, unet_case):
    """CNAttnProcessor(num_tokens=4) on a 93-row context: the 89 text rows, read in place."""
    from mvedit_amd._lib import MveError
    from mvedit_amd.controlnet import ControlNetEngine, MultiControlNetEngine
    c = unet_case
    (sd1, cond1), (sd2, cond2) = _cn_case(1), _cn_case(2)
    ctx, ctx89 = c['ctx'], c['ctx'][:, :89].contiguous()
    same = lambda p, q: all(torch.equal(a, b) for a, b in zip(list(p[0]) + [p[1]], list(q[0]) + [q[1]]))
    plain = ControlNetEngine.from_state_dict(sd1, CFG, DT)
    want, full = plain(c['x'], 300, ctx89, cond1, 0.7), plain(c['x'], 300, ctx, cond1, 0.7)
    assert len(want[0]) == 6
    cn = ControlNetEngine.from_state_dict(sd1, CFG, DT)
    cn.set_attn_processor(S.CNAttnProcessor(num_tokens=4))
    got = cn(c['x'], 300, ctx, cond1, 0.7)
    assert same(got, want) and not any(torch.equal(a, b) for a, b in zip(list(got[0])[1:] + [got[1]], list(full[0])[1:] + [full[1]]))
    cn.set_attn_processor(S.AttnProcessor2_0())                                   # unload: all 93 rows again
    assert same(cn(c['x'], 300, ctx, cond1, 0.7), full)
    # MultiControlNetEngine.set_attn_processor fans out; the second net accumulates into the first one's outputs
    mk = lambda: MultiControlNetEngine([ControlNetEngine.from_state_dict(sd1, CFG, DT), ControlNetEngine.from_state_dict(sd2, CFG, DT)])
    ref_multi, multi = mk(), mk()
    want2 = ref_multi(c['x'], 300, ctx89, [cond1, cond2], [0.7, 1.2])
    multi.set_attn_processor(S.CNAttnProcessor())
    got2 = multi(c['x'], 300, ctx, [cond1, cond2], [0.7, 1.2])
    assert same(got2, want2) and not same(got2, ref_multi(c['x'], 300, ctx, [cond1, cond2], [0.7, 1.2]))
    cn.set_attn_processor(S.CNAttnProcessor(num_tokens=93))
    with pytest.raises(MveError, match='cannot ignore the last 93 rows of a context of 93 rows'):
        cn(c['x'], 300, ctx, cond1, 0.7)
    cn.set_attn_processor(S.CNAttnProcessor(num_tokens=4))
    assert same(cn(c['x'], 300, ctx, cond1, 0.7), want)


def test_refusals_leave_a_real_engine_untouched(lib, unet_case):
    from mvedit_amd.attn_processors import attn_processor_names
    c = unet_case
    names = attn_processor_names(CFG)
    attn2 = [n for n in names if n.endswith('attn2.processor')]
    a = _engine(c['sd'], c['ip'])
    a.set_ip_adapter(16, 0.6)
    want = _run(a, c)
    b = _engine(c['sd'])
    half = S.ip_table(CFG, names, 16, 0.6)
    for n in attn2[::2]:
        half[n] = S.AttnProcessor2_0()
    with pytest.raises(NotImplementedError, match=attn2[0].replace('.', r'\.')):
        b.set_attn_processor(half)
    assert not b._attn_governs
    table = S.ip_table(CFG, names, 16, 0.6)
    b.set_attn_processor(table)
    torch.nn.ModuleList(b.attn_processors.values()).load_state_dict(S.ip_checkpoint(c['ip'], names))
    table[attn2[2]].scale = 0.7
    out = torch.full_like(want, float('nan'))
    with pytest.raises(ValueError, match=f'{attn2[0]} has scale=0.6 but {attn2[2]} has scale=0.7'.replace('.', r'\.')):
        b(c['x'], 250, c['ctx'], out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                                 # nothing was launched
    table[attn2[2]].scale = 0.6
    assert torch.equal(b(c['x'], 250, c['ctx'], out=out)[0], want)


def test_bake_xyz_shading_fun_unwraps_through_the_mesh(lib):
    from mvedit_amd.mesh_ops import Mesh, MeshRenderer
    from scene import face_atlas, icosphere
    v, f = icosphere(1, 0.6)
    vt, ft = face_atlas(f)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mr = MeshRenderer(near=0.01, far=100, texture_filter='linear')
    shade = lambda world_pos: world_pos * 0.5 + 0.5
    (kept,) = mr.bake_xyz_shading_fun([Mesh(t(v), t(f), t(vt), t(ft))], shade, map_size=48, dilation_iters=2)

    class UnwrappingMesh(Mesh):
        calls = 0

        def auto_uv(self):
            UnwrappingMesh.calls += 1
            self.vt, self.ft = t(vt), t(ft)
    bare = UnwrappingMesh(t(v), t(f), None, None)
    assert bare.vt is None
    (baked,) = mr.bake_xyz_shading_fun([bare], shade, map_size=48, dilation_iters=2)
    assert UnwrappingMesh.calls == 1 and torch.equal(baked.albedo, kept.albedo)
    (again,) = mr.bake_xyz_shading_fun([baked], shade, map_size=48, dilation_iters=2, force_auto_uv=True)
    assert UnwrappingMesh.calls == 2 and torch.equal(again.albedo, kept.albedo)
    with pytest.raises(AssertionError, match='UV unwrapping'):                    # a mesh object that cannot unwrap itself: as before
        mr.bake_xyz_shading_fun([Mesh(t(v), t(f), None, None)], shade, map_size=48)
