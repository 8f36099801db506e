"""CLIPVisionEngine, ResamplerEngine and ImageProjEngine without a GPU: construction from a config, the refusals, the plans, strict loading, the
opt-in drop-in swap, and the golden's generator (where `transformers` imports)."""
import ctypes
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_clip_vision_golden', os.path.join(HERE, 'golden', 'make_clip_vision_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _engine(lib, case='A', **kw):
    from mvedit_amd.vision_encoder import CLIPVisionEngine
    return CLIPVisionEngine(SimpleNamespace(**G.config_dict(case)), device='cpu', with_projection=G.CASES[case]['with_projection'], **kw)


def test_engine_from_a_config_object_plans_the_issue_op_list(lib):
    eng = _engine(lib, 'B')
    assert eng.dtype == torch.float16 and eng.device == torch.device('cpu') and eng.projection_dim == 96 and eng.num_tokens == 257
    # the attribute names the reference reads (ip_adapter.py:67, :79; zero123.py:247)
    assert eng.config.projection_dim == 96 and eng.config.hidden_size == 160 and eng.config.image_size == 224
    assert next(eng.parameters()).dtype == torch.float16 and eng.eval() is eng and eng.requires_grad_(False) is eng
    assert eng.to('cpu') is eng and eng.to(torch.float16) is eng and eng.to('cpu', dtype=torch.float16) is eng
    with pytest.raises(NotImplementedError):
        eng.to(torch.float32)
    with pytest.raises(NotImplementedError):
        eng.to('cuda')
    info = eng.plan(2)
    labels = [lab for _, _, lab in eng.op_table()]
    layer = ['layernorm', 'self_attn.qkv', 'attention', 'self_attn.out_proj+residual', 'layernorm', 'mlp.fc1', 'gelu', 'mlp.fc2+residual', 'hidden state -> output']
    assert labels == ['patchify', 'patch_embedding', 'class + position embedding', 'layernorm', 'hidden state -> output'] + layer * 3 + \
        ['last_hidden_state -> output', 'layernorm', 'visual_projection']
    assert info['n_ops'] == len(labels) and info['workspace_bytes'] > 0
    B, T, C, I = 2, 257, 160, 640
    M = B * T
    assert info['flops']['linear'] == 2.0 * (B * 256) * C * 592 + 3 * 2.0 * M * (3 * C * C + C * C + 2 * C * I) + 2.0 * B * 96 * C
    assert info['flops']['attention'] == 3 * 4.0 * B * 2 * T * T * 80
    plain = _engine(lib, 'C', dtype=torch.bfloat16)
    assert plain.dtype == torch.bfloat16 and plain.projection_dim == 0
    plain.plan(1)
    labels = [lab for _, _, lab in plain.op_table()]
    assert labels[-1] == 'layernorm' and 'quick_gelu' in labels and 'visual_projection' not in labels
    # a dict works like an object, and unsupported geometry is refused at create
    from mvedit_amd.vision_encoder import CLIPVisionEngine
    assert CLIPVisionEngine(G.config_dict('A'), device='cpu').config.image_size == 112
    for bad, match in ((dict(hidden_size=208), 'head_dim must be 64 or 80'),                       # OpenCLIP bigG's head_dim 104
                       (dict(hidden_size=96), 'head_dim'),
                       (dict(hidden_size=4096, num_attention_heads=64), '2048'),
                       (dict(image_size=100), 'multiple of patch_size'),
                       (dict(intermediate_size=100), 'intermediate_size'),
                       (dict(projection_dim=12), 'projection_dim')):
        with pytest.raises(lib.MveError, match=match):
            CLIPVisionEngine(dict(G.config_dict('A'), **bad), device='cpu')
    with pytest.raises(NotImplementedError, match='hidden_act'):
        CLIPVisionEngine(dict(G.config_dict('A'), hidden_act='relu'), device='cpu')
    with pytest.raises(ValueError, match='patch_size'):
        CLIPVisionEngine({k: v for k, v in G.config_dict('A').items() if k != 'patch_size'}, device='cpu')


def test_refusals_come_before_any_launch(lib):
    eng = _engine(lib)
    px = torch.zeros(2, 3, 112, 112)
    with pytest.raises(NotImplementedError, match='output_attentions'):
        eng(px, output_attentions=True)
    with pytest.raises(NotImplementedError, match='interpolate_pos_encoding'):
        eng(px, interpolate_pos_encoding=True)
    for bad in (torch.zeros(2, 3, 224, 224), torch.zeros(2, 1, 112, 112), torch.zeros(3, 112, 112), torch.zeros(0, 3, 112, 112), torch.zeros(2, 3, 112, 98)):
        with pytest.raises(ValueError, match=r'\[B, 3, 112, 112\]'):
            eng(bad)
    with pytest.raises(ValueError, match='floating'):
        eng(torch.zeros(2, 3, 112, 112, dtype=torch.uint8))
    with pytest.raises(ValueError, match='pixel_values'):
        eng(None)


def test_strict_load_names_the_first_missing_parameter(lib):
    eng = _engine(lib, 'B')
    names = eng.expected_parameters()
    assert names[0] == 'vision_model.embeddings.class_embedding' and names[-1] == 'visual_projection.weight' and 'vision_model.pre_layrnorm.weight' in names
    assert sorted(names) == sorted(G.make_weights('B'))
    assert 'visual_projection.weight' not in _engine(lib, 'C').expected_parameters()
    sd = {k: torch.zeros(1) for k in names if k != 'vision_model.encoder.layers.1.mlp.fc1.bias'}
    with pytest.raises(KeyError, match=r'vision_model\.encoder\.layers\.1\.mlp\.fc1\.bias'):
        eng.load_state_dict(sd)
    bare = {k[len('vision_model.'):] if k.startswith('vision_model.') else k: v for k, v in sd.items()}      # without the `vision_model.` level
    with pytest.raises(KeyError, match=r'vision_model\.encoder\.layers\.1\.mlp\.fc1\.bias'):
        eng.load_state_dict(bare)


def test_expected_parameters_are_the_transformers_state_dict(lib):
    transformers = pytest.importorskip('transformers')
    from mvedit_amd.vision_encoder import CLIPVisionEngine
    for case in ('A', 'C'):
        m = G.build_module(case, torch.float16)
        eng = CLIPVisionEngine.from_module(m)
        assert eng.with_projection == G.CASES[case]['with_projection'] and eng.dtype == torch.float16 and eng.device.type == 'cpu'
        assert eng.config is m.config and eng.cfg['hidden_act'] == G.CASES[case]['hidden_act'] and eng.cfg['patch_size'] == G.CASES[case]['patch_size']
        keys = [k for k in m.state_dict() if not k.endswith('position_ids')]
        with_level = {(k if k.startswith(('vision_model.', 'visual_projection.')) else 'vision_model.' + k) for k in keys}
        assert set(eng.expected_parameters()) == with_level
        without = {k[len('vision_model.'):] if k.startswith('vision_model.') else k for k in eng.expected_parameters()}
        assert without == {k[len('vision_model.'):] if k.startswith('vision_model.') else k for k in keys}
    cfg = transformers.CLIPVisionConfig(**G.config_dict('B'))
    assert CLIPVisionEngine(cfg, device='cpu').num_tokens == 257


def test_resampler_and_image_proj_surface(lib):
    from mvedit_amd.ip_adapter import ImageProjEngine, ResamplerEngine
    r = ResamplerEngine(device='cpu', **G.RESAMPLER)
    assert sorted(r.expected_parameters()) == sorted(G.make_resampler_weights())
    info = r.plan(1, 257)
    labels = [lab for _, _, lab in r.op_table()]
    layer = ['layernorm', 'layernorm', 'to_q', 'to_kv (image rows)', 'to_kv (latent rows)', 'perceiver attention', 'to_out+residual', 'layernorm', 'ff.1', 'gelu',
             'ff.3+residual']
    assert labels == ['proj_in', 'latents.repeat'] + layer * 2 + ['proj_out', 'layernorm'] and info['n_ops'] == len(labels)
    D, inner, F, E, O, Q, n1 = 128, 128, 512, 160, 192, 16, 257
    assert info['flops']['linear'] == 2.0 * n1 * D * E + 2 * 2.0 * (Q * inner * D + (n1 + Q) * 2 * inner * D + Q * D * inner + 2 * Q * F * D) + 2.0 * Q * O * D
    assert info['flops']['attention'] == 2 * 4.0 * 2 * Q * (n1 + Q) * 64
    assert next(r.parameters()).dtype == torch.float16 and r.eval() is r and r.requires_grad_(False) is r and r.to('cpu') is r
    with pytest.raises(NotImplementedError, match='dim_head'):
        ResamplerEngine(device='cpu', **dict(G.RESAMPLER, dim_head=80))
    with pytest.raises(lib.MveError, match='embedding_dim'):
        ResamplerEngine(device='cpu', **dict(G.RESAMPLER, embedding_dim=100))
    with pytest.raises(lib.MveError, match='output_dim'):
        ResamplerEngine(device='cpu', **dict(G.RESAMPLER, output_dim=4096))
    with pytest.raises(ValueError, match='embedding_dim'):
        r(torch.zeros(1, 257, 128))
    with pytest.raises(KeyError, match=r'layers\.1\.0\.to_kv\.weight'):
        r.load_state_dict({k: torch.zeros(1) for k in r.expected_parameters() if k != 'layers.1.0.to_kv.weight'})
    with pytest.raises(KeyError, match='not a parameter'):
        r.load_state_dict(dict({k: torch.zeros(1) for k in r.expected_parameters()}, extra=torch.zeros(1)))
    p = ImageProjEngine(device='cpu', **G.IMAGE_PROJ)
    assert p.expected_parameters() == ['proj.weight', 'proj.bias', 'norm.weight', 'norm.bias'] and next(p.parameters()).device.type == 'cpu'
    with pytest.raises(KeyError, match='not loaded'):
        p(torch.zeros(3, 64))
    with pytest.raises(KeyError, match='norm.bias'):
        p.load_state_dict({k: torch.zeros(1) for k in ('proj.weight', 'proj.bias', 'norm.weight')})
    with pytest.raises(ValueError, match='proj.weight'):
        p.load_state_dict({k: torch.zeros(1) for k in p.expected_parameters()})
    with pytest.raises(NotImplementedError):
        ImageProjEngine(device='cpu', cross_attention_dim=100)


class _Tower(torch.nn.Module):
    """stand-in with the two things the maker reads: `.config` and a state dict under transformers' names"""

    def __init__(self, case, device='cpu'):
        super().__init__()
        self.config = SimpleNamespace(**G.config_dict(case))
        self.w = torch.nn.Parameter(torch.zeros(1, dtype=torch.float16, device=device))
        if G.CASES[case]['with_projection']:
            self.visual_projection = torch.nn.Linear(2, 2, bias=False)


class Resampler(torch.nn.Module):
    """stand-in recognised by class name, with the attributes ResamplerEngine.from_module reads"""

    def __init__(self):
        super().__init__()
        r = G.RESAMPLER
        self.latents = torch.nn.Parameter(torch.zeros(1, r['num_queries'], r['dim'], dtype=torch.float16))
        self.proj_in, self.proj_out = torch.nn.Linear(r['embedding_dim'], r['dim']), torch.nn.Linear(r['dim'], r['output_dim'])
        attn = torch.nn.Module()
        attn.dim_head, attn.heads = r['dim_head'], r['heads']
        ff = torch.nn.Sequential(torch.nn.LayerNorm(r['dim']), torch.nn.Linear(r['dim'], r['dim'] * r['ff_mult'], bias=False))
        self.layers = torch.nn.ModuleList([torch.nn.ModuleList([attn, ff]) for _ in range(r['depth'])])


class ImageProjModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        p = G.IMAGE_PROJ
        self.cross_attention_dim, self.clip_extra_context_tokens = p['cross_attention_dim'], p['clip_extra_context_tokens']
        self.proj = torch.nn.Linear(p['clip_embeddings_dim'], p['clip_extra_context_tokens'] * p['cross_attention_dim'])
        self.norm = torch.nn.LayerNorm(p['cross_attention_dim'])


class SomethingElse(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_swap_image_encoder_is_opt_in_and_idempotent(lib, monkeypatch):
    from mvedit_amd import dropin
    from mvedit_amd.ip_adapter import ImageProjEngine, ResamplerEngine
    from mvedit_amd.vision_encoder import CLIPVisionEngine
    for name in ('image_encoder', 'vision_encoder', 'image_proj_model'):
        assert name not in dropin.SWAPPED_ATTRS and name not in dropin.MAKERS
    enc, plus, plain_proj, other = _Tower('B'), Resampler(), ImageProjModel(), SomethingElse()
    ip_plus = SimpleNamespace(image_encoder=enc, image_proj_model=plus, pipe=None)                  # shaped like IPAdapter
    z123p = SimpleNamespace(vision_encoder=_Tower('A'), unet=None, vae=None)                        # Zero123PlusPipeline
    z123 = SimpleNamespace(image_encoder=_Tower('A'), unet=None, vae=None)                          # Zero123Pipeline
    before = (ip_plus.image_encoder, ip_plus.image_proj_model, z123p.vision_encoder, z123.image_encoder)
    for obj in (ip_plus, z123p, z123):
        dropin.swap_engines(obj)
    assert before == (ip_plus.image_encoder, ip_plus.image_proj_model, z123p.vision_encoder, z123.image_encoder)      # the default swap leaves them alone
    dropin.install()
    try:
        assert before == (ip_plus.image_encoder, ip_plus.image_proj_model, z123p.vision_encoder, z123.image_encoder)  # and so does install()
    finally:
        dropin.uninstall()
    with pytest.raises(RuntimeError, match='CPU'):                                                  # the makers' on-accelerator check
        dropin.swap_image_encoder(ip_plus)
    assert ip_plus.image_encoder is enc
    with pytest.raises(TypeError, match='SomethingElse'):
        dropin.make_image_proj(other)
    # on an accelerator the makers build from the module; here the construction is observed and the packing (which needs the device) is not run
    made = []

    def fake(cls):
        real = cls.from_module.__func__

        def from_module(m, dtype=None, device=None):
            eng = real(cls, m, dtype=dtype, device='cpu')
            made.append((m, eng))
            return eng
        return staticmethod(from_module)
    monkeypatch.setattr(dropin, '_module_dtype_device', lambda m: (torch.float16, torch.device('cuda', 0)))
    for cls in (CLIPVisionEngine, ResamplerEngine, ImageProjEngine):
        monkeypatch.setattr(cls, 'from_module', fake(cls))
    dropin.swap_image_encoder(ip_plus)
    assert [m for m, _ in made] == [enc, plus]
    e_enc, e_proj = ip_plus.image_encoder, ip_plus.image_proj_model
    assert isinstance(e_enc, CLIPVisionEngine) and e_enc.with_projection and e_enc.config.hidden_size == 160
    assert isinstance(e_proj, ResamplerEngine) and (e_proj.dim, e_proj.depth, e_proj.heads, e_proj.num_queries, e_proj.embedding_dim, e_proj.output_dim,
                                                    e_proj.ff_mult) == (128, 2, 2, 16, 160, 192, 4)
    dropin.swap_image_encoder(ip_plus)                                                              # idempotent: engines stay, nothing is rebuilt
    assert ip_plus.image_encoder is e_enc and ip_plus.image_proj_model is e_proj and len(made) == 2
    again = SimpleNamespace(image_encoder=enc, image_proj_model=other)                              # a second object over the same module shares the engine,
    dropin.swap_image_encoder(again)                                                                # and an unknown image_proj_model class is left alone
    assert again.image_encoder is e_enc and again.image_proj_model is other and len(made) == 2
    with torch.no_grad():                                                                           # a changed parameter rebuilds
        enc.w.add_(1)
    third = dropin.swap_image_encoder(SimpleNamespace(image_encoder=enc))
    assert third.image_encoder is not e_enc and len(made) == 3
    dropin.swap_image_encoder(z123p)
    dropin.swap_image_encoder(z123)
    assert isinstance(z123p.vision_encoder, CLIPVisionEngine) and isinstance(z123.image_encoder, CLIPVisionEngine) and len(made) == 5
    base = dropin.swap_image_encoder(SimpleNamespace(image_encoder=None, image_proj_model=plain_proj))
    assert base.image_encoder is None and isinstance(base.image_proj_model, ImageProjEngine) and base.image_proj_model.clip_extra_context_tokens == 4


def test_golden_regenerates(lib):
    pytest.importorskip('transformers')
    head, hidden = G.generate('A')
    ref, href = np.load(G.REF), np.load(G.HIDDEN_REF)
    for case in G.CASES:
        assert str(ref[f'{case}.weights_sha256']) == G.digest(G.make_weights(case)), case
        assert str(ref[f'{case}.pixels_sha256']) == G.digest({'pixel_values': G.make_pixels(case)}), case
    assert str(ref['R.weights_sha256']) == G.digest(G.make_resampler_weights()) and str(ref['P.weights_sha256']) == G.digest(G.make_image_proj_weights())
    for k, v in head.items():
        if v.dtype.kind in 'iU':
            assert np.array_equal(ref[k], v), k
        elif k.split('.')[1].startswith('err_'):
            np.testing.assert_allclose(ref[k], v, rtol=0.05, err_msg=k)             # 16-bit CPU kernels: the summation order may differ between hosts
        else:
            np.testing.assert_allclose(ref[k], v, rtol=1e-6, atol=1e-6, err_msg=k)  # float64 stored as float32
    for k, v in hidden.items():
        np.testing.assert_allclose(href[k], v, rtol=1e-6, atol=1e-6, err_msg=k)
    assert os.path.getsize(G.REF) < (1 << 20) and os.path.getsize(G.HIDDEN_REF) < (1 << 20)
    assert ref['R.tokens'].shape == (1, 16, 192) and ref['P.tokens'].shape == (3, 4, 192)


def test_c_abi_argument_errors_name_the_argument(lib):
    """host logic only: each call fails its checks before the device is touched (the pointers are host addresses that are never read)"""
    buf = torch.zeros(4096)
    p, f = ctypes.c_void_p(buf.data_ptr()), ctypes.c_float
    odd = ctypes.c_void_p(p.value + 2)

    def bad(name, *args, match):
        with pytest.raises(lib.MveError, match=match):
            lib.call(name, *args)
    bad('mve_clip_patchify', 0, p, 1, 56, 56, 14, p, 592, None, match='dtype')
    bad('mve_clip_patchify', 1, None, 1, 56, 56, 14, p, 592, None, match='null')
    bad('mve_clip_patchify', 1, p, 1, 56, 42, 14, p, 592, None, match='W 42')
    bad('mve_clip_patchify', 1, p, 1, 50, 50, 14, p, 592, None, match='H 50')
    bad('mve_clip_patchify', 1, p, 1, 56, 56, 14, p, 588, None, match='ld 588')
    bad('mve_clip_patchify', 1, odd, 1, 56, 56, 14, p, 592, None, match='aligned')
    bad('mve_clip_vision_embed', 0, p, p, p, p, 1, 16, 64, None, match='dtype')
    bad('mve_clip_vision_embed', 1, p, None, p, p, 1, 16, 64, None, match='null')
    bad('mve_clip_vision_embed', 1, p, p, p, p, 1, 16, 60, None, match=' C 60 ')
    bad('mve_clip_vision_embed', 1, p, p, odd, p, 1, 16, 64, None, match='aligned')
    h = ctypes.c_void_p()
    bad('mve_clip_vision_create', ctypes.byref(h), 1, 224, 14, 1664, 2, 16, 8192, 1, f(1e-5), 0, match='head_dim must be 64 or 80')
    bad('mve_clip_vision_create', ctypes.byref(h), 1, 224, 14, 128, 2, 2, 512, 3, f(1e-5), 0, match='act')
    bad('mve_ip_resampler_create', ctypes.byref(h), 1, 100, 2, 2, 16, 160, 192, 4, match='dim 100')
    assert not h.value
    eng, text = _engine(lib, 'B'), ctypes.c_void_p()
    lib.call('mve_clip_text_create', ctypes.byref(text), 1, 512, 77, 128, 2, 2, 512, 0, f(1e-5), 0)
    try:
        bad('mve_clip_vision_forward', text, p, 1, p, p, None, None, p, 1 << 20, None, None, match='not a CLIP vision tower')
        bad('mve_clip_vision_plan', text, 1, None, None, None, match='not a CLIP vision tower')
        bad('mve_ip_resampler_plan', eng._h, 1, 257, None, None, None, match='not a Resampler')
        bad('mve_clip_text_plan', eng._h, 1, 7, None, None, None, match='not a CLIP text tower')
        bad('mve_unet_forward', eng._h, 0, p, 1, p, p, 1, 8, 8, 77, 1, None, None, 0, p, p, 1 << 20, None, None, match='CLIP')
        bad('mve_clip_vision_forward', eng._h, p, 1, p, p, p, None, p, 1 << 20, None, None, match='vision_model.embeddings.class_embedding')
    finally:
        lib.call('mve_unet_destroy', text)
