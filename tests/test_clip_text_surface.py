"""CLIPTextEngine without a GPU: construction from a config, the refusals, the ModelOutput-style result, strict loading, the opt-in drop-in
swap, and the golden's generator (where `transformers` imports)."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_clip_text_golden', os.path.join(HERE, 'golden', 'make_clip_text_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _engine(lib, case='A', **kw):
    from mvedit_amd.text_encoder import CLIPTextEngine
    return CLIPTextEngine(SimpleNamespace(**G.config_dict(case)), device='cpu', with_projection=G.CASES[case]['with_projection'], **kw)


def test_engine_from_a_config_object_plans_the_issue_op_list(lib):
    eng = _engine(lib, 'B')
    assert eng.dtype == torch.float16 and eng.device == torch.device('cpu') and eng.config.hidden_size == 128 and eng.projection_dim == 64
    assert next(eng.parameters()).dtype == torch.float16 and eng.eval() is eng and eng.to('cpu') is eng and eng.to(torch.float16) is eng
    with pytest.raises(NotImplementedError):
        eng.to(torch.float32)
    with pytest.raises(NotImplementedError):
        eng.to('cuda')
    info = eng.plan(2, 77)
    labels = [lab for _, _, lab in eng.op_table()]
    layer = ['layernorm', 'self_attn.qkv', 'causal attention', 'self_attn.out_proj+residual', 'layernorm', 'mlp.fc1', 'gelu', 'mlp.fc2+residual', 'hidden state -> output']
    assert labels == ['token + position embedding', 'hidden state -> output'] + layer * 3 + ['layernorm', 'end-of-text pooling', 'text_projection']
    assert info['n_ops'] == len(labels) and info['workspace_bytes'] > 0
    M, C, I = 2 * 77, 128, 512
    assert info['flops']['linear'] == 3 * 2.0 * M * (3 * C * C + C * C + 2 * C * I) + 2.0 * 2 * 64 * C
    plain = _engine(lib, 'A', dtype=torch.bfloat16)
    assert plain.dtype == torch.bfloat16 and [lab for _, _, lab in (plain.plan(1, 5), plain.op_table())[1]][-1] == 'end-of-text pooling'
    assert 'quick_gelu' in [lab for _, _, lab in plain.op_table()]
    # a dict works like an object, and unsupported geometry is refused at create
    from mvedit_amd.text_encoder import CLIPTextEngine
    assert CLIPTextEngine(G.config_dict('A'), device='cpu').config.vocab_size == 512
    for bad in (dict(hidden_size=96), dict(num_attention_heads=4), dict(hidden_size=4096, num_attention_heads=64), dict(intermediate_size=100)):
        with pytest.raises(lib.MveError):
            CLIPTextEngine(dict(G.config_dict('A'), **bad), device='cpu')
    with pytest.raises(NotImplementedError, match='hidden_act'):
        CLIPTextEngine(dict(G.config_dict('A'), hidden_act='relu'), device='cpu')
    with pytest.raises(lib.MveError, match='128'):
        CLIPTextEngine(dict(G.config_dict('A'), max_position_embeddings=256), device='cpu').plan(1, 129)


def test_refusals_come_before_any_launch(lib):
    eng = _engine(lib)
    ids = torch.zeros(2, 7, dtype=torch.long)
    with pytest.raises(NotImplementedError, match='attention_mask'):
        eng(ids, attention_mask=torch.tensor([[1] * 5 + [0] * 2] * 2))
    with pytest.raises(NotImplementedError, match='position_ids'):
        eng(ids, position_ids=torch.arange(7)[None])
    with pytest.raises(NotImplementedError, match='inputs_embeds'):
        eng(None, inputs_embeds=torch.zeros(2, 7, 128))
    with pytest.raises(NotImplementedError, match='output_attentions'):
        eng(ids, output_attentions=True)
    for bad in (-1, 512):
        with pytest.raises(ValueError, match='vocab_size'):
            eng(torch.tensor([[1, bad, 3]]))
    with pytest.raises(ValueError, match='max_position_embeddings'):
        eng(torch.zeros(1, 78, dtype=torch.long))
    with pytest.raises(ValueError, match='input_ids'):
        eng(None)


def test_result_indexes_like_a_model_output():
    from mvedit_amd.text_encoder import CLIPTextOutput
    last, pooled, embeds, hs = torch.zeros(1, 3, 4), torch.ones(1, 4), torch.full((1, 2), 2.0), (torch.zeros(1), torch.ones(1), torch.full((1,), 2.0))
    plain = CLIPTextOutput([('last_hidden_state', last), ('pooler_output', pooled), ('hidden_states', hs)])
    assert plain[0] is last and plain[1] is pooled and plain[2] is hs and plain[-1][-2] is hs[1] and len(plain) == 3
    assert plain.last_hidden_state is last and plain.pooler_output is pooled and plain['pooler_output'] is pooled and plain.attentions is None
    assert plain.keys() == ['last_hidden_state', 'pooler_output', 'hidden_states'] and tuple(plain) == plain.to_tuple() == (last, pooled, hs)
    short = CLIPTextOutput([('last_hidden_state', last), ('pooler_output', pooled), ('hidden_states', None)])       # None fields are skipped
    assert len(short) == 2 and short[-1] is pooled and short.hidden_states is None
    with pytest.raises(KeyError):
        short['hidden_states']
    proj = CLIPTextOutput([('text_embeds', embeds), ('last_hidden_state', last), ('hidden_states', hs)])
    assert proj[0] is embeds and proj[1] is last and proj[-1][-2] is hs[1] and proj.text_embeds is embeds and not hasattr(proj, 'pooler_output')


def test_strict_load_names_the_first_missing_parameter(lib):
    eng = _engine(lib, 'B')
    names = eng.expected_parameters()
    assert names[0] == 'text_model.embeddings.token_embedding.weight' and names[-1] == 'text_projection.weight'
    assert sorted(names) == sorted(G.make_weights('B'))
    sd = {k: torch.zeros(1) for k in names if k != 'text_model.encoder.layers.1.mlp.fc1.bias'}
    with pytest.raises(KeyError, match=r'text_model\.encoder\.layers\.1\.mlp\.fc1\.bias'):
        eng.load_state_dict(sd)
    # CLIPTextModel's own state dict lost the `text_model.` level in transformers 5: both spellings name the same parameters
    bare = {k[len('text_model.'):] if k.startswith('text_model.') else k: v for k, v in sd.items()}
    with pytest.raises(KeyError, match=r'text_model\.encoder\.layers\.1\.mlp\.fc1\.bias'):
        eng.load_state_dict(bare)
    with pytest.raises(KeyError, match='final_layer_norm'):
        eng.text_model.final_layer_norm(torch.zeros(1, 3, 128))


class _Tower(torch.nn.Module):
    """stand-in with the two things the maker reads: `.config` and a state dict under transformers' names"""

    def __init__(self, case, device):
        super().__init__()
        self.config = SimpleNamespace(**G.config_dict(case))
        self.w = torch.nn.Parameter(torch.zeros(1, dtype=torch.float16, device=device))
        if G.CASES[case]['with_projection']:
            self.text_projection = torch.nn.Linear(2, 2, bias=False)


def test_swap_text_encoder_is_opt_in_and_idempotent(lib, monkeypatch):
    from mvedit_amd import dropin
    from mvedit_amd.text_encoder import CLIPTextEngine
    assert 'text_encoder' not in dropin.SWAPPED_ATTRS and 'text_encoder' not in dropin.MAKERS
    te, te2 = _Tower('A', 'cpu'), _Tower('B', 'cpu')
    pipe = SimpleNamespace(text_encoder=te, text_encoder_2=te2, unet=None)
    dropin.swap_engines(pipe)
    assert pipe.text_encoder is te and pipe.text_encoder_2 is te2                     # the default swap leaves the towers alone
    with pytest.raises(RuntimeError, match='CPU'):                                    # the makers' on-accelerator check
        dropin.swap_text_encoder(pipe)
    assert pipe.text_encoder is te
    # on an accelerator the maker builds from the module; here the construction is observed and the packing (which needs the device) is not run
    made = []

    def fake_from_module(m, dtype=None, device=None):
        eng = CLIPTextEngine(m.config, dtype=dtype, device='cpu', with_projection=hasattr(m, 'text_projection'))
        made.append((m, eng))
        return eng
    monkeypatch.setattr(dropin, '_module_dtype_device', lambda m: (torch.float16, torch.device('cuda', 0)))
    monkeypatch.setattr(CLIPTextEngine, 'from_module', staticmethod(fake_from_module))
    dropin.swap_text_encoder(pipe)
    assert [m for m, _ in made] == [te, te2]
    e1, e2 = pipe.text_encoder, pipe.text_encoder_2
    assert e1 is made[0][1] and e2 is made[1][1] and not e1.with_projection and e2.with_projection and e2.projection_dim == 64
    dropin.swap_text_encoder(pipe)                                                    # idempotent: engines stay, nothing is rebuilt
    assert pipe.text_encoder is e1 and pipe.text_encoder_2 is e2 and len(made) == 2
    again = SimpleNamespace(text_encoder=te)                                          # a second pipeline over the same module shares the engine
    assert dropin.swap_text_encoder(again).text_encoder is e1 and len(made) == 2
    assert dropin.swap_text_encoder(SimpleNamespace(text_encoder=None)).text_encoder is None


def test_from_module_reads_a_transformers_module(lib):
    transformers = pytest.importorskip('transformers')
    from mvedit_amd.text_encoder import CLIPTextEngine
    for case in ('A', 'B'):
        m = G.build_module(case, torch.float16)
        eng = CLIPTextEngine.from_module(m)
        assert eng.with_projection == G.CASES[case]['with_projection'] and eng.dtype == torch.float16 and eng.device.type == 'cpu'
        assert eng.config is m.config and eng.cfg['eos_token_id'] == G.CASES[case]['eos_token_id'] and eng.cfg['hidden_act'] == G.CASES[case]['hidden_act']
        own = {(k if k.startswith(('text_model.', 'text_projection.')) else 'text_model.' + k) for k in m.state_dict()}
        assert set(eng.expected_parameters()) <= own
    assert isinstance(m, transformers.CLIPTextModelWithProjection)


def test_golden_regenerates(lib):
    pytest.importorskip('transformers')
    head, hidden = G.generate('A')
    ref, href = np.load(G.REF), np.load(G.HIDDEN_REF)
    assert str(ref['A.weights_sha256']) == G.weights_digest(G.make_weights('A')) and str(ref['B.weights_sha256']) == G.weights_digest(G.make_weights('B'))
    for k, v in head.items():
        if v.dtype.kind in 'iU':
            assert np.array_equal(ref[k], v), k
        elif k.split('.')[2].startswith('err_'):
            np.testing.assert_allclose(ref[k], v, rtol=0.05, err_msg=k)             # 16-bit CPU kernels: the summation order may differ between hosts
        else:
            np.testing.assert_allclose(ref[k], v, rtol=1e-9, atol=1e-9, err_msg=k)  # float64
    for k, v in hidden.items():
        np.testing.assert_allclose(href[k], v, rtol=1e-9, atol=1e-9, err_msg=k)
    assert os.path.getsize(G.REF) < (1 << 20) and os.path.getsize(G.HIDDEN_REF) < (1 << 20)


def test_c_abi_argument_errors_name_the_argument(lib):
    """host logic only: each call fails its checks before the device is touched (the pointers are host addresses that are never read)"""
    import ctypes
    buf = torch.zeros(4096)
    p, f = ctypes.c_void_p(buf.data_ptr()), ctypes.c_float

    def bad(name, *args, match):
        with pytest.raises(lib.MveError, match=match):
            lib.call(name, *args)
    for L, hd, match in ((0, 64, r' L 0 '), (129, 64, r' L 129 '), (16, 40, 'head_dim 40')):
        bad('mve_attention_causal', 1, p, 192, p, 192, p, 192, p, 64, 1, L, 1, hd, f(0.125), None, match=match)
    bad('mve_attention_causal', 0, p, 192, p, 192, p, 192, p, 64, 1, 16, 1, 64, f(0.125), None, match='dtype')
    bad('mve_attention_causal', 1, p, 100, p, 192, p, 192, p, 64, 1, 16, 1, 64, f(0.125), None, match='ldq')
    bad('mve_attention_causal', 1, p, 192, p, 192, p, 64, p, 64, 1, 16, 2, 64, f(0.125), None, match='ldv')
    bad('mve_attention_causal', 1, p, 192, None, 192, p, 192, p, 64, 1, 16, 1, 64, f(0.125), None, match='null')
    bad('mve_attention_causal', 1, p, 192, ctypes.c_void_p(p.value + 2), 192, p, 192, p, 64, 1, 16, 1, 64, f(0.125), None, match='aligned')
    bad('mve_clip_embed', 1, p, p, p, p, 1, 78, 64, 100, 77, None, match='max_pos')
    bad('mve_clip_embed', 1, p, p, p, p, 1, 7, 60, 100, 77, None, match=' C 60 ')
    bad('mve_clip_embed', 1, None, p, p, p, 1, 7, 64, 100, 77, None, match='null')
    bad('mve_act', 1, 2, p, p, 16, None, match='kind')
    bad('mve_act', 0, 0, p, p, 16, None, match='dtype')
    bad('mve_clip_pool', 1, p, None, p, 1, 7, 64, 2, None, match='null')
    bad('mve_clip_pool', 1, p, p, p, 1, 0, 64, 2, None, match=' L 0')
    h = ctypes.c_void_p()
    bad('mve_clip_text_create', ctypes.byref(h), 1, 512, 77, 128, 2, 2, 512, 3, f(1e-5), 0, match='act')
    bad('mve_clip_text_create', ctypes.byref(h), 1, 512, 77, 128, 2, 2, 512, 0, f(1e-5), 12, match='projection_dim')
    assert not h.value
    eng, vae = _engine(lib, 'B'), ctypes.c_void_p()
    lib.call('mve_vae_create', ctypes.byref(vae), 1, 1, 4, 3, 2, (ctypes.c_int * 2)(64, 128), 1, 32, f(1e-6))
    try:
        bad('mve_clip_text_forward', vae, p, 1, 7, 2, p, p, None, None, p, 1 << 20, None, None, match='not a CLIP text tower')
        bad('mve_clip_text_plan', vae, 1, 7, None, None, None, match='not a CLIP text tower')
        bad('mve_vae_plan', eng._h, 1, 8, 8, 1, None, None, None, match='not a VAE')
        bad('mve_unet_forward', eng._h, 0, p, 1, p, p, 1, 8, 8, 77, 1, None, None, 0, p, p, 1 << 20, None, None, match='CLIP')
        bad('mve_clip_text_forward', eng._h, p, 1, 7, 300, p, p, p, None, p, 1 << 20, None, None, match='text_model.embeddings.token_embedding.weight')
    finally:
        lib.call('mve_unet_destroy', vae)
