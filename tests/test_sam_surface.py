"""SamImageEncoderEngine without a GPU: the numpy rule (tests/sam_rule.py) against transformers' SamVisionEncoder through the golden, the key
mapping of both state-dict layouts, the refusals (all before any launch), the ViT-H plan, the C-ABI argument errors and the opt-in drop-in."""
import ctypes
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_sam_encoder_golden', os.path.join(HERE, 'golden', 'make_sam_encoder_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
sys.path.insert(0, HERE)
import sam_rule as R  # noqa: E402


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize('case', ['A', 'B'])
def test_numpy_rule_is_transformers_sam_vision_encoder(case):
    """The rule, run from the regenerated weights and pixels, reproduces every hidden state and the neck output the golden stores from transformers'
    float64 module -- to the float32 the golden is stored in.  Block 0 is windowed (three of the four windows mostly padding), the last-but-one
    (A) / last (B) block is global: partition, padding tokens as keys, both bias terms, un-partition and the neck are all in that comparison.
    With the two tables of block 0 zeroed the rule moves hidden state 1 by percents: the comparison sees the bias."""
    ref = np.load(G.REF)
    sd, cfg, px = G.make_weights(case), G.config_dict(case), G.make_pixels(case)
    assert str(ref[f'{case}.weights_sha256']) == G.digest(sd) and str(ref[f'{case}.pixels_sha256']) == G.digest({'pixel_values': px})
    hs, neck = R.encoder_forward(sd, cfg, px)
    assert len(hs) == cfg['num_hidden_layers'] + 1
    for name, t in zip(G.tensor_names(case), hs + [neck]):
        assert tuple(ref[f'{case}.{name}.shape']) == t.shape, name
        got = t.reshape(-1)[G.sample_index(case, name, t.size)]
        assert rel_l2(got, ref[f'{case}.{name}']) < 1e-6, name
    keep = {}
    one = R.block_forward({k: np.asarray(v, np.float64) for k, v in sd.items()}, cfg, 0, hs[0], keep)
    assert np.array_equal(one, hs[1]) and keep['grid'] == 14 and keep['q'].shape == (4 * G.CASES[case]['B'], 196, 2, cfg['hidden_size'] // 2)
    flat = dict(sd)
    flat['layers.0.attn.rel_pos_h'] = np.zeros_like(sd['layers.0.attn.rel_pos_h'])
    flat['layers.0.attn.rel_pos_w'] = np.zeros_like(sd['layers.0.attn.rel_pos_w'])
    assert rel_l2(R.block_forward({k: np.asarray(v, np.float64) for k, v in flat.items()}, cfg, 0, hs[0]), hs[1]) > 1e-2
    assert float(ref[f'{case}.neck_change_without_tables']) > 1e-2 and float(ref[f'{case}.max_softmax_probability']) > 0.2


def test_rule_partition_pads_with_zeros_and_inverts():
    x = np.random.RandomState(0).standard_normal((2, 16, 16, 8))
    win = R.window_partition(x, 14)
    assert win.shape == (2 * 4, 196, 8)
    w0 = win.reshape(2, 2, 2, 14, 14, 8)
    assert np.array_equal(w0[:, 0, 0], x[:, :14, :14]) and np.array_equal(w0[:, 0, 1, :, :2], x[:, :14, 14:]) and not w0[:, 0, 1, :, 2:].any()
    assert not w0[:, 1, 1, 2:].any() and np.array_equal(w0[:, 1, 1, :2, :2], x[:, 14:, 14:])
    assert np.array_equal(R.window_unpartition(win, 2, 16, 14), x)
    assert np.array_equal(R.window_unpartition(R.window_partition(x[:, :14, :14], 14), 2, 14, 14), x[:, :14, :14])


def test_golden_regenerates():
    pytest.importorskip('transformers')
    out = G.generate('A')
    ref = np.load(G.REF)
    for k, v in out.items():
        if v.dtype.kind in 'iU':
            assert np.array_equal(ref[k], v), k
        elif '.err_' in k or k.endswith('neck_change_without_tables'):
            np.testing.assert_allclose(ref[k], v, rtol=0.05, err_msg=k)             # 16-bit CPU kernels: the summation order may differ between hosts
        else:
            np.testing.assert_allclose(ref[k], v, rtol=1e-6, atol=1e-6, err_msg=k)  # float64 stored as float32
    assert os.path.getsize(G.REF) < (1 << 20)


def test_both_key_layouts_map_onto_the_engine_names_once(lib):
    from mvedit_amd.sam import SamImageEncoderEngine, transformers_key
    eng = SamImageEncoderEngine(G.config_dict('A'), torch.float16, 'cpu')
    sd = G.make_weights('A')
    assert sorted(sd) == sorted(eng.expected_parameters())                          # transformers' own SamVisionEncoder state dict
    sa = G.segment_anything_keys(sd)
    assert 'patch_embed.proj.weight' in sa and 'blocks.1.norm2.bias' in sa and 'blocks.0.attn.rel_pos_h' in sa and 'blocks.2.mlp.lin1.weight' in sa
    assert 'neck.0.weight' in sa and 'neck.1.bias' in sa and 'neck.2.weight' in sa and 'neck.3.weight' in sa and 'pos_embed' in sa
    assert not set(sa) & (set(sd) - {'pos_embed'})                                  # every other key is spelled differently
    for layout in (sd, sa):
        for prefix in ('', 'image_encoder.', 'vision_encoder.'):
            mapped = eng.map_state_dict({prefix + k: v for k, v in layout.items()})
            assert sorted(mapped) == sorted(sd) and all(mapped[transformers_key(prefix + k)] is v for k, v in layout.items())
    with pytest.raises(KeyError, match='mask_decoder'):                             # a key of neither layout is refused by name, not skipped
        eng.map_state_dict(dict(sd, **{'mask_decoder.iou_token.weight': np.zeros(1)}))
    with pytest.raises(KeyError, match='another key'):                              # two keys for one destination
        eng.map_state_dict(dict(sd, **{'blocks.0.norm1.weight': sd['layers.0.layer_norm1.weight']}))
    with pytest.raises(ValueError, match='interpolation'):                          # a 64 x 64 table on a 14 x 14 window
        eng.map_state_dict(dict(sd, **{'layers.0.attn.rel_pos_h': np.zeros((127, 64))}))
    with pytest.raises(KeyError, match='neck.conv2.weight'):
        eng.load_state_dict({k: v for k, v in sd.items() if k != 'neck.conv2.weight'})


def test_refusals_come_before_any_launch(lib):
    from mvedit_amd.sam import SAM_VIT_B_CONFIG, SAM_VIT_H_CONFIG, SAM_VIT_L_CONFIG, SamImageEncoderEngine
    cfg = G.config_dict('A')
    eng = SamImageEncoderEngine(cfg, torch.float16, 'cpu')
    assert eng.img_size == 256 and eng.grid == 16 and eng.config.window_size == 14
    with pytest.raises(NotImplementedError, match='output_attentions'):
        eng(torch.zeros(1, 3, 256, 256), output_attentions=True)
    for bad in (torch.zeros(1, 3, 224, 224), torch.zeros(3, 256, 256), torch.zeros(1, 1, 256, 256), torch.zeros(0, 3, 256, 256), None):
        with pytest.raises(ValueError, match=r'\[B, 3, 256, 256\]'):
            eng(bad)
    with pytest.raises(ValueError, match='floating'):
        eng(torch.zeros(1, 3, 256, 256, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match='inference only'):
        eng.train()
    with pytest.raises(NotImplementedError):
        eng.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        eng.to(torch.bfloat16)
    with pytest.raises(NotImplementedError):
        eng.to('cuda')
    assert eng.eval() is eng and eng.train(False) is eng and eng.requires_grad_(False) is eng and eng.to('cpu') is eng and eng.to(torch.float16) is eng
    assert next(eng.parameters()).dtype == torch.float16
    for k, v, match in (('use_rel_pos', False, 'use_rel_pos'), ('use_abs_pos', False, 'use_abs_pos'), ('qkv_bias', False, 'qkv_bias'), ('hidden_act', 'relu', 'hidden_act'),
                        ('num_channels', 1, 'num_channels')):
        with pytest.raises(NotImplementedError, match=match):
            SamImageEncoderEngine(dict(cfg, **{k: v}), torch.float16, 'cpu')
    for k, v, match in (('num_attention_heads', 4, 'head_dim must be 64 or 80'), ('image_size', 250, 'multiple of patch_size'), ('window_size', 17, 'window_size 17'),
                        ('output_channels', 100, 'output_channels 100'), ('mlp_dim', 100, 'mlp_dim 100'), ('global_attn_indexes', (3,), 'global_attn_indexes'),
                        ('image_size', 2048, '64 x 64')):
        with pytest.raises(lib.MveError, match=match):
            SamImageEncoderEngine(dict(cfg, **{k: v}), torch.float16, 'cpu')
    with pytest.raises(lib.MveError, match='2048 channels'):
        SamImageEncoderEngine(dict(cfg, hidden_size=2560, num_attention_heads=32), torch.float16, 'cpu')
    # a forward on an engine without parameters names the first missing one; nothing has been launched
    p = ctypes.c_void_p(torch.zeros(4096).data_ptr())
    with pytest.raises(lib.MveError, match='patch_embed.projection.weight'):
        lib.call('mve_sam_encoder_forward', eng._h, p, 1, p, None, p, 1 << 30, None, None)
    for c, layers, hidden in ((SAM_VIT_H_CONFIG, 32, 1280), (SAM_VIT_L_CONFIG, 24, 1024), (SAM_VIT_B_CONFIG, 12, 768)):
        e = SamImageEncoderEngine(c, torch.bfloat16, 'cpu')
        assert (e.cfg['num_hidden_layers'], e.cfg['hidden_size'], e.img_size, e.grid, len(e.cfg['global_attn_indexes'])) == (layers, hidden, 1024, 64, 4)


def test_vit_h_plan_is_the_op_list_of_the_header(lib):
    from mvedit_amd.sam import SAM_VIT_H_CONFIG, SamImageEncoderEngine
    eng = SamImageEncoderEngine(SAM_VIT_H_CONFIG, torch.float16, 'cpu')
    info = eng.plan(1)
    labels = [lab for _, _, lab in eng.op_table()]
    count = lambda s: sum(lab == s for lab in labels)
    assert labels[:4] == ['patchify', 'patch_embed', 'position embedding', 'hidden state -> output']
    assert labels[-5:] == ['neck.conv1', 'layernorm', 'neck.conv2', 'layernorm', 'nhwc->nchw']
    assert count('rel-pos attention (windows)') == count('window partition') == count('window un-partition') == 28 and count('rel-pos attention (global)') == 4
    assert count('attn.qkv') == count('attn.proj+residual') == count('mlp.lin1') == count('gelu') == count('mlp.lin2+residual') == 32
    assert count('layernorm') == 66 and count('hidden state -> output') == 33 and info['n_ops'] == len(labels) == 353
    # block 7 is the first global one: no partition around its attention
    i = [k for k, lab in enumerate(labels) if lab == 'rel-pos attention (global)'][0]
    assert labels[i - 2:i + 2] == ['layernorm', 'attn.qkv', 'rel-pos attention (global)', 'attn.proj+residual']
    M, C, I, Mw = 4096, 1280, 5120, 25 * 196
    linear = 2.0 * M * C * 768 + 28 * 2.0 * Mw * 3 * C * C + 4 * 2.0 * M * 3 * C * C + 32 * (2.0 * M * C * C + 4.0 * M * C * I) + 2.0 * M * 256 * C
    attn = 28 * 4.0 * 25 * 16 * 196 * 196 * 80 + 4 * 4.0 * 16 * 4096 * 4096 * 80
    assert info['flops']['linear'] == pytest.approx(linear, rel=1e-12) and info['flops']['attention'] == pytest.approx(attn, rel=1e-12)
    assert info['flops']['conv'] == pytest.approx(2.0 * M * 256 * 9 * 256, rel=1e-12)
    assert 4.5e12 < linear < 6e12                                                   # "about 5 TFLOP" of linears
    # the widest live set: the padded q|k|v rows, their source, the residual stream -- tens of MB, and linear in the batch
    assert 40e6 < info['workspace_bytes'] < 120e6
    assert 1.9 < eng.plan(2)['workspace_bytes'] / info['workspace_bytes'] < 2.1 and eng.plan(2)['n_ops'] == 353


def test_c_abi_argument_errors_name_the_argument(lib):
    """host logic only: each call fails its checks before the device is touched (the pointers are host addresses that are never read)"""
    buf = torch.zeros(4096)
    p, f = ctypes.c_void_p(buf.data_ptr()), ctypes.c_float
    odd = ctypes.c_void_p(p.value + 2)

    def bad(name, *args, match):
        with pytest.raises(lib.MveError, match=match):
            lib.call(name, *args)
    ok = (1, p, 384, p, 384, p, 384, p, p, p, 128, 3, 14, 14, 2, 64, f(0.125), None)

    def attn(**kw):
        names = ('dtype', 'Q', 'ldq', 'K', 'ldk', 'V', 'ldv', 'rel_h', 'rel_w', 'O', 'ldo', 'NS', 'gh', 'gw', 'heads', 'head_dim', 'scale', 'stream')
        return tuple(kw.get(n, v) for n, v in zip(names, ok))
    bad('mve_attention_relpos', *attn(dtype=0), match='dtype')
    bad('mve_attention_relpos', *attn(rel_w=None), match='null')
    bad('mve_attention_relpos', *attn(head_dim=48), match='head_dim 48')
    bad('mve_attention_relpos', *attn(gh=115), match='gh 115')                 # 115 + 14 > 128: the two tables of a query do not fit
    bad('mve_attention_relpos', *attn(gw=0), match='gw 0')
    bad('mve_attention_relpos', *attn(NS=0), match='NS 0')
    bad('mve_attention_relpos', *attn(ldq=100), match='ldq 100')
    bad('mve_attention_relpos', *attn(ldk=388), match='ldk 388')
    bad('mve_attention_relpos', *attn(ldv=64), match='ldv 64')
    bad('mve_attention_relpos', *attn(ldo=64), match='ldo 64')
    bad('mve_attention_relpos', *attn(rel_h=odd), match='aligned')
    bad('mve_attention_relpos', *attn(scale=f(0.0)), match='scale')
    for name in ('mve_sam_window_partition', 'mve_sam_window_unpartition'):
        bad(name, 0, p, 1, 16, 64, 14, p, None, match='dtype')
        bad(name, 1, p, 1, 16, 64, 14, None, None, match='null')
        bad(name, 1, p, 1, 16, 60, 14, p, None, match=' C 60 ')
        bad(name, 1, p, 1, 16, 64, 17, p, None, match='window 17')
        bad(name, 1, p, 1, 16, 64, 0, p, None, match='window 0')
        bad(name, 1, odd, 1, 16, 64, 14, p, None, match='aligned')
    bad('mve_sam_pos_add', 0, p, p, p, 1, 16, 64, None, match='dtype')
    bad('mve_sam_pos_add', 1, p, None, p, 1, 16, 64, None, match='null')
    bad('mve_sam_pos_add', 1, p, p, p, 1, 16, 60, None, match=' C 60 ')
    bad('mve_sam_pos_add', 1, p, odd, p, 1, 16, 64, None, match='aligned')
    h, g = ctypes.c_void_p(), (ctypes.c_int * 1)(1)
    bad('mve_sam_encoder_create', ctypes.byref(h), 1, 256, 16, 128, 3, 2, 512, 14, g, 1, 256, f(1e-6), 0, 1, match='use_rel_pos')
    bad('mve_sam_encoder_create', ctypes.byref(h), 1, 256, 16, 128, 3, 2, 512, 14, g, 1, 256, f(1e-6), 1, 0, match='use_abs_pos')
    bad('mve_sam_encoder_create', ctypes.byref(h), 3, 256, 16, 128, 3, 2, 512, 14, g, 1, 256, f(1e-6), 1, 1, match='dtype')
    assert not h.value
    from mvedit_amd.sam import SamImageEncoderEngine
    eng, text = SamImageEncoderEngine(G.config_dict('A'), torch.float16, 'cpu'), ctypes.c_void_p()
    lib.call('mve_clip_text_create', ctypes.byref(text), 1, 512, 77, 128, 2, 2, 512, 0, f(1e-5), 0)
    try:
        bad('mve_sam_encoder_plan', text, 1, None, None, None, match='not a SAM image encoder')
        bad('mve_sam_encoder_forward', text, p, 1, p, None, p, 1 << 20, None, None, match='not a SAM image encoder')
        bad('mve_clip_vision_plan', eng._h, 1, None, None, None, match='a SAM image encoder, not a CLIP vision tower')
        shape = (ctypes.c_longlong * 2)(127, 64)
        bad('mve_unet_load_param', eng._h, b'layers.0.attn.rel_pos_h', p, 0, 2, shape, None, match='expected 1728 elements')      # 27 x 64: no interpolation
        bad('mve_unet_load_param', eng._h, b'blocks.0.norm1.weight', p, 0, 2, shape, None, match='not a parameter')
    finally:
        lib.call('mve_sam_encoder_destroy', text)


# ---- drop-in ------------------------------------------------------------------------------------------------------------------------------
class ImageEncoderViT(torch.nn.Module):
    """stand-in with what `config_from_image_encoder_vit` reads off segment_anything's module"""

    def __init__(self, case='A'):
        super().__init__()
        c = G.config_dict(case)
        self.img_size = c['image_size']
        self.patch_embed = torch.nn.Module()
        self.patch_embed.proj = torch.nn.Conv2d(3, c['hidden_size'], 16, 16)
        self.pos_embed = torch.nn.Parameter(torch.zeros(1, 16, 16, c['hidden_size']))
        self.blocks = torch.nn.ModuleList()
        for k in range(c['num_hidden_layers']):
            b = torch.nn.Module()
            b.window_size = 0 if k in c['global_attn_indexes'] else c['window_size']
            b.norm1 = torch.nn.LayerNorm(c['hidden_size'], eps=1e-6)
            b.attn = torch.nn.Module()
            b.attn.num_heads, b.attn.use_rel_pos = c['num_attention_heads'], True
            b.attn.qkv = torch.nn.Linear(c['hidden_size'], 3 * c['hidden_size'])
            b.mlp = torch.nn.Module()
            b.mlp.lin1 = torch.nn.Linear(c['hidden_size'], c['mlp_dim'])
            self.blocks.append(b)
        self.neck = torch.nn.Sequential(torch.nn.Conv2d(c['hidden_size'], 256, 1, bias=False))


class Sam(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.image_encoder = ImageEncoderViT()
        self.prompt_encoder, self.mask_decoder = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)


def test_swap_sam_image_encoder_is_opt_in_and_undone(lib, monkeypatch):
    from mvedit_amd import dropin
    from mvedit_amd.sam import SamImageEncoderEngine, config_from_image_encoder_vit
    assert 'predictor' not in dropin.SWAPPED_ATTRS and 'image_encoder' not in dropin.MAKERS
    sam = Sam()
    enc = sam.image_encoder
    want = G.config_dict('A')
    assert config_from_image_encoder_vit(enc) == want
    runner = SimpleNamespace(predictor=SimpleNamespace(model=sam))                 # Adapter3DRunner after load_sam_predictor
    dropin.swap_engines(runner)
    dropin.install()
    try:
        assert sam.image_encoder is enc                                            # neither the default swap nor install() touches the predictor
    finally:
        dropin.uninstall()
    empty = SimpleNamespace(predictor=None)
    assert dropin.swap_sam_image_encoder(empty) is empty and empty.predictor is None
    with pytest.raises(RuntimeError, match='CPU'):                                 # the makers' on-accelerator check
        dropin.swap_sam_image_encoder(runner)
    assert sam.image_encoder is enc
    made = []
    real = SamImageEncoderEngine.from_module.__func__

    def from_module(m, dtype=None, device=None):
        eng = real(SamImageEncoderEngine, m, dtype=dtype, device='cpu')            # the construction is observed; the packing (which needs the device) is not run
        made.append((m, eng))
        return eng
    monkeypatch.setattr(dropin, '_module_dtype_device', lambda m: (torch.float16, torch.device('cuda', 0)))
    monkeypatch.setattr(SamImageEncoderEngine, 'from_module', staticmethod(from_module))
    assert dropin.swap_sam_image_encoder(runner) is runner
    eng = sam.image_encoder
    assert isinstance(eng, SamImageEncoderEngine) and [m for m, _ in made] == [enc] and eng.cfg == want and eng.img_size == 256
    # Sam is an nn.Module: the engine sits past nn.Module.__setattr__, the torch encoder stays registered, the other two members are untouched
    assert sam._modules['image_encoder'] is enc and 'image_encoder.pos_embed' in sam.state_dict() and isinstance(sam.mask_decoder, torch.nn.Linear)
    dropin.swap_sam_image_encoder(runner)                                          # idempotent
    dropin.swap_sam_image_encoder(runner.predictor)                                # a SamPredictor
    dropin.swap_sam_image_encoder(sam)                                             # the Sam model itself
    assert sam.image_encoder is eng and len(made) == 1
    other = SimpleNamespace(image_encoder=enc)                                     # a Sam-like plain object over the same module shares the engine
    dropin.swap_sam_image_encoder(other)
    assert other.image_encoder is eng and len(made) == 1
    dropin.uninstall()                                                             # undone, whether or not install() ran
    assert sam.image_encoder is enc and other.image_encoder is enc
    with torch.no_grad():                                                          # a changed parameter rebuilds
        enc.patch_embed.proj.weight.add_(1)
    dropin.swap_sam_image_encoder(sam)
    assert sam.image_encoder is not eng and isinstance(sam.image_encoder, SamImageEncoderEngine) and len(made) == 2
    dropin.uninstall()
    assert sam.image_encoder is enc
    # transformers' classes are read through their config
    tf = SimpleNamespace(config=SimpleNamespace(vision_config=SimpleNamespace(**G.config_dict('B'))), parameters=lambda: iter([torch.zeros(1)]))
    assert real(SamImageEncoderEngine, tf).cfg == G.config_dict('B')
    with pytest.raises(TypeError, match='neither'):
        real(SamImageEncoderEngine, torch.nn.Linear(2, 2))
