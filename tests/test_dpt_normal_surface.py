"""DPTNormalEngine without a GPU: the refusals (all before the library launches anything), the key table of both checkpoint layouts, the pack-time
weight standardisation, the opt-in drop-in swap, and the full-size plan."""
import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_dpt_normal_golden', os.path.join(HERE, 'golden', 'make_dpt_normal_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _engine(lib, case='A', **kw):
    from mvedit_amd.normal_model import DPTNormalEngine
    return DPTNormalEngine(dict(G.engine_config(case), **kw.pop('cfg', {})), device='cpu', **kw)


def _forbid_forward(lib, monkeypatch):
    """Any refusal must come before the library is touched: the forward and the parameter loader raise if they are reached."""
    real = lib.call

    def guarded(name, *a):
        assert name not in ('mve_dpt_forward', 'mve_unet_load_param'), f'{name} was reached'
        return real(name, *a)
    monkeypatch.setattr(lib, 'call', guarded)


def test_refusals_come_before_any_launch(lib, monkeypatch):
    from mvedit_amd.normal_model import DPTNormalEngine
    _forbid_forward(lib, monkeypatch)
    eng = _engine(lib)
    assert eng.dtype == torch.float16 and eng.device == torch.device('cpu') and eng.num_tokens == 37 and eng.config.features == 64
    for bad in (torch.zeros(2, 1, 96, 96), torch.zeros(3, 96, 96), torch.zeros(0, 3, 96, 96), torch.zeros(2, 3, 96, 64), torch.zeros(2, 3, 96, 96, 1), None):
        with pytest.raises(ValueError, match=r'\[B, 3, S, S\]'):
            eng(bad)
    for S in (100, 48, 80):
        with pytest.raises(ValueError, match='multiple of 32'):
            eng(torch.zeros(1, 3, S, S))
    with pytest.raises(ValueError, match='floating'):
        eng(torch.zeros(1, 3, 96, 96, dtype=torch.uint8))
    for S in (128, 64, 384):                  # a token grid other than the position table's: the reference would resample the table
        with pytest.raises(NotImplementedError, match='position table'):
            eng(torch.zeros(1, 3, S, S))
    with pytest.raises(NotImplementedError, match='project'):
        _engine(lib, cfg=dict(readout='ignore'))
    with pytest.raises(NotImplementedError, match='project'):
        _engine(lib, cfg=dict(readout='add'))
    with pytest.raises(NotImplementedError, match='hybrid'):
        _engine(lib, cfg=dict(backbone='vitl16_384'))
    with pytest.raises(NotImplementedError, match='head_dim 64'):
        _engine(lib, cfg=dict(hidden_size=160, num_heads=2))
    with pytest.raises(NotImplementedError, match='head_dim 64'):
        _engine(lib, cfg=dict(hidden_size=96, num_heads=3))
    with pytest.raises(ValueError, match='tap_layers'):
        DPTNormalEngine({k: v for k, v in G.engine_config('A').items() if k != 'tap_layers'}, device='cpu')
    with pytest.raises(NotImplementedError, match='inference only'):
        eng.requires_grad_(True)
    assert eng.requires_grad_(False) is eng and eng.eval() is eng and next(eng.parameters()).dtype == torch.float16
    assert eng.to('cpu') is eng and eng.to(torch.float16) is eng and eng.to('cpu', dtype=torch.float16) is eng
    for a, kw in (((torch.float32,), {}), ((torch.bfloat16,), {}), (('cuda',), {}), ((), dict(device='cuda:1')), ((), dict(dtype=torch.float64))):
        with pytest.raises(NotImplementedError):
            eng.to(*a, **kw)
    # geometry the kernels do not take is refused at create, by name
    for bad, match in ((dict(image_size=2080), 'image_size'), (dict(num_channels=9), 'num_channels'), (dict(features=24), 'features'),
                       (dict(stage_widths=(64, 128, 200)), 'stage_widths'), (dict(num_groups=3), 'num_groups'), (dict(tap_layers=(3, 1)), 'tap_layers'),
                       (dict(tap_layers=(1, 4)), 'tap_layers'), (dict(neck_channels=(100, 128)), 'neck_channels'), (dict(intermediate_size=100), 'intermediate_size')):
        with pytest.raises(lib.MveError, match=match):
            _engine(lib, cfg=bad)
    # a state dict with a dropped or an unknown key is refused before anything is packed
    with pytest.raises(KeyError):
        eng.load_state_dict({})
    with pytest.raises(NotImplementedError):
        eng.load_state_dict({}, strict=False)


def _reference_state(case):
    """The case's weights under the reference checkpoint's names, with the keys that checkpoint carries and the engine drops."""
    from mvedit_amd.normal_model import key_table
    cfg = G.engine_config(case)
    tr, ref = key_table(cfg, 'transformers'), key_table(cfg, 'reference')
    w = {k: torch.from_numpy(v) for k, v in G.make_weights(case).items()}
    sd = {}
    for logical, key in ref.items():
        if '?' in logical:
            sd[key] = torch.zeros(3)                     # timm's classifier head: optional, dropped
        elif '.qkv.' in logical:
            sd[key] = torch.cat([w[tr[logical.replace('.qkv.', f'.{n}.')]] for n in 'qkv'], 0)
        else:
            sd[key] = w[tr[logical]]
    return sd


@pytest.mark.parametrize('case', ['A', 'B'])
def test_each_layout_is_consumed_exactly_once_and_a_dropped_key_is_named(lib, case):
    from mvedit_amd.normal_model import detect_layout, key_table, match_state_dict, pack_slots
    cfg = G.engine_config(case)
    tr = {k: torch.from_numpy(v) for k, v in G.make_weights(case).items()}
    ref = _reference_state(case)
    assert detect_layout(tr) == 'transformers' and detect_layout(ref) == 'reference'
    # the transformers table is exactly that module's state dict (the generator loads these names into DPTForDepthEstimation with strict checks)
    assert set(key_table(cfg, 'transformers').values()) == set(tr)
    table = key_table(cfg, 'reference')
    assert len(set(table.values())) == len(table)                                      # no key is named twice
    # the reference's own constructors name the decoder half (blocks.py:62-73, :313-316, :247-252; vit.py:41, :431-462; dpt_depth.py:91-99)
    for key in ('scratch.layer1_rn.weight', 'scratch.layer4_rn.weight', 'scratch.refinenet4.resConfUnit1.conv1.weight', 'scratch.refinenet1.resConfUnit2.conv2.bias',
                'scratch.refinenet2.out_conv.weight', 'scratch.output_conv.0.weight', 'scratch.output_conv.2.bias', 'scratch.output_conv.4.weight',
                'pretrained.act_postprocess3.0.project.0.weight', 'pretrained.act_postprocess3.3.weight', 'pretrained.act_postprocess4.3.bias',
                'pretrained.act_postprocess4.4.weight',
                # timm's naming of vit_base_resnet50_384, restated (unverified: timm is not a dependency)
                'pretrained.model.patch_embed.backbone.stem.conv.weight', 'pretrained.model.patch_embed.backbone.stem.norm.bias',
                'pretrained.model.patch_embed.backbone.stages.0.blocks.0.downsample.conv.weight', 'pretrained.model.patch_embed.backbone.stages.2.blocks.0.norm3.weight',
                'pretrained.model.patch_embed.proj.weight', 'pretrained.model.cls_token', 'pretrained.model.pos_embed', 'pretrained.model.blocks.0.attn.qkv.weight',
                'pretrained.model.blocks.1.mlp.fc2.bias', 'pretrained.model.norm.weight'):
        assert key in table.values(), key
    a, b = match_state_dict(cfg, tr), match_state_dict(cfg, ref)
    sa, sb = pack_slots(cfg, a), pack_slots(cfg, b)
    assert list(sa) == list(sb) and all(torch.equal(sa[k].double(), sb[k].double()) for k in sa)      # both layouts pack to the same slots
    assert not any(k.startswith('_') for k in a) and 'f4.u1.c1.w' not in sa and f'l{cfg["tap_layers"][1]}.qkv.w' in sa
    assert sa['stem.w'].shape == (cfg['stem_width'], 152) and bool((sa['stem.w'][:, 147:] == 0).all())
    assert sa['h4.w'].shape == (8, 32) and bool((sa['h4.w'][cfg['num_channels']:] == 0).all()) and sa['r3.wt'].shape == sa['r3.wc'].shape
    for sd, layout in ((tr, 'transformers'), (ref, 'reference')):
        for key in list(sd)[::7]:
            if 'model.head.' in key:
                continue                                   # optional
            short = {k: v for k, v in sd.items() if k != key}
            with pytest.raises(KeyError, match=key.replace('.', r'\.')):
                match_state_dict(cfg, short, layout)
        with pytest.raises(KeyError, match=r'not\.a\.parameter'):
            match_state_dict(cfg, dict(sd, **{'not.a.parameter': torch.zeros(1)}), layout)
    without_head = {k: v for k, v in ref.items() if 'model.head.' not in k}
    assert set(match_state_dict(cfg, without_head)) == set(b)


def test_pack_time_standardisation_is_the_modules_forward_formula():
    from mvedit_amd.normal_model import WS_EPS, conv_k_order, standardize_weight
    g = torch.Generator().manual_seed(3)
    for shape in ((32, 3, 7, 7), (16, 64, 1, 1), (16, 16, 3, 3)):
        w = (0.05 * torch.randn(shape, generator=g) + 0.02).double()
        # transformers WeightStandardizedConv2d.forward / timm StdConv2dSame.forward, in float64
        want = torch.nn.functional.batch_norm(w.reshape(1, shape[0], -1), None, None, training=True, momentum=0.0, eps=1e-8).reshape_as(w)
        got = standardize_weight(w)
        assert WS_EPS == 1e-8 and got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12
        assert float(got.reshape(shape[0], -1).mean(1).abs().max()) < 1e-12 and float((got.reshape(shape[0], -1).var(1, unbiased=False) - 1).abs().max()) < 1e-4
        assert standardize_weight(w.half()).dtype == torch.float64                    # 16-bit checkpoints are standardised in float64 too
    # the conv K order: [O][3][3][I], and [O][I/64][3][3][64] once I is a multiple of 64 (MVE_CONV_W_CHUNK64)
    w = torch.arange(8 * 16 * 9, dtype=torch.float32).reshape(8, 16, 3, 3)
    assert torch.equal(conv_k_order(w), w.permute(0, 2, 3, 1))
    w = torch.arange(8 * 128 * 9, dtype=torch.float32).reshape(8, 128, 3, 3)
    k = conv_k_order(w)
    assert k.shape == (8, 2, 3, 3, 64) and float(k[3, 1, 2, 0, 5]) == float(w[3, 64 + 5, 2, 0])


def test_swap_normal_model_is_opt_in(lib, monkeypatch):
    from mvedit_amd import dropin
    made = []

    class Fake(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(4))

    def fake_make(m):
        eng = SimpleNamespace(source=m)
        made.append(eng)
        return eng
    monkeypatch.setattr(dropin, 'make_normal_model', fake_make)
    pipe = SimpleNamespace(normal_model=Fake(), unet=None)
    src = pipe.normal_model
    assert dropin.swap_normal_model(pipe) is pipe and pipe.normal_model is made[0] and made[0].source is src and made[0]._mve_is_engine
    dropin.swap_normal_model(pipe)                                  # idempotent: the engine is left alone
    assert len(made) == 1 and pipe.normal_model is made[0]
    again = SimpleNamespace(normal_model=src)                       # the engine is cached on the source module
    dropin.swap_normal_model(again)
    assert len(made) == 1 and again.normal_model is made[0]
    none = SimpleNamespace(normal_model=None)
    assert dropin.swap_normal_model(none).normal_model is None and dropin.swap_normal_model(SimpleNamespace()) is not None
    # install() / swap_engines leave normal_model alone
    assert 'normal_model' not in dropin.MAKERS
    import inspect
    assert 'swap_normal_model' not in inspect.getsource(dropin.install) and 'swap_normal_model' not in inspect.getsource(dropin.swap_engines)
    # a module on the CPU is refused by the real maker (nothing is packed without an accelerator), not silently kept
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match='CPU'):
        dropin.swap_normal_model(SimpleNamespace(normal_model=Fake()))


def test_full_size_plan_reports_ops_and_flops(lib):
    from mvedit_amd.normal_model import VITB_RN50_384_CONFIG, DPTNormalEngine
    eng = DPTNormalEngine(device='cpu')
    assert eng.cfg['stage_depths'] == (3, 4, 9) and eng.cfg == dict(VITB_RN50_384_CONFIG) and eng.num_tokens == 577
    B = 2
    info = eng.plan(B)
    labels = [lab for _, _, lab in eng.op_table()]
    assert info['n_ops'] == len(labels) and info['workspace_bytes'] > 0
    assert labels[:5] == ['stem window rows', 'stem.conv 7x7/2', 'stem.norm+relu', 'stem.maxpool 3x3/2', 'stem -> tap'] and labels[-1] == 'NHWC -> NCHW'
    assert labels.count('attention') == 12 and labels.count('bottleneck add+relu') == 16 and labels.count('shortcut stride-2 gather') == 2
    assert labels.count('bottleneck.downsample.norm') == 3 and labels.count('fusion out_conv') == 4 and labels.count('resConfUnit.conv2+residual') == 7
    assert labels.count('readout (token half + class row)') == 2 and labels.count('act_postprocess4 conv3x3/2') == 1
    T, C, I, heads = 577, 768, 3072, 12
    assert info['flops']['attention'] == 12 * 4.0 * B * heads * T * T * 64
    # linear: stem GEMM, bottleneck 1 x 1 convs, the projection, the ViT, the readouts, fusion out_convs, the head's 1 x 1
    vit = 12 * 2.0 * B * T * (3 * C * C + C * C + 2 * C * I)
    assert info['flops']['linear'] > vit + 2.0 * B * 192 * 192 * 64 * 152
    # conv: the 16 bottleneck 3 x 3, four layerN_rn, 14 resConfUnit convs, act_postprocess4's, the head's two
    head = 2.0 * B * (192 * 192 * 128 * 9 * 256 + 384 * 384 * 32 * 9 * 128)
    assert info['flops']['conv'] > head and info['flops']['norm'] == 0 and info['flops']['other'] == 0
    small = _engine(lib, 'B', dtype=torch.bfloat16)
    assert small.dtype == torch.bfloat16 and small.plan(1)['n_ops'] < info['n_ops']
