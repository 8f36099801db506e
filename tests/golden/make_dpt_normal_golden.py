"""Golden for the DPT-hybrid normal predictor engine (mvedit_amd/normal_model.py): transformers' `DPTModel` + neck for the backbone and the neck,
the REFERENCE's own decoder (`_make_scratch`, `ProjectReadout`, `FeatureFusionBlock_custom`, the head `nn.Sequential` of `DPTDepthModel.__init__`)
on the same weights, all in float64 on the CPU.

    python tests/golden/make_dpt_normal_golden.py --reference <root of the reference tree>      (needs `transformers`; writes dpt_normal_ref.npz)

The generator asserts that the reference's decoder and transformers' neck agree in float64 (|diff| <= 1e-12) -- the in-tree half is thereby pinned
to the reference itself -- and takes the head from the reference (transformers' has one channel).  The reference's modules are obtained by import
under an empty stand-in module named `timm` (omnidata_modules/midas/vit.py imports it at the top and uses it in one constructor that is never
called here); the stand-in is seeded AFTER `import transformers`, which probes `timm` with `find_spec`.  The head is cut out of dpt_depth.py with
`ast` (importing that file pulls base_model.py and nothing else, but the Sequential is a local of `__init__`).

Stored per case and tap (TAPS: stem, three stages, the two token taps, the four fusion outputs, the output): the float64 reference as float32 and
the rel-L2 of the `.half()` / `.bfloat16()` CPU modules against float64 (the engine's bar is 1.5 x these).  One committed file may not exceed
1 MiB and the taps of the two cases hold about a million values, so a tap of more than SAMPLE values is stored -- and its 16-bit errors are
measured -- on a fixed pseudo-random subset of SAMPLE flat NCHW positions (`sample_index`, regenerated from the case's seed by the readers).
Weights and pixels are not stored: `make_weights` / `make_pixels` regenerate them from numpy's frozen `RandomState` stream and the readers check
the sha256 recorded here.  All of them are fp16-representable values.

  case A   B = 2, S = 96 (37 tokens), stem 32, stages 64 / 128 / 256 with depths 2 / 1 / 2 (stage 1: a first layer with a shortcut convolution and a
           later one with an identity shortcut), 8 groups, ViT 128 wide / 2 heads / 4 layers tapped after blocks 1 and 3, features 64, 3 channels
  case B   B = 1, S = 128 (65 tokens: an 8 x 8 position table), depths 1 / 2 / 1, ViT 192 wide / 3 heads / 3 layers tapped after blocks 0 and 2,
           features 32, 1 channel (the squeeze)
"""
import argparse
import ast
import hashlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, 'dpt_normal_ref.npz')
SAMPLE = 8192

CASES = {
    'A': dict(B=2, image_size=96, stem_width=32, stage_widths=(64, 128, 256), stage_depths=(2, 1, 2), num_groups=8, hidden_size=128, num_heads=2, num_layers=4,
              tap_layers=(1, 3), neck_channels=(128, 128), features=64, num_channels=3, seed=3101),
    'B': dict(B=1, image_size=128, stem_width=32, stage_widths=(64, 128, 256), stage_depths=(1, 2, 1), num_groups=8, hidden_size=192, num_heads=3, num_layers=3,
              tap_layers=(0, 2), neck_channels=(96, 160), features=32, num_channels=1, seed=3102),
}
LAYER_NORM_EPS = 1e-6          # timm's ViT
TAPS = ('stem', 'stage1', 'stage2', 'stage3', 'tokens3', 'tokens4', 'fusion4', 'fusion3', 'fusion2', 'fusion1', 'output')


def engine_config(case):
    """The case as the engine's own config fields (mvedit_amd.normal_model.CONFIG_FIELDS)."""
    c = CASES[case]
    d = {k: c[k] for k in ('image_size', 'stem_width', 'stage_widths', 'stage_depths', 'num_groups', 'hidden_size', 'num_layers', 'num_heads', 'tap_layers',
                           'neck_channels', 'features', 'num_channels')}
    d.update(intermediate_size=4 * c['hidden_size'], layer_norm_eps=LAYER_NORM_EPS, readout='project', backbone='vitb_rn50_384')
    return d


def n_tokens(case):
    return (CASES[case]['image_size'] // 16) ** 2 + 1


def _fp16(a):
    return a.astype(np.float16).astype(np.float64)


def make_weights(case):
    """-> {transformers DPTForDepthEstimation state-dict name: float64 array of fp16-representable values}; the head (`head.head.{0,2,4}`) has the
    case's num_channels outputs -- the reference's head, under transformers' names."""
    c, rs = CASES[case], np.random.RandomState(CASES[case]['seed'])
    C, I, F, G, nc = c['hidden_size'], 4 * c['hidden_size'], c['features'], c['num_groups'], c['num_channels']
    sd = {}

    def put(name, shape, std, mean=0.0):
        sd[name] = _fp16(mean + std * rs.standard_normal(shape))

    def norm(name, n):
        put(name + '.weight', (n,), 0.1, 1.0)
        put(name + '.bias', (n,), 0.1)

    def conv(name, o, i, k, bias=True, gain=1.0):
        put(name + '.weight', (o, i, k, k), gain * (i * k * k) ** -0.5)
        if bias:
            put(name + '.bias', (o,), 0.1)

    bb = 'dpt.embeddings.backbone.bit.'
    # the standardised convolutions: any scale and a non-zero mean, which the standardisation must remove
    put(bb + 'embedder.convolution.weight', (c['stem_width'], 3, 7, 7), 0.05, 0.02)
    norm(bb + 'embedder.norm', c['stem_width'])
    cin = c['stem_width']
    for s in range(3):
        cout, mid = c['stage_widths'][s], c['stage_widths'][s] // 4
        for m in range(c['stage_depths'][s]):
            b = f'{bb}encoder.stages.{s}.layers.{m}.'
            if m == 0:
                put(b + 'downsample.conv.weight', (cout, cin, 1, 1), 0.05, 0.02)
                norm(b + 'downsample.norm', cout)
            put(b + 'conv1.weight', (mid, cin, 1, 1), 0.05, 0.02)
            norm(b + 'norm1', mid)
            put(b + 'conv2.weight', (mid, mid, 3, 3), 0.05, 0.02)
            norm(b + 'norm2', mid)
            put(b + 'conv3.weight', (cout, mid, 1, 1), 0.05, 0.02)
            norm(b + 'norm3', cout)
            cin = cout
    conv('dpt.embeddings.projection', C, cin, 1, gain=0.5)
    put('dpt.embeddings.cls_token', (1, 1, C), 0.2)
    put('dpt.embeddings.position_embeddings', (1, n_tokens(case), C), 0.2)
    w_attn, w_fc1 = 4.0 * C ** -0.5 * (2 * c['num_layers']) ** -0.5, 4.0 * (2 * C) ** -0.5
    for k in range(c['num_layers']):
        b = f'dpt.encoder.layer.{k}.'
        for n in ('attention.attention.query', 'attention.attention.key', 'attention.attention.value', 'attention.output.dense'):
            put(b + n + '.weight', (C, C), w_attn)
            put(b + n + '.bias', (C,), 0.1)
        put(b + 'intermediate.dense.weight', (I, C), w_fc1)
        put(b + 'intermediate.dense.bias', (I,), 0.1)
        put(b + 'output.dense.weight', (C, I), w_attn)
        put(b + 'output.dense.bias', (C,), 0.1)
        norm(b + 'layernorm_before', C)
        norm(b + 'layernorm_after', C)
    norm('dpt.layernorm', C)
    neck = (c['stage_widths'][0], c['stage_widths'][1]) + tuple(c['neck_channels'])
    for i in (2, 3):
        conv(f'neck.reassemble_stage.layers.{i}.projection', neck[i], C, 1)
    conv('neck.reassemble_stage.layers.3.resize', neck[3], neck[3], 3)
    for i in (2, 3):
        put(f'neck.reassemble_stage.readout_projects.{i}.0.weight', (C, 2 * C), (2 * C) ** -0.5)
        put(f'neck.reassemble_stage.readout_projects.{i}.0.bias', (C,), 0.1)
    for i in range(4):
        conv(f'neck.convs.{i}', F, neck[i], 3, bias=False)
    for i in range(4):
        f = f'neck.fusion_stage.layers.{i}.'
        conv(f + 'projection', F, F, 1)
        for u in ('residual_layer1', 'residual_layer2'):
            conv(f + u + '.convolution1', F, F, 3)
            conv(f + u + '.convolution2', F, F, 3, gain=0.5)
    conv('head.head.0', F // 2, F, 3)
    conv('head.head.2', 32, F // 2, 3)
    conv('head.head.4', nc, 32, 1)
    sd['head.head.4.bias'] = _fp16(sd['head.head.4.bias'] + 0.2)          # about half of the outputs above the trailing ReLU's zero
    return sd


def make_pixels(case):
    """float64 [B, 3, S, S] of fp16-representable values in a normalised image's range."""
    c = CASES[case]
    rs = np.random.RandomState(c['seed'] * 10)
    S = c['image_size']
    ramp = np.linspace(-1.0, 1.0, S)
    px = 0.5 * rs.standard_normal((c['B'], 3, S, S)) + 0.5 * ramp[None, None, :, None] * (1 + np.arange(c['B']))[:, None, None, None] - 0.5 * ramp[None, None, None, :]
    return _fp16(px)


def digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].astype(np.float16)).tobytes())
    return h.hexdigest()


def sample_index(case, tap, n):
    """The flat (NCHW / [B,T,C]) positions of a tap of n values that are stored: all of them up to SAMPLE, else SAMPLE sorted positions drawn without
    replacement from the case's seed and the tap's number."""
    if n <= SAMPLE:
        return np.arange(n)
    rs = np.random.RandomState(CASES[case]['seed'] * 100 + TAPS.index(tap))
    return np.sort(rs.choice(n, SAMPLE, replace=False))


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- transformers' side -------------------------------------------------------------------------------------------------------------------------------
def transformers_config(case):
    from transformers import BitConfig, DPTConfig
    c = CASES[case]
    G = c['image_size'] // 16
    bc = BitConfig(layer_type='bottleneck', global_padding='same', embedding_dynamic_padding=True, out_features=['stage1', 'stage2', 'stage3'],
                   embedding_size=c['stem_width'], hidden_sizes=list(c['stage_widths']), depths=list(c['stage_depths']), num_groups=c['num_groups'])
    return DPTConfig(is_hybrid=True, readout_type='project', neck_ignore_stages=[0, 1], reassemble_factors=[1, 1, 1, 0.5], backbone_config=bc,
                     hidden_size=c['hidden_size'], num_attention_heads=c['num_heads'], num_hidden_layers=c['num_layers'], intermediate_size=4 * c['hidden_size'],
                     image_size=c['image_size'], patch_size=16, backbone_out_indices=[0, 0, c['tap_layers'][0], c['tap_layers'][1]],
                     neck_hidden_sizes=[c['stage_widths'][0], c['stage_widths'][1], c['neck_channels'][0], c['neck_channels'][1]],
                     fusion_hidden_size=c['features'], backbone_featmap_shape=[1, c['stage_widths'][2], G, G], layer_norm_eps=LAYER_NORM_EPS, hidden_act='gelu',
                     qkv_bias=True)


def build_module(case, dtype):
    """transformers' DPTForDepthEstimation with the case's weights (its own one-channel head keeps its initialisation: it is not used)."""
    import torch
    from transformers import DPTForDepthEstimation
    m = DPTForDepthEstimation(transformers_config(case))
    sd = {k: torch.from_numpy(v) for k, v in make_weights(case).items() if not k.startswith('head.')}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith('head.') for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


# ---- the reference's side -----------------------------------------------------------------------------------------------------------------------------
def load_reference(root):
    """-> namespace with the reference's `_make_scratch`, `FeatureFusionBlock_custom`, `Interpolate`, `ProjectReadout` and `make_head(features,
    num_channels)` -- the head Sequential of DPTDepthModel.__init__, cut out with `ast`."""
    import transformers  # noqa: F401  (before the stand-in: transformers probes `timm` with find_spec and raises on a spec-less module)
    import torch.nn as nn
    if 'timm' not in sys.modules:
        sys.modules['timm'] = types.ModuleType('timm')
    if root not in sys.path:
        sys.path.insert(0, root)
    from omnidata_modules.midas import blocks, vit
    with open(os.path.join(root, 'omnidata_modules', 'midas', 'dpt_depth.py')) as fh:
        tree = ast.parse(fh.read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'DPTDepthModel']
    init = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name == '__init__']
    head = [n for n in init[0].body if isinstance(n, ast.Assign) and getattr(n.targets[0], 'id', None) == 'head']
    assert len(head) == 1, 'the head Sequential was not found in DPTDepthModel.__init__'
    code = compile(ast.Expression(body=head[0].value), 'dpt_depth.py::DPTDepthModel.__init__::head', 'eval')

    def make_head(features, num_channels):
        return eval(code, {'nn': nn, 'Interpolate': blocks.Interpolate, 'features': features, 'num_channels': num_channels, 'non_negative': True})

    return types.SimpleNamespace(make_scratch=blocks._make_scratch, FeatureFusionBlock_custom=blocks.FeatureFusionBlock_custom, Interpolate=blocks.Interpolate,
                                 ProjectReadout=vit.ProjectReadout, make_head=make_head)


def build_reference_decoder(case, ref, dtype):
    """The reference's modules with the case's weights: (readout3, readout4, post3, post4, scratch with refinenet1-4, head)."""
    import torch
    import torch.nn as nn
    c, w = CASES[case], make_weights(case)
    C, F, N = c['hidden_size'], c['features'], c['neck_channels']
    t = lambda k: torch.from_numpy(w[k])
    ro = {}
    for n, i in ((3, 2), (4, 3)):
        r = ref.ProjectReadout(C, 1)
        r.load_state_dict({'project.0.weight': t(f'neck.reassemble_stage.readout_projects.{i}.0.weight'),
                           'project.0.bias': t(f'neck.reassemble_stage.readout_projects.{i}.0.bias')}, strict=True)
        ro[n] = r
    # act_postprocess3[3] and act_postprocess4[3:5] of _make_vit_b_rn50_backbone (vit.py:431-462): Conv2d 1x1; Conv2d 1x1 + Conv2d 3x3 stride 2 padding 1
    post3 = nn.Sequential(nn.Conv2d(C, N[0], kernel_size=1, stride=1, padding=0))
    post4 = nn.Sequential(nn.Conv2d(C, N[1], kernel_size=1, stride=1, padding=0), nn.Conv2d(N[1], N[1], kernel_size=3, stride=2, padding=1))
    post3.load_state_dict({'0.weight': t('neck.reassemble_stage.layers.2.projection.weight'), '0.bias': t('neck.reassemble_stage.layers.2.projection.bias')})
    post4.load_state_dict({'0.weight': t('neck.reassemble_stage.layers.3.projection.weight'), '0.bias': t('neck.reassemble_stage.layers.3.projection.bias'),
                           '1.weight': t('neck.reassemble_stage.layers.3.resize.weight'), '1.bias': t('neck.reassemble_stage.layers.3.resize.bias')})
    scratch = ref.make_scratch([c['stage_widths'][0], c['stage_widths'][1], N[0], N[1]], F, groups=1, expand=False)
    sd = {f'layer{i + 1}_rn.weight': t(f'neck.convs.{i}.weight') for i in range(4)}
    for n in (1, 2, 3, 4):
        setattr(scratch, f'refinenet{n}', ref.FeatureFusionBlock_custom(F, nn.ReLU(False), deconv=False, bn=False, expand=False, align_corners=True))
        f = f'neck.fusion_stage.layers.{4 - n}.'
        for s in ('weight', 'bias'):
            sd[f'refinenet{n}.out_conv.{s}'] = t(f + 'projection.' + s)
            for ui in (1, 2):
                for ci in (1, 2):
                    sd[f'refinenet{n}.resConfUnit{ui}.conv{ci}.{s}'] = t(f + f'residual_layer{ui}.convolution{ci}.{s}')
    scratch.load_state_dict(sd, strict=True)
    head = ref.make_head(F, c['num_channels'])
    head.load_state_dict({f'{i}.{s}': t(f'head.head.{i}.{s}') for i in (0, 2, 4) for s in ('weight', 'bias')}, strict=True)
    mods = (ro[3], ro[4], post3, post4, scratch, head)
    for m in mods:
        m.to(dtype).eval()
    return mods


def run_case(case, ref, dtype, check_decoders=False):
    """-> {tap: float64 array} of the `dtype` CPU modules: transformers' DPTModel and neck, the reference's head (and, with check_decoders, the
    reference's whole decoder next to transformers' neck, asserted equal)."""
    import torch
    c = CASES[case]
    G = c['image_size'] // 16
    m = build_module(case, dtype)
    ro3, ro4, post3, post4, scratch, head = build_reference_decoder(case, ref, dtype)
    feats = {}
    bit = m.dpt.embeddings.backbone.bit
    hooks = [bit.embedder.register_forward_hook(lambda mod, i, o: feats.__setitem__('stem', o))]
    for s in range(3):
        hooks.append(bit.encoder.stages[s].register_forward_hook(lambda mod, i, o, s=s: feats.__setitem__(f'stage{s + 1}', o)))
    with torch.no_grad():
        px = torch.from_numpy(make_pixels(case)).to(dtype)
        out = m.dpt(px, output_hidden_states=True)
        for h in hooks:
            h.remove()
        hs = out.hidden_states
        feats['tokens3'], feats['tokens4'] = hs[c['tap_layers'][0] + 1], hs[c['tap_layers'][1] + 1]
        assert torch.equal(out.intermediate_activations[0], feats['stage1']) and torch.equal(out.intermediate_activations[1], feats['stage2'])
        fused = m.neck([feats['stage1'], feats['stage2'], feats['tokens3'], feats['tokens4']], patch_height=G, patch_width=G)
        for k, f in enumerate(fused):
            feats[f'fusion{4 - k}'] = f
        if check_decoders:
            # the reference's forward_vit / DPT.forward (vit.py:61-99, dpt_depth.py:71-83) on the same taps
            l3 = post3(ro3(feats['tokens3']).transpose(1, 2).unflatten(2, (G, G)))
            l4 = post4(ro4(feats['tokens4']).transpose(1, 2).unflatten(2, (G, G)))
            p4 = scratch.refinenet4(scratch.layer4_rn(l4))
            p3 = scratch.refinenet3(p4, scratch.layer3_rn(l3))
            p2 = scratch.refinenet2(p3, scratch.layer2_rn(feats['stage2']))
            p1 = scratch.refinenet1(p2, scratch.layer1_rn(feats['stage1']))
            for n, p in ((4, p4), (3, p3), (2, p2), (1, p1)):
                d = float((p - feats[f'fusion{n}']).abs().max())
                assert d <= 1e-12, (case, n, d, "the reference's decoder and transformers' neck disagree in float64")
        feats['output'] = head(feats['fusion1']).squeeze(dim=1)          # DPTDepthModel.forward
    return {k: v.double().numpy() for k, v in feats.items()}


def generate(case, ref):
    import torch
    out = {}
    key = f'{case}.'
    out[key + 'weights_sha256'] = np.array(digest(make_weights(case)))
    out[key + 'pixels_sha256'] = np.array(digest({'pixels': make_pixels(case)}))
    full = run_case(case, ref, torch.float64, check_decoders=True)
    assert full['output'].min() >= 0.0 and 0.2 < float((full['output'] > 0).mean()) < 0.98, (case, float((full['output'] > 0).mean()))
    idx = {t: sample_index(case, t, full[t].size) for t in TAPS}
    for t in TAPS:
        out[key + t] = full[t].reshape(-1)[idx[t]].astype(np.float32)
        out[key + t + '.shape'] = np.array(full[t].shape)
    for tag, dtype in (('fp16', torch.float16), ('bf16', torch.bfloat16)):
        low = run_case(case, ref, dtype)
        for t in TAPS:
            err = rel_l2(low[t].reshape(-1)[idx[t]], full[t].reshape(-1)[idx[t]])
            out[key + f'err_{tag}.' + t] = np.array(err)
            if tag == 'fp16':
                # a structural error shows at 1e-1 or more: 1.5 x this bound keeps the engine's bar a factor three below that
                assert err < 2e-2, (case, t, err, 'the fixture is too hot to discriminate')
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='root of the reference tree (read for omnidata_modules/midas only)')
    args = ap.parse_args()
    ref = load_reference(os.path.abspath(args.reference))
    out = {}
    for case in CASES:
        out.update(generate(case, ref))
    np.savez_compressed(REF, **out)
    for k in sorted(out):
        if out[k].ndim == 0:
            print(f'{k:32s} {out[k]}')
    print(REF, os.path.getsize(REF), 'bytes')
    assert os.path.getsize(REF) < (1 << 20), 'a committed file may not exceed 1 MiB'


if __name__ == '__main__':
    sys.exit(main())
