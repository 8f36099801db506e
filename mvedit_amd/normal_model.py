"""Host-side mirror of the reference's normal predictor -- Omnidata's `DPTDepthModel(backbone='vitb_rn50_384', num_channels=3)` ("DPT Hybrid":
omnidata_modules/midas/dpt_depth.py:87-107, loaded at lib/apis/adapter3d.py:338-352, called through `enable_normals`,
lib/pipelines/mvedit_3d_pipeline.py:262-273) -- on the native executor (csrc/unet.hip in DPT mode, csrc/builder_dpt.h, csrc/dpt.hip):

    normal_model(F.interpolate(images, 384).to(dtype)).clamp(0, 1)

`load_state_dict` takes the layout of the checkpoint the runner loads (`pretrained.model.*`, `pretrained.act_postprocess{3,4}.*`, `scratch.*`)
or transformers' `DPTForDepthEstimation` layout (`dpt.*`, `neck.*`, `head.*`); neither `timm` nor `transformers` is imported here.  Everything
that is more than a copy happens once, at load: the ResNetV2's weight standardisation (float64, the module's eps, then ONE rounding to the engine
dtype), the q|k|v concatenation, the split of the "project" readout's Linear into its token and class halves, the convolutions' K order.  What
the kernels do not implement raises before any launch -- there is no PyTorch fallback.

The decoder half of the reference key names is taken from the reference's own constructors (`_make_scratch`, `_make_vit_b_rn50_backbone`).
The backbone half (`pretrained.model.patch_embed.backbone.*`, `pretrained.model.blocks.*`) restates timm's naming of `vit_base_resnet50_384`
and is UNVERIFIED: timm was not available when this was written."""
import ctypes
import math
from types import SimpleNamespace

import torch

from . import _lib
from .ops import dt as _dt
from .module_surface import EngineHandle

CONFIG_FIELDS = ('image_size', 'stem_width', 'stage_widths', 'stage_depths', 'num_groups', 'hidden_size', 'num_layers', 'num_heads', 'intermediate_size',
                 'tap_layers', 'neck_channels', 'features', 'num_channels', 'layer_norm_eps', 'readout', 'backbone')
# timm's vit_base_resnet50_384 (ResNetV2-50 stages 3/4/9, 32 groups; ViT-B/16 geometry over the stage-3 map, LayerNorm eps 1e-6) under the reference's
# DPT(features=256, hooks=[0, 1, 8, 11], readout='project') with the three-channel head of lib/apis/adapter3d.py:338
VITB_RN50_384_CONFIG = dict(image_size=384, stem_width=64, stage_widths=(256, 512, 1024), stage_depths=(3, 4, 9), num_groups=32, hidden_size=768, num_layers=12,
                            num_heads=12, intermediate_size=3072, tap_layers=(8, 11), neck_channels=(768, 768), features=256, num_channels=3, layer_norm_eps=1e-6,
                            readout='project', backbone='vitb_rn50_384')
WS_EPS = 1e-8            # the eps of every weight-standardised convolution of the backbone (timm StdConv2dSame(eps=1e-8); transformers passes the same)
TAP_NAMES = ('stem', 'stage1', 'stage2', 'stage3', 'tokens3', 'tokens4', 'fusion4', 'fusion3', 'fusion2', 'fusion1')


def config_from_transformers(cfg):
    """A transformers `DPTConfig` (is_hybrid=True over a `BitConfig`) as the engine's own fields; `num_channels` is the head's (1 there)."""
    get = (lambda o, k, d=None: o.get(k, d)) if isinstance(cfg, dict) else (lambda o, k, d=None: getattr(o, k, d))
    if not get(cfg, 'is_hybrid'):
        raise NotImplementedError('DPT config with is_hybrid=False: the native plan is the hybrid (ResNetV2 + ViT) backbone only')
    bc = get(cfg, 'backbone_config')
    bget = (lambda k, d=None: bc.get(k, d)) if isinstance(bc, dict) else (lambda k, d=None: getattr(bc, k, d))
    if bget('layer_type') != 'bottleneck' or str(bget('global_padding')).lower() != 'same':
        raise NotImplementedError("DPT backbone: the native plan is BiT with layer_type='bottleneck' and global_padding='same'")
    image = get(cfg, 'image_size')
    image = image[0] if isinstance(image, (tuple, list)) else image
    if get(cfg, 'hidden_act') != 'gelu' or get(cfg, 'patch_size') != 16:
        raise NotImplementedError('DPT config: the native plan is hidden_act gelu, patch_size 16')
    if list(get(cfg, 'reassemble_factors'))[2:] != [1, 0.5] or list(get(cfg, 'neck_ignore_stages')) != [0, 1]:
        raise NotImplementedError('DPT config: the native plan is reassemble_factors [.., .., 1, 0.5] with neck_ignore_stages [0, 1]')
    nh = list(get(cfg, 'neck_hidden_sizes'))
    return dict(image_size=int(image), stem_width=int(bget('embedding_size')), stage_widths=tuple(bget('hidden_sizes'))[:3], stage_depths=tuple(bget('depths'))[:3],
                num_groups=int(bget('num_groups')), hidden_size=int(get(cfg, 'hidden_size')), num_layers=int(get(cfg, 'num_hidden_layers')),
                num_heads=int(get(cfg, 'num_attention_heads')), intermediate_size=int(get(cfg, 'intermediate_size')),
                tap_layers=tuple(get(cfg, 'backbone_out_indices'))[2:], neck_channels=(nh[2], nh[3]), features=int(get(cfg, 'fusion_hidden_size')), num_channels=1,
                layer_norm_eps=float(get(cfg, 'layer_norm_eps')), readout=get(cfg, 'readout_type'), backbone='vitb_rn50_384')


def _config_dict(config):
    if not isinstance(config, dict) and hasattr(config, 'is_hybrid'):
        return config_from_transformers(config)
    get = (lambda k: config.get(k)) if isinstance(config, dict) else (lambda k: getattr(config, k, None))
    cfg = {}
    for k in CONFIG_FIELDS:
        v = get(k)
        if v is None:
            if k not in ('readout', 'backbone', 'layer_norm_eps'):
                raise ValueError(f'DPT config: field {k} is missing')
            v = VITB_RN50_384_CONFIG[k]
        cfg[k] = v
    for k, n in (('stage_widths', 3), ('stage_depths', 3), ('tap_layers', 2), ('neck_channels', 2)):
        cfg[k] = tuple(int(v) for v in cfg[k])
        if len(cfg[k]) != n:
            raise ValueError(f'DPT config: {k} needs {n} entries, got {cfg[k]}')
    return cfg


def standardize_weight(w, eps=WS_EPS):
    """The weight a weight-standardised convolution convolves with (timm `StdConv2dSame.forward`, transformers `WeightStandardizedConv2d.forward`:
    `F.batch_norm(w.reshape(1, Cout, -1), None, None, training=True, momentum=0, eps=eps)`): per output channel (w - mean) / sqrt(biased var + eps),
    in float64."""
    w = w.detach().double()
    flat = w.reshape(w.shape[0], -1)
    mean = flat.mean(dim=1, keepdim=True)
    var = flat.var(dim=1, unbiased=False, keepdim=True)
    return ((flat - mean) / torch.sqrt(var + eps)).reshape(w.shape)


def conv_k_order(w):
    """[O, I, 3, 3] -> the K order mve_conv3x3 reads: [O][I/64][3][3][64] when I is a multiple of 64 (MVE_CONV_W_CHUNK64), else [O][3][3][I]."""
    O, I = w.shape[:2]
    if I % 64 == 0:
        return w.reshape(O, I // 64, 64, 3, 3).permute(0, 1, 3, 4, 2).contiguous()
    return w.permute(0, 2, 3, 1).contiguous()


# ---- the key table ----------------------------------------------------------------------------------------------------------------------------------
def key_table(cfg, layout):
    """logical parameter name -> checkpoint key, for `layout` 'reference' (the checkpoint the runner loads) or 'transformers'.  A logical name that
    starts with '_' is accepted and dropped: it exists in the checkpoint but never reaches the prediction (the backbone's final LayerNorm, the ViT
    blocks behind the last tap, refinenet4's resConfUnit1 -- that block has one input).  Names ending in '?' are optional (timm's classifier head)."""
    ref = layout == 'reference'
    if layout not in ('reference', 'transformers'):
        raise ValueError(f'layout {layout!r}: reference | transformers')
    t = {}

    def put(logical, key, suffixes=('weight', 'bias')):
        for s in suffixes:
            t[f'{logical}.{s}'] = f'{key}.{s}'

    bb = 'pretrained.model.patch_embed.backbone' if ref else 'dpt.embeddings.backbone.bit'
    put('stem.conv', f'{bb}.stem.conv' if ref else f'{bb}.embedder.convolution', ('weight',))
    put('stem.norm', f'{bb}.stem.norm' if ref else f'{bb}.embedder.norm')
    for s in range(3):
        for m in range(cfg['stage_depths'][s]):
            blk = f'{bb}.stages.{s}.blocks.{m}' if ref else f'{bb}.encoder.stages.{s}.layers.{m}'
            for i in (1, 2, 3):
                put(f's{s}.b{m}.conv{i}', f'{blk}.conv{i}', ('weight',))
                put(f's{s}.b{m}.norm{i}', f'{blk}.norm{i}')
            if m == 0:
                put(f's{s}.b{m}.downsample.conv', f'{blk}.downsample.conv', ('weight',))
                put(f's{s}.b{m}.downsample.norm', f'{blk}.downsample.norm')
    put('proj', 'pretrained.model.patch_embed.proj' if ref else 'dpt.embeddings.projection')
    t['cls'] = 'pretrained.model.cls_token' if ref else 'dpt.embeddings.cls_token'
    t['pos'] = 'pretrained.model.pos_embed' if ref else 'dpt.embeddings.position_embeddings'
    last = cfg['tap_layers'][1]
    for k in range(cfg['num_layers']):
        p = f'l{k}' if k <= last else f'_l{k}'
        if ref:
            b = f'pretrained.model.blocks.{k}'
            for logical, key in (('norm1', 'norm1'), ('qkv', 'attn.qkv'), ('o', 'attn.proj'), ('norm2', 'norm2'), ('fc1', 'mlp.fc1'), ('fc2', 'mlp.fc2')):
                put(f'{p}.{logical}', f'{b}.{key}')
        else:
            b = f'dpt.encoder.layer.{k}'
            for logical, key in (('norm1', 'layernorm_before'), ('q', 'attention.attention.query'), ('k', 'attention.attention.key'),
                                 ('v', 'attention.attention.value'), ('o', 'attention.output.dense'), ('norm2', 'layernorm_after'),
                                 ('fc1', 'intermediate.dense'), ('fc2', 'output.dense')):
                put(f'{p}.{logical}', f'{b}.{key}')
    put('_final_norm', 'pretrained.model.norm' if ref else 'dpt.layernorm')
    if ref:
        put('_classifier?', 'pretrained.model.head')
    for n, i in ((3, 2), (4, 3)):
        put(f'r{n}.readout', f'pretrained.act_postprocess{n}.0.project.0' if ref else f'neck.reassemble_stage.readout_projects.{i}.0')
        put(f'r{n}.p', f'pretrained.act_postprocess{n}.3' if ref else f'neck.reassemble_stage.layers.{i}.projection')
    put('r4.z', 'pretrained.act_postprocess4.4' if ref else 'neck.reassemble_stage.layers.3.resize')
    for n in (1, 2, 3, 4):
        put(f'rn{n}', f'scratch.layer{n}_rn' if ref else f'neck.convs.{n - 1}', ('weight',))
        f = f'scratch.refinenet{n}' if ref else f'neck.fusion_stage.layers.{4 - n}'
        for ui in (1, 2):
            u = f'{f}.resConfUnit{ui}' if ref else f'{f}.residual_layer{ui}'
            p = f'_f{n}.u{ui}' if (n == 4 and ui == 1) else f'f{n}.u{ui}'
            put(f'{p}.c1', f'{u}.conv1' if ref else f'{u}.convolution1')
            put(f'{p}.c2', f'{u}.conv2' if ref else f'{u}.convolution2')
        put(f'f{n}.out', f'{f}.out_conv' if ref else f'{f}.projection')
    for i in (0, 2, 4):
        put(f'h{i}', f'scratch.output_conv.{i}' if ref else f'head.head.{i}')
    return t


def detect_layout(state_dict):
    return 'transformers' if any(k.startswith(('dpt.', 'neck.')) for k in state_dict) else 'reference'


def match_state_dict(cfg, state_dict, layout=None):
    """-> {logical name: tensor} with every key of `state_dict` consumed exactly once; a missing or unused key is named in a KeyError."""
    layout = layout or detect_layout(state_dict)
    table = key_table(cfg, layout)
    out, used = {}, set()
    for logical, key in table.items():
        optional = '?' in logical
        if key not in state_dict:
            if optional:
                continue
            raise KeyError(f'DPT parameter {key} is missing from the state dict ({layout} layout)')
        used.add(key)
        if not logical.startswith('_'):
            out[logical] = state_dict[key]
    unused = [k for k in state_dict if k not in used]
    if unused:
        raise KeyError(f'state dict key {unused[0]} is not a parameter of this DPT model ({layout} layout; {len(unused)} unused)')
    return out


def pack_slots(cfg, params):
    """{logical name: tensor} -> {engine slot name: float32 / float64 tensor of the slot's size} (include/mvedit_amd.h: mve_dpt_create)."""
    C, nc = cfg['hidden_size'], cfg['num_channels']
    g = lambda n: params[n].detach()
    s = {}

    def norm(slot, logical):
        s[slot + '.g'], s[slot + '.b'] = g(logical + '.weight'), g(logical + '.bias')

    w = standardize_weight(g('stem.conv.weight')).reshape(cfg['stem_width'], 147)
    s['stem.w'] = torch.nn.functional.pad(w, (0, 5))
    norm('stem', 'stem.norm')
    for st in range(3):
        for m in range(cfg['stage_depths'][st]):
            b = f's{st}.b{m}'
            s[b + '.c1.w'] = standardize_weight(g(b + '.conv1.weight')).flatten(1)
            s[b + '.c2.w'] = conv_k_order(standardize_weight(g(b + '.conv2.weight')))
            s[b + '.c3.w'] = standardize_weight(g(b + '.conv3.weight')).flatten(1)
            for i in (1, 2, 3):
                norm(f'{b}.n{i}', f'{b}.norm{i}')
            if m == 0:
                s[b + '.ds.w'] = standardize_weight(g(b + '.downsample.conv.weight')).flatten(1)
                norm(b + '.dn', b + '.downsample.norm')
    s['proj.w'], s['proj.b'] = g('proj.weight').flatten(1), g('proj.bias')
    s['cls'], s['pos'] = g('cls').reshape(-1), g('pos').reshape(-1, C)
    for k in range(cfg['tap_layers'][1] + 1):
        p = f'l{k}'
        norm(p + '.n1', p + '.norm1')
        norm(p + '.n2', p + '.norm2')
        if p + '.qkv.weight' in params:
            s[p + '.qkv.w'], s[p + '.qkv.b'] = g(p + '.qkv.weight'), g(p + '.qkv.bias')
        else:
            s[p + '.qkv.w'] = torch.cat([g(f'{p}.{n}.weight') for n in 'qkv'], 0)
            s[p + '.qkv.b'] = torch.cat([g(f'{p}.{n}.bias') for n in 'qkv'], 0)
        for n in ('o', 'fc1', 'fc2'):
            s[f'{p}.{n}.w'], s[f'{p}.{n}.b'] = g(f'{p}.{n}.weight'), g(f'{p}.{n}.bias')
    for r in ('r3', 'r4'):
        w = g(r + '.readout.weight')                       # Linear(2C, C) over cat(token, cls): columns [0, C) the token's, [C, 2C) the class token's
        s[r + '.wt'], s[r + '.wc'], s[r + '.b'] = w[:, :C], w[:, C:], g(r + '.readout.bias')
        s[r + '.p.w'], s[r + '.p.b'] = g(r + '.p.weight').flatten(1), g(r + '.p.bias')
    s['r4.z.w'], s['r4.z.b'] = conv_k_order(g('r4.z.weight')), g('r4.z.bias')
    for n in (1, 2, 3, 4):
        s[f'rn{n}.w'] = conv_k_order(g(f'rn{n}.weight'))
        for ui in ((2,) if n == 4 else (1, 2)):
            for ci in (1, 2):
                s[f'f{n}.u{ui}.c{ci}.w'], s[f'f{n}.u{ui}.c{ci}.b'] = conv_k_order(g(f'f{n}.u{ui}.c{ci}.weight')), g(f'f{n}.u{ui}.c{ci}.bias')
        s[f'f{n}.out.w'], s[f'f{n}.out.b'] = g(f'f{n}.out.weight').flatten(1), g(f'f{n}.out.bias')
    for i in (0, 2):
        s[f'h{i}.w'], s[f'h{i}.b'] = conv_k_order(g(f'h{i}.weight')), g(f'h{i}.bias')
    s['h4.w'] = torch.nn.functional.pad(g('h4.weight').flatten(1), (0, 0, 0, 8 - nc))          # rows >= num_channels zero: the GEMM wants N % 8 == 0
    s['h4.b'] = torch.nn.functional.pad(g('h4.bias'), (0, 8 - nc))
    return s


def reference_module_config(m):
    """The engine config of a loaded reference `DPTDepthModel` / `DPT` (vitb_rn50_384): read off its modules, nothing assumed but head_dim 64."""
    vit = m.pretrained.model
    if not hasattr(vit.patch_embed, 'backbone'):
        raise NotImplementedError('DPT backbone without a ResNetV2 stem: the native plan is the hybrid vitb_rn50_384 only')
    bb = vit.patch_embed.backbone
    ro = m.pretrained.act_postprocess3[0]
    if type(ro).__name__ != 'ProjectReadout':
        raise NotImplementedError(f"readout {type(ro).__name__}: the native plan is readout='project'")
    taps = tuple(i for i, b in enumerate(vit.blocks) if len(b._forward_hooks))
    C = vit.cls_token.shape[-1]
    G = int(round(math.sqrt(vit.pos_embed.shape[1] - 1)))
    stages = list(bb.stages)
    return dict(image_size=16 * G, stem_width=bb.stem.conv.weight.shape[0], stage_widths=tuple(s.blocks[0].conv3.weight.shape[0] for s in stages),
                stage_depths=tuple(len(s.blocks) for s in stages), num_groups=bb.stem.norm.num_groups, hidden_size=C, num_layers=len(vit.blocks),
                num_heads=C // 64, intermediate_size=vit.blocks[0].mlp.fc1.weight.shape[0], tap_layers=taps,
                neck_channels=(m.pretrained.act_postprocess3[3].weight.shape[0], m.pretrained.act_postprocess4[3].weight.shape[0]),
                features=m.scratch.layer1_rn.weight.shape[0], num_channels=m.scratch.output_conv[4].weight.shape[0],
                layer_norm_eps=float(vit.blocks[0].norm1.eps), readout='project', backbone='vitb_rn50_384')


class DPTNormalEngine(EngineHandle):
    """`DPTDepthModel(backbone='vitb_rn50_384', num_channels=N)` on the native executor: [B, 3, S, S] -> [B, N, S, S] (dimension 1 squeezed when N == 1)."""

    def __init__(self, config=None, dtype=torch.float16, device='cuda'):
        assert dtype in (torch.float16, torch.bfloat16)
        self.cfg = c = _config_dict(VITB_RN50_384_CONFIG if config is None else config)
        if c['readout'] != 'project':
            raise NotImplementedError(f"readout {c['readout']!r}: the native plan is readout='project' (the hybrid's)")
        if c['backbone'] != 'vitb_rn50_384':
            raise NotImplementedError(f"backbone {c['backbone']!r}: the native plan is the hybrid vitb_rn50_384 only")
        if c['hidden_size'] != 64 * c['num_heads']:
            raise NotImplementedError(f"hidden_size {c['hidden_size']} / num_heads {c['num_heads']}: the native attention of this plan has head_dim 64")
        if c['image_size'] % 32:
            raise ValueError(f"image_size {c['image_size']} must be a multiple of 32")
        self.config = SimpleNamespace(**c)
        self.dtype, self.device = dtype, torch.device(device)
        self._h = ctypes.c_void_p()
        i3, i2 = ctypes.c_int * 3, ctypes.c_int * 2
        _lib.call('mve_dpt_create', ctypes.byref(self._h), _dt(dtype), int(c['image_size']), int(c['stem_width']), i3(*c['stage_widths']), i3(*c['stage_depths']),
                  int(c['num_groups']), int(c['hidden_size']), int(c['num_layers']), int(c['num_heads']), int(c['intermediate_size']), i2(*c['tap_layers']),
                  i2(*c['neck_channels']), int(c['features']), int(c['num_channels']), float(c['layer_norm_eps']))
        self.num_tokens = (c['image_size'] // 16) ** 2 + 1
        self._ws = None

    @classmethod
    def from_module(cls, m, dtype=None, device=None):
        """From a loaded reference `DPTDepthModel` or a transformers `DPTForDepthEstimation`: its geometry, state dict, dtype and device.  A module
        whose parameters sit on the CPU gives a plan-only engine (nothing is packed without an accelerator)."""
        p = next(iter(m.parameters()))
        dtype = dtype or (p.dtype if p.dtype in (torch.float16, torch.bfloat16) else torch.float16)
        device = torch.device(device) if device is not None else p.device
        if hasattr(m, 'config') and hasattr(m.config, 'is_hybrid'):
            cfg = config_from_transformers(m.config)
            cfg['num_channels'] = m.head.head[4].weight.shape[0]
        elif hasattr(m, 'pretrained') and hasattr(m, 'scratch'):
            cfg = reference_module_config(m)
        else:
            raise TypeError(f'{type(m).__name__} is neither the reference DPT / DPTDepthModel nor a transformers DPTForDepthEstimation')
        eng = cls(cfg, dtype=dtype, device=device)
        if device.type != 'cpu':
            eng.load_state_dict(m.state_dict())
        return eng

    def load_state_dict(self, state_dict, strict=True, layout=None):
        if not strict:
            raise NotImplementedError('DPTNormalEngine.load_state_dict(strict=False): every key is consumed exactly once')
        slots = pack_slots(self.cfg, match_state_dict(self.cfg, state_dict, layout))
        with torch.cuda.device(self.device):
            s = _lib.stream_ptr(self.device)
            keep = []
            for name, t in slots.items():
                keep.append(self._push_param(name, t.to(dtype=torch.float32).reshape(-1), s))      # a slot is a flat run of its size (a conv's K order has 5 axes)
            torch.cuda.current_stream(self.device).synchronize()
        missing, first = self._missing_params()
        if missing:
            raise KeyError(f'{missing} DPT slots were not filled (first: {first})')
        return self

    # ---- planning / profiling -----------------------------------------------------------------------------------------------------------
    def plan(self, B):
        ws, n_ops, flops = ctypes.c_size_t(), ctypes.c_int(), (ctypes.c_double * 5)()
        _lib.call('mve_dpt_plan', self._h, int(B), ctypes.byref(ws), ctypes.byref(n_ops), flops)
        return self._plan_result(ws, n_ops, flops)

    def op_table(self):
        return [row[1:] for row in self._op_rows()]

    # ---- forward ------------------------------------------------------------------------------------------------------------------------
    def _check_input(self, x):
        if x is None or not torch.is_tensor(x) or x.dim() != 4 or x.shape[0] == 0 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise ValueError(f'input: shape {None if x is None or not torch.is_tensor(x) else tuple(x.shape)} is not [B, 3, S, S]')
        S = int(x.shape[2])
        if S % 32:
            raise ValueError(f'input: S = {S} is not a multiple of 32 (input [B, 3, S, S])')
        if not x.is_floating_point():
            raise ValueError(f'input: dtype {x.dtype} is not a floating-point type')
        if S != self.cfg['image_size']:
            raise NotImplementedError(f"input: S = {S} gives a {S // 16} x {S // 16} token grid, the position table is for {self.cfg['image_size'] // 16} x "
                                      f"{self.cfg['image_size'] // 16}: resampling the table (the reference's _resize_pos_embed) is not implemented")
        return x

    def _tap_shapes(self, B):
        c = self.cfg
        S, C, F, T = c['image_size'], c['hidden_size'], c['features'], self.num_tokens
        w = c['stage_widths']
        return [(B, S // 4, S // 4, c['stem_width']), (B, S // 4, S // 4, w[0]), (B, S // 8, S // 8, w[1]), (B, S // 16, S // 16, w[2]), (B, T, C), (B, T, C),
                (B, S // 16, S // 16, F), (B, S // 8, S // 8, F), (B, S // 4, S // 4, F), (B, S // 2, S // 2, F)]

    def run(self, x, output_features=False, profile=False):
        """-> output [B, N, S, S] ([B, S, S] when N == 1); with output_features=True -> (output, {name: tensor}) with the named taps of TAP_NAMES
        (feature maps as NCHW views, the token taps [B, T, C]) plus 'output'; with profile=True the per-op milliseconds are appended."""
        x = self._check_input(x)
        B, S, nc, dev = x.shape[0], self.cfg['image_size'], self.cfg['num_channels'], self.device
        x = x.to(device=dev, dtype=self.dtype).contiguous()
        with torch.cuda.device(dev):
            info = self.plan(B)
            ws = self._workspace(info['workspace_bytes'])
            out = torch.empty(B, nc, S, S, dtype=self.dtype, device=dev)
            taps = [torch.empty(s, dtype=self.dtype, device=dev) for s in self._tap_shapes(B)] if output_features else None
            tp = (ctypes.c_void_p * len(TAP_NAMES))(*[t.data_ptr() for t in taps]) if taps else None
            op_ms = (ctypes.c_float * info['n_ops'])() if profile else None
            _lib.call('mve_dpt_forward', self._h, _lib.ptr(x), B, _lib.ptr(out), tp, _lib.ptr(ws), ws.numel(), op_ms, _lib.stream_ptr(dev))
        out = out.squeeze(1) if nc == 1 else out              # DPTDepthModel.forward: `.squeeze(dim=1)`
        res = out
        if output_features:
            feats = {n: (t if t.dim() == 3 else t.permute(0, 3, 1, 2)) for n, t in zip(TAP_NAMES, taps)}
            feats['output'] = out
            res = (out, feats)
        if profile:
            res = (res if isinstance(res, tuple) else (res,)) + (list(op_ms),)
        return res

    def __call__(self, x):
        return self.run(x)

    forward = __call__
