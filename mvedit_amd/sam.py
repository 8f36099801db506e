"""Host-side mirror of Segment Anything's image encoder (segment_anything `ImageEncoderViT`; the same arithmetic as transformers'
`SamVisionEncoder`) on the native executor (csrc/unet.hip in SAM mode, csrc/builder_sam.h, csrc/sam.hip):

    SamPredictor.set_image -> self.model.image_encoder(input_image)          (lib/apis/adapter3d.py:363-372, :723-734; lib/pipelines/utils.py:114-131)

The engine stands where `predictor.model.image_encoder` stands: `__call__(x)` takes the preprocessed [B, 3, S, S] image and returns the
[B, 256, G, G] embedding, and `.img_size` is there because `Sam.preprocess` and `SamPredictor.__init__` read it.  The prompt encoder, the two-way
mask decoder and the mask post-processing are NOT here: they stay the torch modules they are (about 4 M parameters over a handful of prompt tokens).

State dicts load under either key layout -- segment_anything's (`patch_embed.proj`, `blocks.N.norm1 / norm2`, `blocks.N.attn.*`,
`blocks.N.mlp.lin1 / lin2`, `neck.0..3`) or transformers' (`patch_embed.projection`, `layers.N.layer_norm1 / layer_norm2`, `neck.conv1 /
layer_norm1 / conv2 / layer_norm2`), with an `image_encoder.` / `vision_encoder.` prefix stripped.  Neither package is imported here.  What the
kernels do not implement (attention maps, training, relative-position tables that would need interpolation, other image sizes) raises -- there
is no PyTorch fallback.

Unverified here, because neither the package nor the checkpoint is at hand: the real `sam_vit_h_4b8939.pth`, segment_anything's key names (restated
from its source as published), and a run of `SamPredictor.set_image` itself over the engine."""
import ctypes
import re
from types import SimpleNamespace

import torch

from . import _lib
from .ops import dt as _dt
from .module_surface import EngineHandle

CONFIG_FIELDS = ('hidden_size', 'num_hidden_layers', 'num_attention_heads', 'image_size', 'patch_size', 'mlp_dim', 'window_size', 'global_attn_indexes',
                 'output_channels', 'layer_norm_eps', 'hidden_act', 'qkv_bias', 'use_rel_pos', 'use_abs_pos', 'num_channels')
CONFIG_DEFAULTS = dict(image_size=1024, patch_size=16, window_size=14, output_channels=256, layer_norm_eps=1e-6, hidden_act='gelu', qkv_bias=True,
                       use_rel_pos=True, use_abs_pos=True, num_channels=3, mlp_dim=None)
# segment_anything's build_sam_vit_h / _l / _b (the reference loads `sam_vit_h_4b8939.pth`)
SAM_VIT_H_CONFIG = dict(CONFIG_DEFAULTS, hidden_size=1280, num_hidden_layers=32, num_attention_heads=16, mlp_dim=5120, global_attn_indexes=(7, 15, 23, 31))
SAM_VIT_L_CONFIG = dict(CONFIG_DEFAULTS, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, mlp_dim=4096, global_attn_indexes=(5, 11, 17, 23))
SAM_VIT_B_CONFIG = dict(CONFIG_DEFAULTS, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, mlp_dim=3072, global_attn_indexes=(2, 5, 8, 11))

PREFIXES = ('vision_encoder.', 'image_encoder.')
_SA_NECK = {'0': 'conv1', '1': 'layer_norm1', '2': 'conv2', '3': 'layer_norm2'}
_SA_BLOCK = {'norm1': 'layer_norm1', 'norm2': 'layer_norm2'}


def transformers_key(key):
    """A state-dict key of either layout -> the engine's (transformers') name.  Keys of neither layout come back unchanged (the loader then
    refuses them by name)."""
    for p in PREFIXES:
        if key.startswith(p):
            key = key[len(p):]
            break
    if key.startswith('patch_embed.proj.'):
        return 'patch_embed.projection.' + key[len('patch_embed.proj.'):]
    m = re.match(r'blocks\.(\d+)\.(.+)$', key)
    if m:
        head, _, tail = m.group(2).partition('.')
        return f'layers.{m.group(1)}.' + _SA_BLOCK.get(head, head) + (('.' + tail) if tail else '')
    m = re.match(r'neck\.([0-3])\.(.+)$', key)
    if m:
        return f'neck.{_SA_NECK[m.group(1)]}.{m.group(2)}'
    return key


def _config_dict(config):
    get = (lambda k: config.get(k)) if isinstance(config, dict) else (lambda k: getattr(config, k, None))
    cfg = {}
    for k in CONFIG_FIELDS:
        v = get(k)
        if v is None:
            if k not in CONFIG_DEFAULTS:
                raise ValueError(f'SAM vision config: field {k} is missing')
            v = CONFIG_DEFAULTS[k]
        cfg[k] = v
    if cfg['mlp_dim'] is None:
        ratio = get('mlp_ratio')
        cfg['mlp_dim'] = int(cfg['hidden_size'] * (4.0 if ratio is None else ratio))
    cfg['global_attn_indexes'] = tuple(int(i) for i in cfg['global_attn_indexes'])
    return cfg


def config_from_image_encoder_vit(m):
    """The configuration of a segment_anything `ImageEncoderViT`, read off the module itself (it keeps no config object)."""
    proj, blocks, neck = m.patch_embed.proj, list(m.blocks), m.neck
    windows = [int(b.window_size) for b in blocks]
    windowed = sorted({w for w in windows if w > 0})
    if len(windowed) > 1:
        raise NotImplementedError(f'ImageEncoderViT with several window sizes {windowed}: the engine takes one')
    return dict(hidden_size=int(proj.out_channels), num_hidden_layers=len(blocks), num_attention_heads=int(blocks[0].attn.num_heads), image_size=int(m.img_size),
                patch_size=int(proj.kernel_size[0]), mlp_dim=int(blocks[0].mlp.lin1.out_features), window_size=windowed[0] if windowed else int(m.img_size) // int(proj.kernel_size[0]),
                global_attn_indexes=tuple(i for i, w in enumerate(windows) if w == 0), output_channels=int(neck[0].out_channels),
                layer_norm_eps=float(blocks[0].norm1.eps), hidden_act='gelu', qkv_bias=blocks[0].attn.qkv.bias is not None,
                use_rel_pos=bool(getattr(blocks[0].attn, 'use_rel_pos', False)), use_abs_pos=getattr(m, 'pos_embed', None) is not None,
                num_channels=int(proj.in_channels))


class SamImageEncoderEngine(EngineHandle):
    """`ImageEncoderViT` / `SamVisionEncoder` on the native executor: [B, 3, S, S] -> [B, output_channels, G, G]."""

    def __init__(self, config, dtype=torch.float16, device='cuda'):
        assert dtype in (torch.float16, torch.bfloat16)
        self.cfg = c = _config_dict(config)
        if c['hidden_act'] != 'gelu':
            raise NotImplementedError(f"hidden_act {c['hidden_act']!r}: SAM's MLP uses the erf GELU")
        if int(c['num_channels']) != 3:
            raise NotImplementedError(f"num_channels {c['num_channels']}: the native patch embedding takes 3 channels")
        if not c['qkv_bias']:
            raise NotImplementedError('qkv_bias=False: the qkv GEMM of the plan carries a bias')
        if not c['use_rel_pos'] or not c['use_abs_pos']:
            raise NotImplementedError('use_rel_pos=False / use_abs_pos=False: the plan always adds pos_embed and the decomposed relative-position bias')
        self.config = config if not isinstance(config, dict) else SimpleNamespace(**c)
        self.dtype, self.device = dtype, torch.device(device)
        self._h = ctypes.c_void_p()
        g = c['global_attn_indexes']
        _lib.call('mve_sam_encoder_create', ctypes.byref(self._h), _dt(dtype), int(c['image_size']), int(c['patch_size']), int(c['hidden_size']),
                  int(c['num_hidden_layers']), int(c['num_attention_heads']), int(c['mlp_dim']), int(c['window_size']), (ctypes.c_int * max(len(g), 1))(*g), len(g),
                  int(c['output_channels']), float(c['layer_norm_eps']), 1, 1)
        self.grid = int(c['image_size']) // int(c['patch_size'])
        self._ws = None

    @property
    def img_size(self):
        """`ImageEncoderViT.img_size`: read by `Sam.preprocess` and `SamPredictor.__init__`."""
        return int(self.cfg['image_size'])

    @classmethod
    def from_module(cls, m, dtype=None, device=None):
        """From a loaded segment_anything `ImageEncoderViT` (recognised by `patch_embed.proj` and `blocks`) or transformers `SamVisionEncoder` /
        `SamVisionModel` (their config).  A module whose parameters sit on the CPU gives a plan-only engine."""
        p = next(iter(m.parameters()))
        dtype = dtype or (p.dtype if p.dtype in (torch.float16, torch.bfloat16) else torch.float16)
        device = torch.device(device) if device is not None else p.device
        if hasattr(m, 'blocks') and hasattr(getattr(m, 'patch_embed', None), 'proj'):
            config = config_from_image_encoder_vit(m)
        elif hasattr(m, 'config'):
            config = getattr(m.config, 'vision_config', m.config)
        else:
            raise TypeError(f'{type(m).__name__} is neither an ImageEncoderViT nor a SamVisionEncoder / SamVisionModel')
        eng = cls(config, dtype=dtype, device=device)
        if device.type != 'cpu':
            eng.load_state_dict(m.state_dict())
        return eng

    @classmethod
    def from_state_dict(cls, state_dict, config, dtype=torch.float16, device='cuda'):
        return cls(config, dtype, device).load_state_dict(state_dict)

    def _table_rows(self, k):
        n = self.grid if k in self.cfg['global_attn_indexes'] else int(self.cfg['window_size'])
        return 2 * n - 1

    def expected_parameters(self):
        names = ['patch_embed.projection.weight', 'patch_embed.projection.bias', 'pos_embed']
        for k in range(int(self.cfg['num_hidden_layers'])):
            b = f'layers.{k}.'
            names += [b + n + s for n in ('layer_norm1', 'attn.qkv', 'attn.proj', 'layer_norm2', 'mlp.lin1', 'mlp.lin2') for s in ('.weight', '.bias')]
            names += [b + 'attn.rel_pos_h', b + 'attn.rel_pos_w']
        names += ['neck.conv1.weight', 'neck.layer_norm1.weight', 'neck.layer_norm1.bias', 'neck.conv2.weight', 'neck.layer_norm2.weight', 'neck.layer_norm2.bias']
        return names

    def map_state_dict(self, state_dict):
        """-> {engine name: tensor}; every key is consumed exactly once: a key of neither layout, or two keys with the same destination, raise."""
        own, out = set(self.expected_parameters()), {}
        for key, t in state_dict.items():
            name = transformers_key(key)
            if name not in own:
                raise KeyError(f'SAM image encoder: state-dict key {key!r} (-> {name!r}) is not a parameter of this configuration')
            if name in out:
                raise KeyError(f'SAM image encoder: state-dict key {key!r} maps to {name!r}, which another key already filled')
            out[name] = t
        for k in range(int(self.cfg['num_hidden_layers'])):
            for n in ('rel_pos_h', 'rel_pos_w'):
                t = out.get(f'layers.{k}.attn.{n}')
                if t is not None and t.shape[0] != self._table_rows(k):
                    raise ValueError(f'layers.{k}.attn.{n}: {t.shape[0]} rows, the block needs {self._table_rows(k)} (2n - 1); a table of another length would '
                                     f'need the linear interpolation of get_rel_pos, which is not implemented')
        return out

    def load_state_dict(self, state_dict, strict=True):
        mapped = self.map_state_dict(state_dict)
        if strict:
            for n in self.expected_parameters():
                if n not in mapped:
                    raise KeyError(f'SAM image encoder parameter {n} is missing from the state dict')
        with torch.cuda.device(self.device):
            s = _lib.stream_ptr(self.device)
            for name, t in mapped.items():
                self._push_param(name, t, s)
            torch.cuda.current_stream(self.device).synchronize()
        missing, first = self._missing_params()
        if strict and missing:
            raise KeyError(f'{missing} SAM image encoder parameters missing from the state dict (first: {first})')
        return self

    # ---- planning / profiling -----------------------------------------------------------------------------------------------------------
    def plan(self, B):
        ws, n_ops, flops = ctypes.c_size_t(), ctypes.c_int(), (ctypes.c_double * 5)()
        _lib.call('mve_sam_encoder_plan', self._h, int(B), ctypes.byref(ws), ctypes.byref(n_ops), flops)
        return self._plan_result(ws, n_ops, flops)

    def op_table(self):
        return [row[1:] for row in self._op_rows()]

    # ---- forward ------------------------------------------------------------------------------------------------------------------------
    def _check_pixels(self, x):
        S = self.img_size
        if not torch.is_tensor(x) or x.dim() != 4 or tuple(x.shape[1:]) != (3, S, S) or x.shape[0] == 0:
            shape = tuple(x.shape) if torch.is_tensor(x) else type(x).__name__
            raise ValueError(f'image: shape {shape} is not [B, 3, {S}, {S}] (img_size {S}; Sam.preprocess pads to it)')
        if not x.is_floating_point():
            raise ValueError(f'image: dtype {x.dtype} is not a floating-point type')
        return x

    def run(self, x, output_hidden_states=False, profile=False):
        """-> (embedding [B, O, G, G], hidden_states | None[, per-op ms]); hidden_states: num_hidden_layers + 1 tensors [B, G, G, C], entry 0 the
        patch embedding plus pos_embed, entry k + 1 the output of block k."""
        x = self._check_pixels(x)
        B, c, dev, G = x.shape[0], self.cfg, self.device, self.grid
        C, O, n_hidden = int(c['hidden_size']), int(c['output_channels']), int(c['num_hidden_layers']) + 1
        x = x.to(device=dev, dtype=self.dtype).contiguous()
        with torch.cuda.device(dev):
            info = self.plan(B)
            ws = self._workspace(info['workspace_bytes'])
            out = torch.empty(B, O, G, G, dtype=self.dtype, device=dev)
            hidden = tuple(torch.empty(B, G, G, C, dtype=self.dtype, device=dev) for _ in range(n_hidden)) if output_hidden_states else None
            hs = (ctypes.c_void_p * n_hidden)(*[h.data_ptr() for h in hidden]) if hidden else None
            op_ms = (ctypes.c_float * info['n_ops'])() if profile else None
            _lib.call('mve_sam_encoder_forward', self._h, _lib.ptr(x), B, _lib.ptr(out), hs, _lib.ptr(ws), ws.numel(), op_ms, _lib.stream_ptr(dev))
        res = (out, hidden)
        return res + (list(op_ms),) if profile else res

    def __call__(self, x, output_attentions=None):
        if output_attentions:
            raise NotImplementedError('output_attentions=True: the attention kernel does not materialise the attention maps')
        return self.run(x)[0]

    forward = __call__

    def train(self, mode=True):
        if mode:
            raise NotImplementedError('SamImageEncoderEngine.train(): the engine is inference only')
        return self
