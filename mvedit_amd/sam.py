"""Host-side mirror of Segment Anything's image encoder (segment_anything `ImageEncoderViT`; the same arithmetic as transformers'
`SamVisionEncoder`) on the native executor (csrc/unet.hip in SAM mode, csrc/builder_sam.h, csrc/sam.hip):

    SamPredictor.set_image -> self.model.image_encoder(input_image)          (lib/apis/adapter3d.py:363-372, :723-734; lib/pipelines/utils.py:114-131)

The engine stands where `predictor.model.image_encoder` stands: `__call__(x)` takes the preprocessed [B, 3, S, S] image and returns the
[B, 256, G, G] embedding, and `.img_size` is there because `Sam.preprocess` and `SamPredictor.__init__` read it.  The prompt encoder, the two-way
mask decoder and the mask post-processing are `SamMaskDecoderEngine` and `SamPredictorEngine` at the end of this file (fp32 kernels, csrc/sam_decoder.hip).

State dicts load under either key layout -- segment_anything's (`patch_embed.proj`, `blocks.N.norm1 / norm2`, `blocks.N.attn.*`,
`blocks.N.mlp.lin1 / lin2`, `neck.0..3`) or transformers' (`patch_embed.projection`, `layers.N.layer_norm1 / layer_norm2`, `neck.conv1 /
layer_norm1 / conv2 / layer_norm2`), with an `image_encoder.` / `vision_encoder.` prefix stripped.  Neither package is imported here.  What the
kernels do not implement (attention maps, training, relative-position tables that would need interpolation, other image sizes) raises -- there
is no PyTorch fallback.

Unverified here, because neither the package nor the checkpoint is at hand: the real `sam_vit_h_4b8939.pth`, segment_anything's key names (restated
from its source as published), and a run of segment_anything's own `SamPredictor` over the engines (`SamPredictorEngine` restates its surface)."""
import ctypes
import re
from types import SimpleNamespace

import numpy as np
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


# =====================================================================================================================================================
# prompt encoder + two-way mask decoder, and the predictor over both engines
# =====================================================================================================================================================
DECODER_CONFIG_FIELDS = ('hidden_size', 'num_hidden_layers', 'num_attention_heads', 'mlp_dim', 'num_multimask_outputs', 'iou_head_depth', 'iou_head_hidden_dim',
                         'attention_downsample_rate', 'layer_norm_eps', 'final_layer_norm_eps', 'image_embedding_size', 'image_size')
# segment_anything's build_sam (every ViT size shares one decoder); eps: nn.LayerNorm's default everywhere in its TwoWayTransformer
SAM_DECODER_CONFIG = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=8, mlp_dim=2048, num_multimask_outputs=3, iou_head_depth=3, iou_head_hidden_dim=256,
                          attention_downsample_rate=2, layer_norm_eps=1e-5, final_layer_norm_eps=1e-5, image_embedding_size=64, image_size=1024)
# transformers' SamMaskDecoderConfig: layer_norm_eps 1e-6 for layer_norm1..4, nn.LayerNorm's 1e-5 for layer_norm_final_attn
TRANSFORMERS_DECODER_CONFIG = dict(SAM_DECODER_CONFIG, layer_norm_eps=1e-6)
MAX_TOKENS = 16
PIXEL_MEAN, PIXEL_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)

_SA_MARKS = ('pe_layer.', 'point_embeddings.', 'mask_downscaling.', 'output_upscaling.', '.norm_final_attn.', '.norm1.', '.norm2.', '.norm3.', '.norm4.')
_SA_UPSCALE = {'0': 'upscale_conv1', '1': 'upscale_layer_norm', '3': 'upscale_conv2'}
_SA_MLP = {'0': 'proj_in', '1': 'layers.0', '2': 'proj_out'}
# accepted by name and not uploaded: the `mask_input` path (refused), and transformers' tied copy of the gaussian matrix
_UNUSED = re.compile(r'prompt_encoder\.(mask_embed|mask_downscaling)\.|prompt_encoder\.shared_embedding\.positional_embedding$')


def is_segment_anything_layout(keys):
    """True when the state dict spells its keys as segment_anything's `Sam` does (restated from its published source; the package is not installed)."""
    return any(m in k for k in keys for m in _SA_MARKS)


def decoder_transformers_key(key, sa_layout):
    """A prompt-encoder / mask-decoder state-dict key -> the engine's (transformers `SamModel`) name.  Unknown keys come back unchanged."""
    if not sa_layout:
        return key
    if key == 'prompt_encoder.pe_layer.positional_encoding_gaussian_matrix':
        return 'shared_image_embedding.positional_embedding'
    key = key.replace('prompt_encoder.point_embeddings.', 'prompt_encoder.point_embed.').replace('.norm_final_attn.', '.layer_norm_final_attn.')
    key = re.sub(r'(transformer\.layers\.\d+)\.norm([1-4])\.', r'\1.layer_norm\2.', key)
    m = re.match(r'mask_decoder\.output_upscaling\.([013])\.(.+)$', key)
    if m:
        return f'mask_decoder.{_SA_UPSCALE[m.group(1)]}.{m.group(2)}'
    m = re.match(r'(mask_decoder\.(?:output_hypernetworks_mlps\.\d+|iou_prediction_head))\.layers\.([012])\.(.+)$', key)
    if m:
        return f'{m.group(1)}.{_SA_MLP[m.group(2)]}.{m.group(3)}'
    return key


def _decoder_config_dict(config):
    if not isinstance(config, dict):      # a transformers SamConfig / SamMaskDecoderConfig (+ the prompt encoder's sizes)
        md = getattr(config, 'mask_decoder_config', config)
        pe = getattr(config, 'prompt_encoder_config', None)
        config = {k: getattr(md, k) for k in DECODER_CONFIG_FIELDS if hasattr(md, k)}
        config.setdefault('final_layer_norm_eps', 1e-5)
        if pe is not None:
            config.update(image_embedding_size=int(pe.image_embedding_size), image_size=int(pe.image_size))
    cfg = {}
    for k in DECODER_CONFIG_FIELDS:
        if k not in config or config[k] is None:
            raise ValueError(f'SAM mask decoder config: field {k} is missing')
        cfg[k] = config[k]
    return cfg


class SamMaskDecoderEngine(EngineHandle):
    """Prompt encoder + two-way mask decoder (`SamPromptEncoder` + `SamMaskDecoder` / `PromptEncoder` + `MaskDecoder`) on the native executor, fp32
    throughout: image embedding [B, C, G, G] + boxes / points -> low-res mask logits [B, P, M, 4G, 4G] and iou predictions [B, P, M]."""

    def __init__(self, config, device='cuda', embedding_dtype=torch.float16):
        assert embedding_dtype in (torch.float16, torch.bfloat16)
        self.cfg = c = _decoder_config_dict(config)
        if int(c['attention_downsample_rate']) != 2:
            raise NotImplementedError(f"attention_downsample_rate {c['attention_downsample_rate']}: the cross-attentions run at half the width (2)")
        if int(c['hidden_size']) != 32 * int(c['num_attention_heads']):
            raise NotImplementedError(f"hidden_size {c['hidden_size']} / heads {c['num_attention_heads']}: the attention kernel takes head dims 32 (self) and 16 (cross)")
        self.dtype, self.embedding_dtype, self.device = torch.float32, embedding_dtype, torch.device(device)
        self.num_mask_tokens = int(c['num_multimask_outputs']) + 1
        self.grid, self.image_size = int(c['image_embedding_size']), int(c['image_size'])
        self._h = ctypes.c_void_p()
        _lib.call('mve_sam_decoder_create', ctypes.byref(self._h), _dt(embedding_dtype), int(c['hidden_size']), int(c['num_hidden_layers']), int(c['num_attention_heads']),
                  int(c['mlp_dim']), self.num_mask_tokens, int(c['iou_head_hidden_dim']), int(c['iou_head_depth']), int(c['attention_downsample_rate']), self.grid,
                  self.image_size, float(c['layer_norm_eps']), float(c['final_layer_norm_eps']))
        self._ws = None

    # ---- construction ---------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_module(cls, m, device=None, embedding_dtype=torch.float16):
        """From a loaded segment_anything `Sam` (recognised by `prompt_encoder.pe_layer`) or transformers `SamModel`.  The LayerNorm eps values are
        read off the modules themselves.  A module whose parameters sit on the CPU gives a plan-only engine unless `device` says otherwise."""
        pe, md = getattr(m, 'prompt_encoder', None), getattr(m, 'mask_decoder', None)
        if pe is None or md is None:
            raise TypeError(f'{type(m).__name__} has no prompt_encoder / mask_decoder: neither a Sam nor a SamModel')
        p = next(iter(md.parameters()))
        device = torch.device(device) if device is not None else p.device
        tf = md.transformer
        layer0 = tf.layers[0]
        sa = hasattr(pe, 'pe_layer')
        norm1 = layer0.norm1 if sa else layer0.layer_norm1
        final = tf.norm_final_attn if sa else tf.layer_norm_final_attn
        iou = md.iou_prediction_head
        size = pe.image_embedding_size
        image = pe.input_image_size
        config = dict(hidden_size=int(md.iou_token.weight.shape[1]), num_hidden_layers=len(tf.layers), num_attention_heads=int(layer0.self_attn.num_heads if sa else layer0.self_attn.num_attention_heads),
                      mlp_dim=int(layer0.mlp.lin1.out_features), num_multimask_outputs=int(md.mask_tokens.weight.shape[0]) - 1,
                      iou_head_depth=len(iou.layers) if sa else len(iou.layers) + 2, iou_head_hidden_dim=int((iou.layers[0] if sa else iou.proj_in).out_features),
                      attention_downsample_rate=int(md.iou_token.weight.shape[1]) // int(layer0.cross_attn_token_to_image.q_proj.out_features),
                      layer_norm_eps=float(norm1.eps), final_layer_norm_eps=float(final.eps),
                      image_embedding_size=int(size[0] if isinstance(size, (tuple, list)) else size), image_size=int(image[0] if isinstance(image, (tuple, list)) else image))
        eng = cls(config, device=device, embedding_dtype=embedding_dtype)
        if device.type != 'cpu':
            eng.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith(PREFIXES)})
        return eng

    @classmethod
    def from_state_dict(cls, state_dict, config, device='cuda', embedding_dtype=torch.float16):
        return cls(config, device, embedding_dtype).load_state_dict(state_dict)

    # ---- weights --------------------------------------------------------------------------------------------------------------------------------
    def expected_parameters(self):
        c, wb = self.cfg, ('.weight', '.bias')
        attn = lambda p: [p + j + s for j in ('.q_proj', '.k_proj', '.v_proj', '.out_proj') for s in wb]
        names = ['shared_image_embedding.positional_embedding'] + [f'prompt_encoder.point_embed.{k}.weight' for k in range(4)]
        names += ['prompt_encoder.not_a_point_embed.weight', 'prompt_encoder.no_mask_embed.weight', 'mask_decoder.iou_token.weight', 'mask_decoder.mask_tokens.weight']
        tf = 'mask_decoder.transformer.'
        for k in range(int(c['num_hidden_layers'])):
            b = f'{tf}layers.{k}.'
            names += attn(b + 'self_attn') + attn(b + 'cross_attn_token_to_image') + attn(b + 'cross_attn_image_to_token')
            names += [b + n + s for n in ('layer_norm1', 'layer_norm2', 'layer_norm3', 'layer_norm4', 'mlp.lin1', 'mlp.lin2') for s in wb]
        names += attn(tf + 'final_attn_token_to_image') + [tf + 'layer_norm_final_attn' + s for s in wb]
        names += ['mask_decoder.' + n + s for n in ('upscale_conv1', 'upscale_conv2', 'upscale_layer_norm') for s in wb]
        heads = [f'mask_decoder.output_hypernetworks_mlps.{j}' for j in range(self.num_mask_tokens)] + ['mask_decoder.iou_prediction_head']
        names += [h + n + s for h in heads for n in ('.proj_in', '.layers.0', '.proj_out') for s in wb]
        return names

    def map_state_dict(self, state_dict):
        """-> {engine name: tensor}; every key is consumed exactly once.  A key of neither layout, or two keys with one destination, raise KeyError; the
        `mask_input` path's parameters (`mask_embed.*` / `mask_downscaling.*`) and transformers' tied copy of the gaussian matrix are accepted by name
        and left out."""
        own, out = set(self.expected_parameters()), {}
        sa = is_segment_anything_layout(state_dict.keys())
        for key, t in state_dict.items():
            if _UNUSED.match(key):
                continue
            name = decoder_transformers_key(key, sa)
            if name not in own:
                raise KeyError(f'SAM mask decoder: state-dict key {key!r} (-> {name!r}) is not a parameter of this configuration')
            if name in out:
                raise KeyError(f'SAM mask decoder: state-dict key {key!r} maps to {name!r}, which another key already filled')
            out[name] = t
        return out

    def load_state_dict(self, state_dict, strict=True):
        mapped = self.map_state_dict(state_dict)
        if strict:
            for n in self.expected_parameters():
                if n not in mapped:
                    raise KeyError(f'SAM mask decoder parameter {n} is missing from the state dict')
        with torch.cuda.device(self.device):
            s = _lib.stream_ptr(self.device)
            keep = [self._push_param(name, t, s) for name, t in mapped.items()]
            if not self._missing_params()[0]:
                _lib.call('mve_sam_decoder_finalize', self._h, s)
            torch.cuda.current_stream(self.device).synchronize()
            del keep
        return self

    # ---- planning -------------------------------------------------------------------------------------------------------------------------------
    def n_tokens(self, n_points, has_box):
        return 1 + self.num_mask_tokens + n_points + (1 if n_points and not has_box else 0) + (2 if has_box else 0)

    def plan(self, B=1, P=1, n_points=0, has_box=True):
        ws, n_ops, flops = ctypes.c_size_t(), ctypes.c_int(), (ctypes.c_double * 5)()
        _lib.call('mve_sam_decoder_plan', self._h, int(B), int(P), int(n_points), int(bool(has_box)), ctypes.byref(ws), ctypes.byref(n_ops), flops)
        return self._plan_result(ws, n_ops, flops)

    def op_table(self):
        return [row[1:] for row in self._op_rows()]

    def tap_names(self):
        L = int(self.cfg['num_hidden_layers'])
        return ['tokens'] + [f'{n}.{k}' for k in range(L) for n in ('queries', 'keys')] + ['queries.final', 'upscaled', 'hyper_in', 'dense_pe']

    # ---- forward --------------------------------------------------------------------------------------------------------------------------------
    def check_prompts(self, B, input_boxes, input_points, input_labels):
        """Shapes and labels of one call's prompts, before anything is launched -> (P, n_points, boxes | None, points | None, labels | None) as
        host-or-device fp32 / int32 tensors.  Labels that are on the host are checked against {-1, 0, 1}."""
        if input_boxes is None and input_points is None:
            raise ValueError('SAM mask decoder: no prompt at all (neither input_boxes nor input_points)')
        if (input_points is None) != (input_labels is None):
            raise ValueError('SAM mask decoder: input_points and input_labels come together')
        boxes = points = labels = None
        P = None
        if input_boxes is not None:
            boxes = torch.as_tensor(input_boxes)
            if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 4:
                raise ValueError(f'input_boxes: shape {tuple(boxes.shape)} is not [B = {B}, P, 4] (every image of a call takes the same number of prompts)')
            P = int(boxes.shape[1])
        n_points = 0
        if input_points is not None:
            points, labels = torch.as_tensor(input_points), torch.as_tensor(input_labels)
            if points.dim() != 4 or points.shape[0] != B or points.shape[3] != 2:
                raise ValueError(f'input_points: shape {tuple(points.shape)} is not [B = {B}, P, n_points, 2] (every prompt of a call takes the same number of points)')
            if tuple(labels.shape) != tuple(points.shape[:3]):
                raise ValueError(f'input_labels: shape {tuple(labels.shape)} does not match the points {tuple(points.shape[:3])}')
            if P is not None and int(points.shape[1]) != P:
                raise ValueError(f'prompts of unequal shape within one call: {P} boxes but {int(points.shape[1])} point sets per image')
            P, n_points = int(points.shape[1]), int(points.shape[2])
            if n_points == 0:
                raise ValueError('input_points: zero points per prompt; pass None instead')
            if labels.device.type == 'cpu' and not bool(((labels == -1) | (labels == 0) | (labels == 1)).all()):
                raise ValueError('input_labels: labels outside {-1, 0, 1}')
        if P == 0:
            raise ValueError('SAM mask decoder: zero prompts per image')
        T = self.n_tokens(n_points, boxes is not None)
        if T > MAX_TOKENS:
            raise NotImplementedError(f'{T} tokens per prompt: the kernels take at most {MAX_TOKENS} (iou + {self.num_mask_tokens} mask tokens + points + box corners)')
        return P, n_points, boxes, points, labels

    def run(self, image_embeddings, input_boxes=None, input_points=None, input_labels=None, multimask_output=True, output_taps=False, profile=False):
        """-> (low_res_masks [B, P, M, 4G, 4G] fp32, iou [B, P, M] fp32, taps | None[, per-op ms]); M = num_multimask_outputs with multimask_output, else
        1 (mask token 0).  `taps`: {name: tensor} of tap_names(), plus the unsliced `low_res_masks` / `iou` of all mask tokens."""
        C, G, Mt = int(self.cfg['hidden_size']), self.grid, self.num_mask_tokens
        if not torch.is_tensor(image_embeddings) or image_embeddings.dim() != 4 or tuple(image_embeddings.shape[1:]) != (C, G, G) or image_embeddings.shape[0] == 0:
            shape = tuple(image_embeddings.shape) if torch.is_tensor(image_embeddings) else type(image_embeddings).__name__
            raise ValueError(f'image_embeddings: shape {shape} is not [B, {C}, {G}, {G}]')
        B, dev = int(image_embeddings.shape[0]), self.device
        P, n_points, boxes, points, labels = self.check_prompts(B, input_boxes, input_points, input_labels)
        N, T, L = B * P, self.n_tokens(n_points, boxes is not None), int(self.cfg['num_hidden_layers'])
        emb = image_embeddings.to(device=dev, dtype=self.embedding_dtype).contiguous()
        f32 = lambda t: None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()
        boxes, points = f32(boxes), f32(points)
        labels = None if labels is None else labels.to(device=dev, dtype=torch.int32).contiguous()
        with torch.cuda.device(dev):
            info = self.plan(B, P, n_points, boxes is not None)
            ws = self._workspace(info['workspace_bytes'])
            low = torch.empty(B, P, Mt, 4 * G, 4 * G, dtype=torch.float32, device=dev)
            iou = torch.empty(B, P, Mt, dtype=torch.float32, device=dev)
            taps = tp = None
            if output_taps:
                new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
                shapes = [(N, T, C)] + [s for _ in range(L) for s in ((N, T, C), (N, G * G, C))] + [(N, T, C), (N, 16 * G * G, C // 8), (N, Mt, C // 8), (G * G, C)]
                taps = dict(zip(self.tap_names(), (new(*s) for s in shapes)))
                tp = (ctypes.c_void_p * len(shapes))(*[t.data_ptr() for t in taps.values()])
            op_ms = (ctypes.c_float * info['n_ops'])() if profile else None
            _lib.call('mve_sam_decoder_forward', self._h, _lib.ptr(emb), B, P, _lib.ptr(boxes), _lib.ptr(points), _lib.ptr(labels), n_points, _lib.ptr(low), _lib.ptr(iou), tp,
                      _lib.ptr(ws), ws.numel(), op_ms, _lib.stream_ptr(dev))
        if taps is not None:
            taps.update(low_res_masks=low, iou=iou)
        sl = slice(1, None) if multimask_output else slice(0, 1)
        res = (low[:, :, sl].contiguous(), iou[:, :, sl].contiguous(), taps)
        return res + (list(op_ms),) if profile else res

    def __call__(self, image_embeddings, input_boxes=None, input_points=None, input_labels=None, multimask_output=True):
        return self.run(image_embeddings, input_boxes, input_points, input_labels, multimask_output)[:2]

    forward = __call__

    def train(self, mode=True):
        if mode:
            raise NotImplementedError('SamMaskDecoderEngine.train(): the engine is inference only')
        return self


def preprocess_shape(h, w, long_side):
    """`ResizeLongestSide.get_preprocess_shape`: the size whose longest side is `long_side`, each side int(side * scale + 0.5)."""
    scale = long_side * 1.0 / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


def preprocess_image(image_u8, long_side, dtype, pixel_mean=None, pixel_std=None):
    """uint8 [h, w, 3] on the device, longest side already `long_side` -> the encoder's [1, 3, S, S] (mve_sam_preprocess: normalise, then zero-pad)."""
    h, w = int(image_u8.shape[0]), int(image_u8.shape[1])
    if image_u8.dtype != torch.uint8 or image_u8.dim() != 3 or image_u8.shape[2] != 3 or max(h, w) > long_side:
        raise ValueError(f'image: {image_u8.dtype} {tuple(image_u8.shape)} is not uint8 [h, w, 3] with sides of at most {long_side}')
    image_u8 = image_u8.contiguous()
    out = torch.empty(1, 3, long_side, long_side, dtype=dtype, device=image_u8.device)
    mean = (ctypes.c_float * 3)(*pixel_mean) if pixel_mean is not None else None
    std = (ctypes.c_float * 3)(*pixel_std) if pixel_std is not None else None
    with torch.cuda.device(image_u8.device):
        _lib.call('mve_sam_preprocess', _dt(dtype), _lib.ptr(image_u8), h, w, int(long_side), mean, std, _lib.ptr(out), _lib.stream_ptr(image_u8.device))
    return out


def postprocess_masks(low_res, long_side, input_size, original_size, mask_threshold=0.0, return_logits=False):
    """`Sam.postprocess_masks` + threshold on [..., L, L] fp32 low-res logits -> ([..., H, W] bool masks, fp32 logits | None) (mve_sam_postprocess)."""
    lead, L = tuple(low_res.shape[:-2]), int(low_res.shape[-1])
    (h_in, w_in), (H, W) = input_size, original_size
    low = low_res.to(torch.float32).contiguous()
    planes = int(np.prod(lead)) if lead else 1
    masks = torch.empty(*lead, H, W, dtype=torch.uint8, device=low.device)
    logits = torch.empty(*lead, H, W, dtype=torch.float32, device=low.device) if return_logits else None
    with torch.cuda.device(low.device):
        _lib.call('mve_sam_postprocess', _lib.ptr(low), planes, L, int(long_side), int(h_in), int(w_in), int(H), int(W), float(mask_threshold), _lib.ptr(masks),
                  _lib.ptr(logits), _lib.stream_ptr(low.device))
    return masks.view(torch.bool), logits


class SamPredictorEngine:
    """segment_anything's `SamPredictor` surface over the two engines: `set_image` (host resize, mve_sam_preprocess, the encoder engine) and
    `predict` / `predict_torch` (the decoder engine, mve_sam_postprocess).  `mask_input` is refused: the mask-embedding path is not implemented."""

    def __init__(self, encoder_engine, decoder_engine, mask_threshold=0.0, pixel_mean=None, pixel_std=None, image_format='RGB'):
        if int(encoder_engine.img_size) != int(decoder_engine.image_size) or int(encoder_engine.grid) != int(decoder_engine.grid):
            raise ValueError(f'encoder (image {encoder_engine.img_size}, grid {encoder_engine.grid}) and decoder (image {decoder_engine.image_size}, grid '
                             f'{decoder_engine.grid}) do not fit together')
        if encoder_engine.dtype != decoder_engine.embedding_dtype:
            raise ValueError(f'the encoder writes {encoder_engine.dtype}, the decoder reads {decoder_engine.embedding_dtype}')
        self.encoder, self.decoder = encoder_engine, decoder_engine
        self.mask_threshold = float(mask_threshold)
        self.pixel_mean = tuple(float(v) for v in (pixel_mean if pixel_mean is not None else PIXEL_MEAN))
        self.pixel_std = tuple(float(v) for v in (pixel_std if pixel_std is not None else PIXEL_STD))
        # what the reference reads off `predictor.model`
        self.model = SimpleNamespace(image_encoder=encoder_engine, mask_decoder=decoder_engine, prompt_encoder=decoder_engine, mask_threshold=self.mask_threshold,
                                     image_format=image_format, device=decoder_engine.device)
        self.reset_image()

    @classmethod
    def from_predictor(cls, p):
        """From a loaded segment_anything `SamPredictor` (or anything with its `.model`): the engines are built from `model.image_encoder` (kept when
        it already is an engine) and `model.prompt_encoder` / `model.mask_decoder`."""
        sam = p.model
        enc = sam.image_encoder
        if not isinstance(enc, SamImageEncoderEngine):
            enc = SamImageEncoderEngine.from_module(enc)
        dec = SamMaskDecoderEngine.from_module(sam, device=enc.device, embedding_dtype=enc.dtype)
        flat = lambda t: None if t is None else [float(v) for v in torch.as_tensor(t).reshape(-1)]
        return cls(enc, dec, mask_threshold=float(getattr(sam, 'mask_threshold', 0.0)), pixel_mean=flat(getattr(sam, 'pixel_mean', None)),
                   pixel_std=flat(getattr(sam, 'pixel_std', None)), image_format=getattr(sam, 'image_format', 'RGB'))

    @property
    def device(self):
        return self.decoder.device

    def reset_image(self):
        self.is_image_set = False
        self.features = None
        self.orig_h = self.orig_w = self.input_h = self.input_w = None
        self.original_size = self.input_size = None

    # ---- set_image ------------------------------------------------------------------------------------------------------------------------------
    def set_image(self, image, image_format='RGB'):
        """image: uint8 [H, W, 3] numpy.  Resized on the host to longest side S with PIL's bilinear filter (what `ResizeLongestSide.apply_image` does)."""
        from PIL import Image
        if image_format not in ('RGB', 'BGR'):
            raise ValueError(f"image_format must be in ['RGB', 'BGR'], is {image_format}.")
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError(f'set_image: {image.dtype} {image.shape} is not uint8 [H, W, 3]')
        if image_format != self.model.image_format:
            image = image[..., ::-1]
        H, W = image.shape[:2]
        nh, nw = preprocess_shape(H, W, self.encoder.img_size)
        resized = np.asarray(Image.fromarray(np.ascontiguousarray(image)).resize((nw, nh), Image.BILINEAR))
        self._set_resized(torch.from_numpy(np.ascontiguousarray(resized)).to(self.device), (H, W))

    def set_torch_image(self, transformed_image, original_image_size):
        """transformed_image: [1, 3, h, w] RGB in 0..255 (any dtype), already resized to longest side S, as `ResizeLongestSide` leaves it; it is rounded
        to uint8, which is exact for what `apply_image` produces."""
        S = self.encoder.img_size
        if not torch.is_tensor(transformed_image) or transformed_image.dim() != 4 or transformed_image.shape[0] != 1 or transformed_image.shape[1] != 3 or \
                max(transformed_image.shape[2:]) != S:
            raise ValueError(f'set_torch_image: input must be [1, 3, h, w] with longest side {S}')
        u8 = transformed_image[0].permute(1, 2, 0).to(self.device)
        if u8.dtype != torch.uint8:
            u8 = u8.float().round().clamp(0, 255).to(torch.uint8)
        self._set_resized(u8, tuple(int(v) for v in original_image_size))

    def _set_resized(self, u8, original_size):
        self.reset_image()
        pixels = preprocess_image(u8, self.encoder.img_size, self.encoder.dtype, self.pixel_mean, self.pixel_std)
        self.features = self.encoder(pixels)
        self.original_size, self.input_size = tuple(original_size), (int(u8.shape[0]), int(u8.shape[1]))
        self.orig_h, self.orig_w = self.original_size
        self.input_h, self.input_w = self.input_size
        self.is_image_set = True

    def get_image_embedding(self):
        if not self.is_image_set:
            raise ValueError('An image must be set with .set_image(...) to generate an embedding.')
        return self.features

    # ---- predict --------------------------------------------------------------------------------------------------------------------------------
    def apply_coords(self, coords):
        """`ResizeLongestSide.apply_coords`: [..., 2] (x, y) in original-image pixels -> input-image pixels, in float64 on the host."""
        (H, W), (nh, nw) = self.original_size, self.input_size
        coords = np.array(coords, dtype=np.float64, copy=True)
        coords[..., 0] *= nw / W
        coords[..., 1] *= nh / H
        return coords

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output=True, return_logits=False):
        """numpy in, numpy out, as `SamPredictor.predict`: -> (masks [M, H, W] bool (fp32 logits with return_logits), iou [M], low_res [M, 4G, 4G])."""
        if not self.is_image_set:
            raise ValueError('An image must be set with .set_image(...) before mask prediction.')
        if mask_input is not None:
            raise NotImplementedError('mask_input: the mask-embedding path of the prompt encoder is not implemented')
        if point_coords is None and box is None:
            raise ValueError('predict: no prompt at all (neither points nor a box)')
        pts = lbl = bx = None
        if point_coords is not None:
            if point_labels is None:
                raise ValueError('point_labels must be supplied if point_coords is supplied.')
            point_coords, point_labels = np.asarray(point_coords), np.asarray(point_labels)
            if point_coords.ndim != 2 or point_coords.shape[1] != 2 or point_labels.shape != point_coords.shape[:1]:
                raise ValueError(f'point_coords {point_coords.shape} / point_labels {point_labels.shape} are not [n, 2] / [n]')
            if not np.isin(point_labels, (-1, 0, 1)).all():
                raise ValueError('point_labels: labels outside {-1, 0, 1}')
            pts = torch.from_numpy(self.apply_coords(point_coords)).float()[None]
            lbl = torch.from_numpy(point_labels.astype(np.int32))[None]
        if box is not None:
            box = np.asarray(box)
            if box.size != 4:
                raise ValueError(f'box {box.shape} is not one box of 4 values')
            bx = torch.from_numpy(self.apply_coords(box.reshape(2, 2)).reshape(1, 4)).float()
        masks, iou, low = self.predict_torch(pts, lbl, bx, None, multimask_output, return_logits)
        return masks[0].cpu().numpy(), iou[0].cpu().numpy(), low[0].cpu().numpy()

    def predict_torch(self, point_coords=None, point_labels=None, boxes=None, mask_input=None, multimask_output=True, return_logits=False):
        """Prompts already in input-image pixels: point_coords [P, n, 2], point_labels [P, n], boxes [P, 4] -> (masks [P, M, H, W], iou [P, M],
        low_res [P, M, 4G, 4G]) on the device."""
        if not self.is_image_set:
            raise ValueError('An image must be set with .set_image(...) before mask prediction.')
        if mask_input is not None:
            raise NotImplementedError('mask_input: the mask-embedding path of the prompt encoder is not implemented')
        if point_coords is None and boxes is None:
            raise ValueError('predict_torch: no prompt at all (neither points nor boxes)')
        un = lambda t: None if t is None else torch.as_tensor(t)[None]
        if boxes is not None and torch.as_tensor(boxes).dim() != 2:
            raise ValueError(f'boxes: shape {tuple(torch.as_tensor(boxes).shape)} is not [P, 4]')
        low, iou, _ = self.decoder.run(self.features, un(boxes), un(point_coords), un(point_labels), multimask_output=multimask_output)
        masks, logits = postprocess_masks(low[0], self.encoder.img_size, self.input_size, self.original_size, self.mask_threshold, return_logits)
        return (logits if return_logits else masks), iou[0], low[0]
