"""Host-side mirror of the reference's image towers (transformers `CLIPVisionModelWithProjection` / `CLIPVisionModel`) on the native executor
(csrc/unet.hip in CLIP vision mode, csrc/builder_clip_vision.h, csrc/clip_vision.hip):

    IPAdapter.image_encoder(clip_image).image_embeds                                      (lib/models/architecture/ip_adapter/ip_adapter.py:130)
    IPAdapter.image_encoder(clip_image, output_hidden_states=True).hidden_states[-2]      (:138, the "plus" checkpoints)
    Zero123PlusPipeline.vision_encoder(image_2, output_hidden_states=False).image_embeds  (lib/pipelines/zero123plus.py:372)
    Zero123Pipeline.image_encoder(image).image_embeds                                     (lib/pipelines/zero123.py:260)

Same state-dict names as transformers, same config field names; `transformers` itself is never imported here.  What the kernels do not
implement (attention maps, interpolated position encodings, other image sizes) raises -- there is no PyTorch fallback.  The PIL resize and
normalisation of `CLIPImageProcessor` stay where they are: the engine starts from `pixel_values`."""
import ctypes
from types import SimpleNamespace

import torch

from . import _lib
from .ops import dt as _dt
from .module_surface import EngineHandle
from .text_encoder import ACTS, CLIPTextOutput

CONFIG_FIELDS = ('hidden_size', 'intermediate_size', 'num_hidden_layers', 'num_attention_heads', 'image_size', 'patch_size', 'hidden_act', 'layer_norm_eps',
                 'projection_dim', 'num_channels')
CONFIG_DEFAULTS = dict(layer_norm_eps=1e-5, projection_dim=512, hidden_act='quick_gelu', num_channels=3)
# the ViT-H/14 tower of the IP-Adapter checkpoints (`models/image_encoder`, laion/CLIP-ViT-H-14-laion2B-s32B-b79K)
VIT_H_14_VISION_CONFIG = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, image_size=224, patch_size=14, hidden_act='gelu',
                              layer_norm_eps=1e-5, projection_dim=1024, num_channels=3)

CLIPVisionOutput = CLIPTextOutput          # the same ModelOutput-style container: attributes, and indexing over the non-None fields


def _config_dict(config):
    get = (lambda k: config.get(k)) if isinstance(config, dict) else (lambda k: getattr(config, k, None))
    cfg = {}
    for k in CONFIG_FIELDS:
        v = get(k)
        if v is None:
            if k not in CONFIG_DEFAULTS:
                raise ValueError(f'CLIP vision config: field {k} is missing')
            v = CONFIG_DEFAULTS[k]
        cfg[k] = v
    return cfg


class CLIPVisionEngine(EngineHandle):
    """`CLIPVisionModelWithProjection` (with_projection=True) or `CLIPVisionModel` (False) on the native executor."""

    def __init__(self, config, dtype=torch.float16, device='cuda', with_projection=True):
        assert dtype in (torch.float16, torch.bfloat16)
        self.cfg = _config_dict(config)
        c = self.cfg
        if c['hidden_act'] not in ACTS:
            raise NotImplementedError(f"hidden_act {c['hidden_act']!r}: the native activations are {sorted(ACTS)}")
        if int(c['num_channels']) != 3:
            raise NotImplementedError(f"num_channels {c['num_channels']}: the native patch embedding takes 3 channels")
        self.config = config if not isinstance(config, dict) else SimpleNamespace(**c)
        self.dtype, self.device, self.with_projection = dtype, torch.device(device), bool(with_projection)
        self.projection_dim = int(c['projection_dim']) if with_projection else 0
        self._h = ctypes.c_void_p()
        _lib.call('mve_clip_vision_create', ctypes.byref(self._h), _dt(dtype), int(c['image_size']), int(c['patch_size']), int(c['hidden_size']),
                  int(c['num_hidden_layers']), int(c['num_attention_heads']), int(c['intermediate_size']), ACTS[c['hidden_act']], float(c['layer_norm_eps']),
                  self.projection_dim)
        self.num_tokens = (int(c['image_size']) // int(c['patch_size'])) ** 2 + 1
        self._ws = None

    @classmethod
    def from_module(cls, m, dtype=None, device=None):
        """From a loaded `CLIPVisionModel` / `CLIPVisionModelWithProjection`: its config, state dict, dtype and device.  A module whose parameters
        sit on the CPU gives a plan-only engine (nothing is packed without an accelerator; its forward raises on the missing parameters)."""
        p = next(iter(m.parameters()))
        dtype = dtype or (p.dtype if p.dtype in (torch.float16, torch.bfloat16) else torch.float16)
        device = torch.device(device) if device is not None else p.device
        eng = cls(m.config, dtype=dtype, device=device, with_projection=hasattr(m, 'visual_projection'))
        if device.type != 'cpu':
            eng.load_state_dict(m.state_dict())
        return eng

    @classmethod
    def from_state_dict(cls, state_dict, config, dtype=torch.float16, device='cuda', with_projection=True):
        return cls(config, dtype, device, with_projection).load_state_dict(state_dict)

    def expected_parameters(self):
        c = self.cfg
        names = ['vision_model.embeddings.class_embedding', 'vision_model.embeddings.patch_embedding.weight', 'vision_model.embeddings.position_embedding.weight',
                 'vision_model.pre_layrnorm.weight', 'vision_model.pre_layrnorm.bias']
        for k in range(int(c['num_hidden_layers'])):
            b = f'vision_model.encoder.layers.{k}.'
            names += [b + n + s for n in ('layer_norm1', 'self_attn.q_proj', 'self_attn.k_proj', 'self_attn.v_proj', 'self_attn.out_proj', 'layer_norm2',
                                          'mlp.fc1', 'mlp.fc2') for s in ('.weight', '.bias')]
        names += ['vision_model.post_layernorm.weight', 'vision_model.post_layernorm.bias']
        if self.with_projection:
            names.append('visual_projection.weight')
        return names

    def load_state_dict(self, state_dict, strict=True):
        own = set(self.expected_parameters())
        # transformers >= 5 dropped the `vision_model.` level from CLIPVisionModel's own state dict; the checkpoints (and the engine) keep it
        state_dict = {(k if k.startswith(('vision_model.', 'visual_projection.')) else 'vision_model.' + k): v for k, v in state_dict.items()}
        if strict:
            for n in self.expected_parameters():
                if n not in state_dict:
                    raise KeyError(f'CLIP vision parameter {n} is missing from the state dict')
        with torch.cuda.device(self.device):
            s = _lib.stream_ptr(self.device)
            for name, t in state_dict.items():
                if name not in own:              # buffers (`vision_model.embeddings.position_ids`), a projection the plain model does not use
                    continue
                self._push_param(name, t, s)
            torch.cuda.current_stream(self.device).synchronize()
        missing, first = self._missing_params()
        if strict and missing:
            raise KeyError(f'{missing} CLIP vision parameters missing from the state dict (first: {first})')
        return self

    # ---- planning / profiling -----------------------------------------------------------------------------------------------------------
    def plan(self, B):
        ws, n_ops, flops = ctypes.c_size_t(), ctypes.c_int(), (ctypes.c_double * 5)()
        _lib.call('mve_clip_vision_plan', self._h, int(B), ctypes.byref(ws), ctypes.byref(n_ops), flops)
        return self._plan_result(ws, n_ops, flops)

    def op_table(self):
        return [row[1:] for row in self._op_rows()]

    # ---- forward ------------------------------------------------------------------------------------------------------------------------
    def _check_pixels(self, pixel_values):
        if pixel_values is None:
            raise ValueError('You have to specify pixel_values')
        S = int(self.cfg['image_size'])
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, S, S) or pixel_values.shape[0] == 0:
            raise ValueError(f'pixel_values: shape {tuple(pixel_values.shape)} is not [B, 3, {S}, {S}] (image_size {S}; other sizes need interpolate_pos_encoding, '
                             f'which is not implemented)')
        if not pixel_values.is_floating_point():
            raise ValueError(f'pixel_values: dtype {pixel_values.dtype} is not a floating-point type')
        return pixel_values

    def run(self, pixel_values, output_hidden_states=False, profile=False):
        """-> (last_hidden_state, pooler_output, image_embeds | None, hidden_states | None[, per-op ms])"""
        px = self._check_pixels(pixel_values)
        B = px.shape[0]
        c, dev = self.cfg, self.device
        C, T, n_hidden = int(c['hidden_size']), self.num_tokens, int(c['num_hidden_layers']) + 1
        px = px.to(device=dev, dtype=self.dtype).contiguous()
        with torch.cuda.device(dev):
            info = self.plan(B)
            ws = self._workspace(info['workspace_bytes'])
            last = torch.empty(B, T, C, dtype=self.dtype, device=dev)
            pooled = torch.empty(B, C, dtype=self.dtype, device=dev)
            embeds = torch.empty(B, self.projection_dim, dtype=self.dtype, device=dev) if self.projection_dim else None
            hidden = tuple(torch.empty(B, T, C, dtype=self.dtype, device=dev) for _ in range(n_hidden)) if output_hidden_states else None
            hs = (ctypes.c_void_p * n_hidden)(*[h.data_ptr() for h in hidden]) if hidden else None
            op_ms = (ctypes.c_float * info['n_ops'])() if profile else None
            _lib.call('mve_clip_vision_forward', self._h, _lib.ptr(px), B, _lib.ptr(last), _lib.ptr(pooled), _lib.ptr(embeds), hs, _lib.ptr(ws),
                      ws.numel(), op_ms, _lib.stream_ptr(dev))
        res = (last, pooled, embeds, hidden)
        return res + (list(op_ms),) if profile else res

    def __call__(self, pixel_values=None, output_attentions=None, output_hidden_states=None, return_dict=None, interpolate_pos_encoding=False):
        if output_attentions:
            raise NotImplementedError('output_attentions=True: the attention kernel does not materialise the attention maps')
        if interpolate_pos_encoding:
            raise NotImplementedError('interpolate_pos_encoding=True: the native embedding uses the trained position table at image_size')
        last, pooled, embeds, hidden = self.run(pixel_values, bool(output_hidden_states))
        if self.with_projection:
            out = CLIPVisionOutput([('image_embeds', embeds), ('last_hidden_state', last), ('hidden_states', hidden)])
        else:
            out = CLIPVisionOutput([('last_hidden_state', last), ('pooler_output', pooled), ('hidden_states', hidden)])
        return out if (return_dict is None or return_dict) else out.to_tuple()

    forward = __call__
