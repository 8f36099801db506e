"""Host-side mirror of the pipelines' `text_encoder` / `text_encoder_2` (transformers `CLIPTextModel` / `CLIPTextModelWithProjection`, built at
lib/pipelines/utils.py:244-283 and called on every request through diffusers' `_encode_prompt` / `encode_prompt`,
lib/pipelines/mvedit_3d_pipeline.py:368) on the native executor (csrc/unet.hip in CLIP mode, csrc/builder_clip.h, csrc/clip_text.hip):

    out = text_encoder(input_ids, attention_mask=None, output_hidden_states=True)
    out[0], out.pooler_output | out.text_embeds, out.hidden_states[-2], out[-1][-2]
    text_encoder.text_model.final_layer_norm(hidden)                                     (diffusers' clip_skip path)

Same state-dict names as transformers, same config field names; `transformers` itself is never imported here.  What the kernels do not
implement (padding masks, custom position ids, input embeddings, attention maps) raises -- there is no PyTorch fallback."""
import ctypes
from types import SimpleNamespace

import torch

from . import _lib
from .ops import dt as _dt
from .module_surface import EngineHandle

OP_CLASSES = ('conv', 'linear', 'attention', 'norm', 'other')
ACTS = {'quick_gelu': 0, 'gelu': 1}
CONFIG_FIELDS = ('vocab_size', 'hidden_size', 'intermediate_size', 'num_hidden_layers', 'num_attention_heads', 'max_position_embeddings', 'hidden_act',
                 'layer_norm_eps', 'eos_token_id', 'projection_dim')
CONFIG_DEFAULTS = dict(layer_norm_eps=1e-5, eos_token_id=2, projection_dim=512, hidden_act='quick_gelu')
# openai/clip-vit-large-patch14's text tower (the SD 1.x `text_encoder`)
VIT_L_14_TEXT_CONFIG = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, max_position_embeddings=77,
                            hidden_act='quick_gelu', layer_norm_eps=1e-5, eos_token_id=2, projection_dim=768)


class CLIPTextOutput:
    """transformers' `ModelOutput` as the callers use it: attributes, and indexing over the non-None fields in transformers' order
    (`BaseModelOutputWithPooling`: last_hidden_state, pooler_output, hidden_states; `CLIPTextModelOutput`: text_embeds, last_hidden_state,
    hidden_states)."""

    def __init__(self, fields):
        self._fields = [(k, v) for k, v in fields]
        for k, v in self._fields:
            setattr(self, k, v)
        self.attentions = None

    def to_tuple(self):
        return tuple(v for _, v in self._fields if v is not None)

    def keys(self):
        return [k for k, v in self._fields if v is not None]

    def __getitem__(self, i):
        if isinstance(i, str):
            d = dict(self._fields)
            if d.get(i) is None:
                raise KeyError(i)
            return d[i]
        return self.to_tuple()[i]

    def __len__(self):
        return len(self.to_tuple())

    def __iter__(self):
        return iter(self.to_tuple())


def _config_dict(config):
    get = (lambda k: config.get(k)) if isinstance(config, dict) else (lambda k: getattr(config, k, None))
    cfg = {}
    for k in CONFIG_FIELDS:
        v = get(k)
        if v is None:
            if k not in CONFIG_DEFAULTS:
                raise ValueError(f'CLIP text config: field {k} is missing')
            v = CONFIG_DEFAULTS[k]
        cfg[k] = v
    return cfg


class _FinalLayerNorm:
    """`text_model.final_layer_norm` as a callable: the native LayerNorm over the last axis of a [..., C] tensor."""

    def __init__(self, engine):
        self._e = engine
        self.weight = self.bias = None

    def __call__(self, x):
        from . import ops
        e = self._e
        if self.weight is None:
            raise KeyError('text_model.final_layer_norm.weight is not loaded')
        if x.shape[-1] != e.cfg['hidden_size']:
            raise ValueError(f'final_layer_norm: last axis {x.shape[-1]} != hidden_size {e.cfg["hidden_size"]}')
        y = ops.layernorm(x.to(device=e.device, dtype=e.dtype).reshape(-1, x.shape[-1]).contiguous(), self.weight, self.bias, eps=e.cfg['layer_norm_eps'])
        return y.reshape(x.shape)

    forward = __call__


class CLIPTextEngine(EngineHandle):
    """`CLIPTextModel` (with_projection=False) or `CLIPTextModelWithProjection` (True) on the native executor."""

    def __init__(self, config, dtype=torch.float16, device='cuda', with_projection=False):
        assert dtype in (torch.float16, torch.bfloat16)
        self.cfg = _config_dict(config)
        c = self.cfg
        if c['hidden_act'] not in ACTS:
            raise NotImplementedError(f"hidden_act {c['hidden_act']!r}: the native activations are {sorted(ACTS)}")
        self.config = config if not isinstance(config, dict) else SimpleNamespace(**c)
        self.dtype, self.device, self.with_projection = dtype, torch.device(device), bool(with_projection)
        self.projection_dim = int(c['projection_dim']) if with_projection else 0
        self._h = ctypes.c_void_p()
        _lib.call('mve_clip_text_create', ctypes.byref(self._h), _dt(dtype), int(c['vocab_size']), int(c['max_position_embeddings']), int(c['hidden_size']),
                  int(c['num_hidden_layers']), int(c['num_attention_heads']), int(c['intermediate_size']), ACTS[c['hidden_act']], float(c['layer_norm_eps']),
                  self.projection_dim)
        self._ws = None
        self.text_model = SimpleNamespace(final_layer_norm=_FinalLayerNorm(self), config=self.config)

    @classmethod
    def from_module(cls, m, dtype=None, device=None):
        """From a loaded `CLIPTextModel` / `CLIPTextModelWithProjection`: its config, state dict, dtype and device.  A module whose parameters sit on
        the CPU gives a plan-only engine (nothing is packed without an accelerator; its forward raises on the missing parameters)."""
        p = next(iter(m.parameters()))
        dtype = dtype or (p.dtype if p.dtype in (torch.float16, torch.bfloat16) else torch.float16)
        device = torch.device(device) if device is not None else p.device
        eng = cls(m.config, dtype=dtype, device=device, with_projection=hasattr(m, 'text_projection'))
        if device.type != 'cpu':
            eng.load_state_dict(m.state_dict())
        return eng

    @classmethod
    def from_state_dict(cls, state_dict, config, dtype=torch.float16, device='cuda', with_projection=False):
        return cls(config, dtype, device, with_projection).load_state_dict(state_dict)

    def expected_parameters(self):
        c, names = self.cfg, ['text_model.embeddings.token_embedding.weight', 'text_model.embeddings.position_embedding.weight']
        for k in range(int(c['num_hidden_layers'])):
            b = f'text_model.encoder.layers.{k}.'
            names += [b + n + s for n in ('layer_norm1', 'self_attn.q_proj', 'self_attn.k_proj', 'self_attn.v_proj', 'self_attn.out_proj', 'layer_norm2',
                                          'mlp.fc1', 'mlp.fc2') for s in ('.weight', '.bias')]
        names += ['text_model.final_layer_norm.weight', 'text_model.final_layer_norm.bias']
        if self.with_projection:
            names.append('text_projection.weight')
        return names

    def load_state_dict(self, state_dict, strict=True):
        own = set(self.expected_parameters())
        # transformers >= 5 dropped the `text_model.` level from CLIPTextModel's own state dict; the checkpoints (and the engine) keep it
        state_dict = {(k if k.startswith(('text_model.', 'text_projection.')) else 'text_model.' + k): v for k, v in state_dict.items()}
        if strict:
            for n in self.expected_parameters():
                if n not in state_dict:
                    raise KeyError(f'CLIP text parameter {n} is missing from the state dict')
        with torch.cuda.device(self.device):
            s = _lib.stream_ptr(self.device)
            for name, t in state_dict.items():
                if name not in own:              # buffers (`text_model.embeddings.position_ids`), a projection the plain model does not use
                    continue
                t = self._push_param(name, t, s)
                if name.startswith('text_model.final_layer_norm.'):
                    setattr(self.text_model.final_layer_norm, name.rsplit('.', 1)[1], t.float())
            torch.cuda.current_stream(self.device).synchronize()
        missing, first = self._missing_params()
        if strict and missing:
            raise KeyError(f'{missing} CLIP text parameters missing from the state dict (first: {first})')
        return self

    # ---- planning / profiling -----------------------------------------------------------------------------------------------------------
    def plan(self, B, L):
        ws, n_ops, flops = ctypes.c_size_t(), ctypes.c_int(), (ctypes.c_double * 5)()
        _lib.call('mve_clip_text_plan', self._h, int(B), int(L), ctypes.byref(ws), ctypes.byref(n_ops), flops)
        return self._plan_result(ws, n_ops, flops)

    def op_table(self):
        return [row[1:] for row in self._op_rows()]

    # ---- forward ------------------------------------------------------------------------------------------------------------------------
    def _check_ids(self, input_ids):
        if input_ids is None:
            raise ValueError('You have to specify input_ids')
        ids = input_ids.reshape(-1, input_ids.shape[-1])
        B, L = ids.shape
        c = self.cfg
        if L > int(c['max_position_embeddings']):
            raise ValueError(f"input_ids: sequence length {L} exceeds max_position_embeddings {c['max_position_embeddings']}")
        if B == 0 or L == 0:
            raise ValueError(f'input_ids: empty batch or sequence {tuple(input_ids.shape)}')
        lo, hi = torch.stack(torch.aminmax(ids)).tolist()          # one transfer when the ids sit on the device
        if lo < 0 or hi >= int(c['vocab_size']):
            raise ValueError(f"input_ids: id {lo if lo < 0 else hi} is outside [0, vocab_size = {c['vocab_size']})")
        return ids

    def run(self, input_ids, output_hidden_states=False, profile=False):
        """-> (last_hidden_state, pooler_output, text_embeds | None, hidden_states | None[, per-op ms])"""
        ids = self._check_ids(input_ids)
        B, L = ids.shape
        c, dev = self.cfg, self.device
        C, n_hidden = int(c['hidden_size']), int(c['num_hidden_layers']) + 1
        ids32 = ids.to(device=dev, dtype=torch.int32).contiguous()
        with torch.cuda.device(dev):
            info = self.plan(B, L)
            ws = self._workspace(info['workspace_bytes'])
            last = torch.empty(B, L, C, dtype=self.dtype, device=dev)
            pooled = torch.empty(B, C, dtype=self.dtype, device=dev)
            embeds = torch.empty(B, self.projection_dim, dtype=self.dtype, device=dev) if self.projection_dim else None
            hidden = tuple(torch.empty(B, L, C, dtype=self.dtype, device=dev) for _ in range(n_hidden)) if output_hidden_states else None
            hs = (ctypes.c_void_p * n_hidden)(*[h.data_ptr() for h in hidden]) if hidden else None
            op_ms = (ctypes.c_float * info['n_ops'])() if profile else None
            _lib.call('mve_clip_text_forward', self._h, _lib.ptr(ids32), B, L, int(c['eos_token_id']), _lib.ptr(last), _lib.ptr(pooled), _lib.ptr(embeds), hs,
                      _lib.ptr(ws), ws.numel(), op_ms, _lib.stream_ptr(dev))
        res = (last, pooled, embeds, hidden)
        return res + (list(op_ms),) if profile else res

    def __call__(self, input_ids=None, attention_mask=None, position_ids=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                 inputs_embeds=None):
        if position_ids is not None:
            raise NotImplementedError('position_ids: the native embedding uses positions 0..L-1')
        if inputs_embeds is not None:
            raise NotImplementedError('inputs_embeds: the native text tower starts from input_ids')
        if output_attentions:
            raise NotImplementedError('output_attentions=True: the causal attention kernel does not materialise the attention maps')
        if attention_mask is not None and not bool((attention_mask == 1).all()):
            raise NotImplementedError('attention_mask: padding masks are not implemented (pass None or all ones, as diffusers does for CLIP)')
        last, pooled, embeds, hidden = self.run(input_ids, bool(output_hidden_states))
        if self.with_projection:
            out = CLIPTextOutput([('text_embeds', embeds), ('last_hidden_state', last), ('hidden_states', hidden)])
        else:
            out = CLIPTextOutput([('last_hidden_state', last), ('pooler_output', pooled), ('hidden_states', hidden)])
        return out if (return_dict is None or return_dict) else out.to_tuple()

    forward = __call__
