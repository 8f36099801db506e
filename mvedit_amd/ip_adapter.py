"""Host-side mirrors of the IP-Adapter image projection models (`IPAdapter.image_proj_model`, built at
lib/models/architecture/ip_adapter/ip_adapter.py:58, :64-83 and called at :131, :136, :139, :146):

    ResamplerEngine    the "plus" checkpoints' `Resampler` (lib/models/architecture/ip_adapter/resampler.py:77-120) on the native executor
                       (csrc/unet.hip in Resampler mode, csrc/builder_clip_vision.h): [B, n1, embedding_dim] -> [B, num_queries, output_dim]
    ImageProjEngine    `ImageProjModel` (ip_adapter.py:15-29): one Linear, a reshape and a LayerNorm -- mve_gemm + mve_layernorm, no handle:
                       [B, clip_embeddings_dim] -> [B, clip_extra_context_tokens, cross_attention_dim]

Both are built with the reference constructors' keywords and load the reference modules' state dicts.  One intended rounding difference in the
Resampler: the reference scales q and k by dim_head^-1/4 each and rounds the softmax to 16 bit; the engine scales the fp32 logits by 1/8 and keeps
the fp32 softmax of mve_attention.  There is no PyTorch fallback."""
import ctypes

import torch

from . import _lib
from .ops import dt as _dt
from .module_surface import EngineHandle, InferenceSurface


class ResamplerEngine(EngineHandle):
    """`Resampler(dim, depth, dim_head, heads, num_queries, embedding_dim, output_dim, ff_mult)` on the native executor."""

    def __init__(self, dim=1024, depth=8, dim_head=64, heads=16, num_queries=8, embedding_dim=768, output_dim=1024, ff_mult=4, dtype=torch.float16, device='cuda'):
        assert dtype in (torch.float16, torch.bfloat16)
        if int(dim_head) != 64:
            raise NotImplementedError(f'dim_head {dim_head}: the native Resampler runs dim_head 64 (every IP-Adapter checkpoint)')
        if int(ff_mult) != ff_mult:
            raise NotImplementedError(f'ff_mult {ff_mult}: the native Resampler takes an integer multiplier')
        self.dim, self.depth, self.dim_head, self.heads, self.num_queries = int(dim), int(depth), 64, int(heads), int(num_queries)
        self.embedding_dim, self.output_dim, self.ff_mult = int(embedding_dim), int(output_dim), int(ff_mult)
        self.dtype, self.device = dtype, torch.device(device)
        self._h = ctypes.c_void_p()
        _lib.call('mve_ip_resampler_create', ctypes.byref(self._h), _dt(dtype), self.dim, self.depth, self.heads, self.num_queries, self.embedding_dim,
                  self.output_dim, self.ff_mult)
        self._ws = None

    @classmethod
    def from_module(cls, m, dtype=None, device=None):
        """From a loaded reference `Resampler`: the geometry is read off its parameters (the module keeps no config)."""
        p = m.latents
        dtype = dtype or (p.dtype if p.dtype in (torch.float16, torch.bfloat16) else torch.float16)
        device = torch.device(device) if device is not None else p.device
        attn = m.layers[0][0]
        eng = cls(dim=p.shape[-1], depth=len(m.layers), dim_head=attn.dim_head, heads=attn.heads, num_queries=p.shape[1], embedding_dim=m.proj_in.in_features,
                  output_dim=m.proj_out.out_features, ff_mult=m.layers[0][1][1].out_features / p.shape[-1], dtype=dtype, device=device)
        if device.type != 'cpu':
            eng.load_state_dict(m.state_dict())
        return eng

    def expected_parameters(self):
        names = ['latents', 'proj_in.weight', 'proj_in.bias', 'proj_out.weight', 'proj_out.bias', 'norm_out.weight', 'norm_out.bias']
        for k in range(self.depth):
            a, f = f'layers.{k}.0.', f'layers.{k}.1.'
            names += [a + 'norm1.weight', a + 'norm1.bias', a + 'norm2.weight', a + 'norm2.bias', a + 'to_q.weight', a + 'to_kv.weight', a + 'to_out.weight',
                      f + '0.weight', f + '0.bias', f + '1.weight', f + '3.weight']
        return names

    def load_state_dict(self, state_dict, strict=True):
        own = self.expected_parameters()
        if strict:
            for n in own:
                if n not in state_dict:
                    raise KeyError(f'Resampler parameter {n} is missing from the state dict')
            extra = [k for k in state_dict if k not in set(own)]
            if extra:
                raise KeyError(f'{extra[0]} is not a parameter of this Resampler')
        with torch.cuda.device(self.device):
            s = _lib.stream_ptr(self.device)
            for name in own:
                if name not in state_dict:
                    continue
                self._push_param(name, state_dict[name], s)
            torch.cuda.current_stream(self.device).synchronize()
        return self

    def plan(self, B, n1):
        ws, n_ops, flops = ctypes.c_size_t(), ctypes.c_int(), (ctypes.c_double * 5)()
        _lib.call('mve_ip_resampler_plan', self._h, int(B), int(n1), ctypes.byref(ws), ctypes.byref(n_ops), flops)
        return self._plan_result(ws, n_ops, flops)

    def op_table(self):
        return [row[1:] for row in self._op_rows()]

    def run(self, x, profile=False):
        if x.dim() != 3 or x.shape[-1] != self.embedding_dim or x.shape[0] == 0 or x.shape[1] == 0:
            raise ValueError(f'Resampler input: shape {tuple(x.shape)} is not [B, n1, embedding_dim = {self.embedding_dim}]')
        B, n1, _ = x.shape
        dev = self.device
        x = x.to(device=dev, dtype=self.dtype).contiguous()
        with torch.cuda.device(dev):
            info = self.plan(B, n1)
            ws = self._workspace(info['workspace_bytes'])
            out = torch.empty(B, self.num_queries, self.output_dim, dtype=self.dtype, device=dev)
            op_ms = (ctypes.c_float * info['n_ops'])() if profile else None
            _lib.call('mve_ip_resampler_forward', self._h, _lib.ptr(x), B, n1, _lib.ptr(out), _lib.ptr(ws), ws.numel(), op_ms, _lib.stream_ptr(dev))
        return (out, list(op_ms)) if profile else out

    def __call__(self, x):
        return self.run(x)

    forward = __call__


class ImageProjEngine(InferenceSurface):
    """`ImageProjModel(cross_attention_dim, clip_embeddings_dim, clip_extra_context_tokens)`: mve_gemm (bias fused) + mve_layernorm."""

    def __init__(self, cross_attention_dim=1024, clip_embeddings_dim=1024, clip_extra_context_tokens=4, dtype=torch.float16, device='cuda'):
        assert dtype in (torch.float16, torch.bfloat16)
        self.cross_attention_dim, self.clip_embeddings_dim = int(cross_attention_dim), int(clip_embeddings_dim)
        self.clip_extra_context_tokens = int(clip_extra_context_tokens)
        if self.cross_attention_dim % 8 or self.clip_embeddings_dim % 8 or self.cross_attention_dim > 2048:
            raise NotImplementedError(f'ImageProjModel {self.clip_embeddings_dim} -> {self.clip_extra_context_tokens} x {self.cross_attention_dim}: the native '
                                      f'kernels take widths that are multiples of 8 and a cross_attention_dim of at most 2048')
        self.dtype, self.device = dtype, torch.device(device)
        self._w = self._b = self._g = self._beta = None

    @classmethod
    def from_module(cls, m, dtype=None, device=None):
        p = m.proj.weight
        dtype = dtype or (p.dtype if p.dtype in (torch.float16, torch.bfloat16) else torch.float16)
        device = torch.device(device) if device is not None else p.device
        eng = cls(cross_attention_dim=m.cross_attention_dim, clip_embeddings_dim=m.proj.in_features, clip_extra_context_tokens=m.clip_extra_context_tokens,
                  dtype=dtype, device=device)
        if device.type != 'cpu':
            eng.load_state_dict(m.state_dict())
        return eng

    def expected_parameters(self):
        return ['proj.weight', 'proj.bias', 'norm.weight', 'norm.bias']

    def load_state_dict(self, state_dict, strict=True):
        for n in self.expected_parameters():
            if n not in state_dict:
                raise KeyError(f'ImageProjModel parameter {n} is missing from the state dict')
        N, K, D = self.clip_extra_context_tokens * self.cross_attention_dim, self.clip_embeddings_dim, self.cross_attention_dim
        want = {'proj.weight': (N, K), 'proj.bias': (N,), 'norm.weight': (D,), 'norm.bias': (D,)}
        for n, shp in want.items():
            if tuple(state_dict[n].shape) != shp:
                raise ValueError(f'ImageProjModel parameter {n}: shape {tuple(state_dict[n].shape)} is not {shp}')
        dev = self.device
        self._w = state_dict['proj.weight'].detach().to(device=dev, dtype=self.dtype).contiguous()
        self._b, self._g, self._beta = (state_dict[n].detach().to(device=dev, dtype=torch.float32).contiguous() for n in ('proj.bias', 'norm.weight', 'norm.bias'))
        return self

    def __call__(self, image_embeds):
        from . import ops
        if self._w is None:
            raise KeyError('proj.weight is not loaded')
        if image_embeds.dim() != 2 or image_embeds.shape[-1] != self.clip_embeddings_dim or image_embeds.shape[0] == 0:
            raise ValueError(f'ImageProjModel input: shape {tuple(image_embeds.shape)} is not [B, clip_embeddings_dim = {self.clip_embeddings_dim}]')
        x = image_embeds.to(device=self.device, dtype=self.dtype).contiguous()
        y = ops.gemm(x, self._w, bias=self._b, flags=ops.NO_SPLITK)
        y = ops.layernorm(y.reshape(-1, self.cross_attention_dim), self._g, self._beta, eps=1e-5)
        return y.reshape(x.shape[0], self.clip_extra_context_tokens, self.cross_attention_dim)

    forward = __call__
