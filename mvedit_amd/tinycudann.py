"""`tinycudann` for the reference on gfx950: `Encoding` with the HashGrid encoding on native HIP kernels (csrc/hashgrid_encode.hip).

The reference builds its hash-grid encoders as

    tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "HashGrid", "n_levels": L, "n_features_per_level": 2,
                  "log2_hashmap_size": 19, "base_resolution": 16, "interpolation": "Smoothstep", "per_level_scale": ...},
                  dtype=torch.float32)

(lib/models/decoders/ingp_decoder.py:62-74, triplane_ingp_decoder.py:102-114), initialises `encoder.params` itself (:88) and trains it
with its own torch optimiser through `self.encoder(x)`.  `mvedit_amd.dropin.install()` seeds this module as `tinycudann`.

Supported: 3-D HashGrid ("HashGrid", or "Grid" with "type": "Hash"), Smoothstep or Linear interpolation, 1/2/4/8 features per level,
at most 16 levels, float32 parameters and output.  Anything else raises NotImplementedError naming the key; there is no fallback.
Gradients: d/dparams and d/dx, first order only (a second-order request raises).
"""
import ctypes

import torch

from . import _lib
from .nerf import level_table

__all__ = ['Encoding']

_INTERPOLATION = {'Linear': 0, 'Smoothstep': 1}           # MVE_INTERP_LINEAR / MVE_INTERP_SMOOTHSTEP (include/mvedit_amd.h)
# tiny-cuda-nn's defaults for the keys a config may leave out
_DEFAULTS = dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=2.0, interpolation='Linear')
_KEYS = set(_DEFAULTS) | {'otype', 'type', 'hash'}


def _parse_config(n_input_dims, config, dtype):
    if n_input_dims != 3:
        raise NotImplementedError(f'n_input_dims={n_input_dims}: only 3-D hash grids are implemented')
    if dtype != torch.float32:
        raise NotImplementedError(f'dtype={dtype}: only torch.float32 parameters are implemented (tinycudann defaults to half; pass '
                                  'dtype=torch.float32 as the reference does)')
    for k in config:
        if k not in _KEYS:
            raise NotImplementedError(f'encoding_config key {k!r} is not implemented')
    otype = config.get('otype')
    if not (otype == 'HashGrid' and config.get('type', 'Hash') == 'Hash' or otype == 'Grid' and config.get('type') == 'Hash'):
        raise NotImplementedError(f'encoding_config otype={otype!r} type={config.get("type")!r}: only the hash grid is implemented')
    if config.get('hash', 'CoherentPrime') != 'CoherentPrime':
        raise NotImplementedError(f'encoding_config hash={config["hash"]!r}: only "CoherentPrime" is implemented')
    c = dict(_DEFAULTS, **{k: v for k, v in config.items() if k in _DEFAULTS})
    if c['interpolation'] not in _INTERPOLATION:
        raise NotImplementedError(f'encoding_config interpolation={c["interpolation"]!r}: only "Smoothstep" and "Linear" are implemented')
    if c['n_features_per_level'] not in (1, 2, 4, 8):
        raise NotImplementedError(f'encoding_config n_features_per_level={c["n_features_per_level"]}: only 1, 2, 4 or 8 are implemented')
    if not 1 <= c['n_levels'] <= 16:
        raise NotImplementedError(f'encoding_config n_levels={c["n_levels"]}: only 1..16 levels are implemented')
    if not 1 <= c['log2_hashmap_size'] <= 30:
        raise NotImplementedError(f'encoding_config log2_hashmap_size={c["log2_hashmap_size"]}: only 1..30 are implemented')
    return c


class _SecondOrderError(torch.autograd.Function):
    """Identity on a first-order gradient computed with create_graph=True; differentiating it raises (instead of a silent zero)."""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError('mvedit_amd.tinycudann.Encoding: second-order gradients (through d enc / d x or d enc / d params) are not '
                           'implemented: the backward is once-differentiable')


class _EncodeFn(torch.autograd.Function):
    """x [N,3] f32 contiguous, params [rows*F] -> enc [N, L*F].  Backward: d params always (into a zeroed scratch that autograd adds to
    `.grad`), d x when x requires it.  The backward is once-differentiable: under create_graph=True its results carry a node that raises
    when they are differentiated."""

    @staticmethod
    def forward(ctx, x, params, enc):
        ctx.enc = enc
        ctx.save_for_backward(x, params)
        return enc._launch_forward(x, params)

    @staticmethod
    def backward(ctx, g):
        x, params = ctx.saved_tensors
        create_graph = torch.is_grad_enabled()
        with torch.no_grad():
            grad_params = torch.zeros_like(params)
            grad_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            ctx.enc._launch_backward(x, params, g.detach().to(torch.float32).contiguous(), grad_params, grad_x)
        if create_graph:
            grad_params = _SecondOrderError.apply(grad_params.requires_grad_())
            grad_x = _SecondOrderError.apply(grad_x.requires_grad_()) if grad_x is not None else None
        return grad_x, grad_params, None


class Encoding(torch.nn.Module):
    """tinycudann.Encoding (HashGrid only).  `params` is the flat [rows * F] table, level-major, F features per row: the layout
    tiny-cuda-nn's checkpoints use and the fused renderer reads (`params.reshape(-1, F)`).  It is initialised U(-1e-4, 1e-4) from
    `seed` with torch's generator: the values differ from tiny-cuda-nn's own RNG stream for the same seed (the reference overwrites
    them in init_weights anyway).  Construction allocates on torch's default device and launches nothing."""

    def __init__(self, n_input_dims, encoding_config, seed=1337, dtype=None):
        super().__init__()
        c = _parse_config(n_input_dims, encoding_config, dtype)
        self.n_input_dims, self.encoding_config, self.dtype, self.seed = n_input_dims, dict(encoding_config), dtype, seed
        self.n_levels, self.n_features_per_level = int(c['n_levels']), int(c['n_features_per_level'])
        self.interpolation = c['interpolation']
        self.n_output_dims = self.n_levels * self.n_features_per_level
        self.meta, self.n_rows = level_table(self.n_levels, c['base_resolution'], c['per_level_scale'], int(c['log2_hashmap_size']))
        L = self.n_levels
        self._scale = (ctypes.c_float * L)(*[m[0] for m in self.meta])
        self._res = (ctypes.c_uint32 * L)(*[m[1] for m in self.meta])
        self._off = (ctypes.c_uint32 * L)(*[m[2] for m in self.meta])
        self._size = (ctypes.c_uint32 * L)(*[m[3] for m in self.meta])
        g = torch.Generator().manual_seed(int(seed))
        init = torch.rand(self.n_rows * self.n_features_per_level, generator=g, dtype=torch.float32) * 2e-4 - 1e-4
        self.params = torch.nn.Parameter(init.to(torch.get_default_device()) if hasattr(torch, 'get_default_device') else init)

    def extra_repr(self):
        return f'n_input_dims={self.n_input_dims}, n_output_dims={self.n_output_dims}, encoding_config={self.encoding_config}'

    def _level_args(self, params):
        return (_lib.ptr(params), self.n_rows, self.n_features_per_level, self.n_levels, self._scale, self._res, self._off, self._size,
                _INTERPOLATION[self.interpolation])

    def _launch_forward(self, x, params):
        out = torch.empty(x.shape[0], self.n_output_dims, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call('mve_hashgrid_encode', _lib.ptr(x), x.shape[0], *self._level_args(params), _lib.ptr(out), _lib.stream_ptr(x.device))
        return out

    def _launch_backward(self, x, params, g, grad_params, grad_x):
        with torch.cuda.device(x.device):
            _lib.call('mve_hashgrid_encode_backward', _lib.ptr(x), x.shape[0], *self._level_args(params), _lib.ptr(g), _lib.ptr(grad_params),
                      _lib.ptr(grad_x), _lib.stream_ptr(x.device))

    def forward(self, x):
        """x [N, 3] in the unit cube (any float dtype / layout: a contiguous float32 copy is taken, as tiny-cuda-nn does) -> [N, n_output_dims]
        float32.  CUDA tensors only."""
        if x.dim() != 2 or x.shape[1] != self.n_input_dims:
            raise ValueError(f'Encoding expects x of shape [N, {self.n_input_dims}], got {tuple(x.shape)}')
        if not x.is_cuda:
            raise RuntimeError('mvedit_amd.tinycudann.Encoding runs on the GPU only: x is a CPU tensor (no CPU fallback)')
        if self.params.numel() != self.n_rows * self.n_features_per_level:
            raise RuntimeError(f'Encoding.params has {self.params.numel()} elements, the level table needs {self.n_rows} x {self.n_features_per_level}')
        if self.params.device != x.device or self.params.dtype != torch.float32 or not self.params.is_contiguous():
            raise RuntimeError(f'Encoding.params must be a contiguous float32 tensor on {x.device} (is {self.params.dtype} on '
                               f'{self.params.device}): move the module with .to(device)')
        x = x.to(torch.float32).contiguous()
        return _EncodeFn.apply(x, self.params, self)
