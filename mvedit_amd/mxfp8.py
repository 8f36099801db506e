"""MXFP8 block-scaled linear: typed wrappers over mve_mxfp8_quantize / mve_mxfp8_gemm (section 2b of include/mvedit_amd.h) and the host
converters that are the written specification of the packed format.

A `[R, K]` matrix (K % 32 == 0) is packed as `q` uint8 `[R, Kp]` (OCP e4m3fn bytes, Kp = 128 * ceil(K / 128)) and `e` uint8 `[R, Kp / 32]` (E8M0:
byte b = 2^(b - 127)); element (r, k) = e4m3(q[r, k]) * 2^(e[r, k // 32] - 127); the padding columns hold q = 0, e = 127.  The scale of a block
is the smallest power of two that brings the block's amax to at most 448 (the clipping-free variant of the MX rule).  No op here has a torch
fallback: `quantize`, `gemm` and `MXFP8Linear` run the HIP kernels or raise.
"""
import torch

from . import _lib
from .ops import dt, _s

BLOCK = 32
E4M3_MAX = 448.0


def packed_k(K):
    """Kp of the packed format (mve_mxfp8_packed_k); raises when K is not a positive multiple of 32."""
    Kp = _lib.raw('mve_mxfp8_packed_k')(int(K))
    if Kp < 0:
        raise ValueError(f'MXFP8: K = {K} must be a positive multiple of 32')
    return Kp


# ----------------------------------------------------------------------------------------------------------------------------------
# host converters: the specification
# ----------------------------------------------------------------------------------------------------------------------------------
def block_exponents(x):
    """[R, K] -> int32 [R, K / 32]: the scale exponent s of every 32-element block (E8M0 byte = s + 127)."""
    R, K = x.shape
    assert K > 0 and K % BLOCK == 0, 'K must be a positive multiple of 32'
    amax = x.float().reshape(R, K // BLOCK, BLOCK).abs().amax(-1)
    m, ex = torch.frexp(amax)                                     # amax = m * 2^ex, 0.5 <= m < 1
    s = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(-127, 127)  # smallest s with amax * 2^-s <= 448 = 0.875 * 2^9
    return torch.where(amax == 0, torch.zeros_like(s), s).to(torch.int32)


def quantize_host(x):
    """Plain-torch quantiser, any device: x [R, K] (f32 / f16 / bf16, finite) -> (q uint8 [R, Kp], e uint8 [R, Kp / 32]), bit for bit what
    mve_mxfp8_quantize writes.  NaN -> 0 as on the device; infinities are outside the contract."""
    R, K = x.shape
    Kp = 128 * ((K + 127) // 128)
    x = x.float()
    x = torch.where(x == x, x, torch.zeros_like(x))
    s = block_exponents(x)
    # the scaling is exact (a power of two) wherever the result is not an f32 subnormal, 2^116 times below e4m3's rounding boundary 2^-10;
    # without the clamp torch's cast turns out-of-range values into NaN
    y = torch.ldexp(x.reshape(R, K // BLOCK, BLOCK), -s.unsqueeze(-1)).clamp(-E4M3_MAX, E4M3_MAX)
    q = torch.zeros(R, Kp, dtype=torch.uint8, device=x.device)
    q[:, :K] = y.reshape(R, K).to(torch.float8_e4m3fn).view(torch.uint8)
    e = torch.full((R, Kp // BLOCK), 127, dtype=torch.uint8, device=x.device)
    e[:, :K // BLOCK] = (s + 127).to(torch.uint8)
    return q, e


def dequantize_host(q, e, K, dtype=torch.float64):
    """(q, e) -> the [R, K] matrix they stand for; exact in float64 (the default) for every byte pair, in float32 wherever the value fits."""
    R, Kp = q.shape
    assert Kp % 128 == 0 and e.shape == (R, Kp // BLOCK) and 0 < K <= Kp
    v = q.view(torch.float8_e4m3fn).to(torch.float64).reshape(R, Kp // BLOCK, BLOCK)
    v = v * torch.pow(torch.tensor(2.0, dtype=torch.float64, device=q.device), e.to(torch.float64) - 127.0).unsqueeze(-1)
    return v.reshape(R, Kp)[:, :K].to(dtype)


# ----------------------------------------------------------------------------------------------------------------------------------
# device entry points
# ----------------------------------------------------------------------------------------------------------------------------------
def quantize(x):
    """x: 2-D CUDA tensor, f32 / f16 / bf16, dense last axis (row-strided views are fine) -> (q, e) on the same device."""
    assert isinstance(x, torch.Tensor) and x.is_cuda, 'native path: CUDA tensors only'
    assert x.dim() == 2 and x.stride(-1) == 1 and x.dtype in (torch.float32, torch.float16, torch.bfloat16), (x.dtype, x.shape)
    R, K = x.shape
    Kp = packed_k(K)
    q = torch.empty(R, Kp, dtype=torch.uint8, device=x.device)
    e = torch.empty(R, Kp // BLOCK, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call('mve_mxfp8_quantize', dt(x), _lib.ptr(x), x.stride(0), R, K, _lib.ptr(q), _lib.ptr(e), _s(x))
    return q, e


def _chk_packed(q, e, K, name):
    assert q.is_cuda and e.is_cuda, 'native path: CUDA tensors only'
    assert q.dtype == torch.uint8 and e.dtype == torch.uint8 and q.is_contiguous() and e.is_contiguous(), f'{name}: contiguous uint8 tensors'
    assert q.dim() == 2 and q.shape[1] == packed_k(K) and e.shape == (q.shape[0], q.shape[1] // BLOCK), (name, q.shape, e.shape, K)


def gemm(aq, ae, wq, we, K, bias=None, residual=None, out_dtype=torch.float16, out=None):
    """Packed A [M, Kp] x packed W [N, Kp] (torch Linear layout) -> [M, N] in `out_dtype` (f32 / f16 / bf16):
    round_once(sum_k A W + bias + residual), fp32 accumulation and adds.  bias: fp32 [N]; residual: [M, N] of out_dtype (row stride free);
    out: optional destination, a view with any row stride."""
    _chk_packed(aq, ae, K, 'A')
    _chk_packed(wq, we, K, 'W')
    M, N = aq.shape[0], wq.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=aq.device)
    assert out.is_cuda and out.shape == (M, N) and out.dtype == out_dtype and out.stride(-1) == 1
    assert bias is None or (bias.is_cuda and bias.dtype == torch.float32 and bias.shape == (N,) and bias.is_contiguous())
    assert residual is None or (residual.is_cuda and residual.dtype == out_dtype and residual.shape == (M, N) and residual.stride(-1) == 1)
    with torch.cuda.device(aq.device):
        _lib.call('mve_mxfp8_gemm', _lib.ptr(aq), _lib.ptr(ae), _lib.ptr(wq), _lib.ptr(we), M, N, int(K), dt(out_dtype), _lib.ptr(out),
                  out.stride(0), _lib.ptr(bias), _lib.ptr(residual), residual.stride(0) if residual is not None else 0, _s(aq))
    return out


class MXFP8Linear:
    """y = x W^T + b with both operands in MXFP8: the weight [N, K] of an nn.Linear is packed once with the quantise kernel, every call
    quantises its activations, runs the block-scaled GEMM and adds the bias in its epilogue.  The output has x's dtype."""

    def __init__(self, weight, bias=None):
        assert weight.is_cuda and weight.dim() == 2, 'native path: a 2-D CUDA weight'
        self.out_features, self.in_features = weight.shape
        self.wq, self.we = quantize(weight.detach())
        self.bias = None if bias is None else bias.detach().to(device=weight.device, dtype=torch.float32).contiguous()

    def __call__(self, x):
        assert isinstance(x, torch.Tensor) and x.is_cuda, 'native path: CUDA tensors only'
        assert x.shape[-1] == self.in_features, (x.shape, self.in_features)
        x2 = x.reshape(-1, self.in_features)
        aq, ae = quantize(x2)
        y = gemm(aq, ae, self.wq, self.we, self.in_features, bias=self.bias, out_dtype=x.dtype)
        return y.reshape(*x.shape[:-1], self.out_features)
