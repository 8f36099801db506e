"""The CLIP vision tower's kernels (csrc/clip_vision.hip) through ctypes, and mve_attention at the shapes the tower and the Resampler add.

mve_clip_patchify and mve_clip_vision_embed are bit-exact: the first moves data, the second rounds one fp32 sum.  mve_attention: fp16 is held to
the per-kernel bar of 1e-3 rel-L2 against float64 torch on the same 16-bit-rounded inputs, bf16 to TOL of tests/test_unet_ops.py (8e-3) on rel-L2
and on max|err| / max|ref| (measured on an MI355X over the five shapes: fp16 2.25e-4 .. 2.28e-4, bf16 1.80e-3 .. 1.83e-3 rel-L2); the hard input
families and the bound per 16-row block are in tests/test_attention_stress_gpu.py."""
import ctypes

import pytest
import torch

from test_unet_ops import TOL

pytestmark = pytest.mark.gpu

DT = {torch.float16: 1, torch.bfloat16: 2}


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('P,S', [(14, 56), (16, 32)])
def test_patchify_is_unfold_with_a_zero_tail(lib, P, S, dtype):
    B, G, K = 2, S // P, 3 * P * P
    ld = (K + 7) // 8 * 8
    px = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(P)).to(dtype)
    want = torch.zeros(B * G * G, ld, dtype=dtype)
    want[:, :K] = torch.nn.functional.unfold(px.float(), kernel_size=P, stride=P).transpose(1, 2).reshape(B * G * G, K).to(dtype)      # (c, ky, kx) columns
    rows, dpx = torch.full((B * G * G, ld), float('nan'), dtype=dtype, device='cuda'), px.cuda()
    lib.call('mve_clip_patchify', DT[dtype], lib.ptr(dpx), B, S, S, P, lib.ptr(rows), ld, lib.stream_ptr(rows.device))
    torch.cuda.synchronize()
    assert (ld > K) == (P == 14)
    assert torch.equal(rows.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_vision_embed_is_one_rounded_sum_with_the_class_row(lib, dtype):
    B, G2, C = 3, 16, 136
    g = torch.Generator().manual_seed(5)
    patch, cls, pos = (torch.randn(s, generator=g).to(dtype).cuda() for s in ((B * G2, C), (C,), (G2 + 1, C)))
    out = torch.full((B, G2 + 1, C), float('nan'), dtype=dtype, device='cuda')
    lib.call('mve_clip_vision_embed', DT[dtype], lib.ptr(patch), lib.ptr(cls), lib.ptr(pos), lib.ptr(out), B, G2, C, lib.stream_ptr(out.device))
    torch.cuda.synchronize()
    a = torch.cat([cls.expand(B, 1, C), patch.reshape(B, G2, C)], 1)
    assert torch.equal(out, (a.float() + pos.float()).to(dtype))


def _rel(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm())


def _hold(what, out, ref, dtype):
    """fp16: rel-L2 <= 1e-3.  bf16: rel-L2 and max|err| / max|ref| <= TOL."""
    rel, rmax = _rel(out, ref), float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f'{what}: rel-L2 {rel:.3e}, max|err| / max|ref| {rmax:.3e}')
    if dtype == torch.float16:
        assert rel <= 1e-3, rel
    else:
        assert rel <= TOL[dtype] and rmax <= TOL[dtype], (rel, rmax)


def _sdpa64(q, k, v, B, heads, hd, scale):
    """q [B*Lq, heads*hd], k / v [B*Lk, heads*hd] (16-bit values) -> float64 [B*Lq, heads*hd]"""
    q, k, v = (t.double().cpu().reshape(B, -1, heads, hd).transpose(1, 2) for t in (q, k, v))
    return (torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v).transpose(1, 2).reshape(-1, heads * hd)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('L,hd', [(65, 64), (257, 64), (65, 80), (257, 80)])
def test_attention_at_the_vision_shapes(lib, L, hd, dtype):
    """Self-attention over the packed q|k|v rows as the tower's GEMM leaves them: 65 tokens (one past a 64-key tile) and 257 (ViT-*/14 at 224).
    fp16: rel-L2 <= 1e-3.  bf16: rel-L2 and max|err| / max|ref| <= 8e-3 (TOL).  Measured on an MI355X over the four shapes: fp16 2.25e-4 .. 2.28e-4,
    bf16 1.80e-3 .. 1.83e-3 rel-L2."""
    B, heads = 2, 2
    C, scale = heads * hd, hd ** -0.5
    qkv = (torch.randn(B * L, 3 * C, generator=torch.Generator().manual_seed(L + hd)) * 1.5).to(dtype).cuda()
    out = torch.full((B * L, C), float('nan'), dtype=dtype, device='cuda')
    lib.call('mve_attention', DT[dtype], lib.ptr(qkv), 3 * C, lib.ptr(qkv[:, C:]), 3 * C, lib.ptr(qkv[:, 2 * C:]), 3 * C, None, 0, None, 0, lib.ptr(out), C, B, L, L, 0,
             heads, hd, ctypes.c_float(scale), lib.stream_ptr(out.device))
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    _hold(f'attention {dtype} L={L} head_dim={hd}', out, _sdpa64(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, heads, hd, scale), dtype)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_attention_at_the_resampler_shape(lib, dtype):
    """The Perceiver layer: 16 latent queries over 257 image keys and, as the second KV segment, the 16 latent keys -- equal to attention over
    cat(x, latents).  fp16: rel-L2 <= 1e-3.  bf16: rel-L2 and max|err| / max|ref| <= 8e-3 (TOL).  Measured on an MI355X: fp16 2.26e-4, bf16 1.80e-3
    rel-L2."""
    B, heads, hd, Lq, Lk, Lk2 = 2, 2, 64, 16, 257, 16
    inner = heads * hd
    g = torch.Generator().manual_seed(9)
    q = (torch.randn(B * Lq, inner, generator=g) * 1.5).to(dtype).cuda()
    kvx = (torch.randn(B * Lk, 2 * inner, generator=g) * 1.5).to(dtype).cuda()
    kvl = (torch.randn(B * Lk2, 2 * inner, generator=g) * 1.5).to(dtype).cuda()
    out = torch.full((B * Lq, inner), float('nan'), dtype=dtype, device='cuda')
    lib.call('mve_attention', DT[dtype], lib.ptr(q), inner, lib.ptr(kvx), 2 * inner, lib.ptr(kvx[:, inner:]), 2 * inner, lib.ptr(kvl), 2 * inner,
             lib.ptr(kvl[:, inner:]), 2 * inner, lib.ptr(out), inner, B, Lq, Lk, Lk2, heads, hd, ctypes.c_float(0.125), lib.stream_ptr(out.device))
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    kv = torch.cat([kvx.reshape(B, Lk, -1), kvl.reshape(B, Lk2, -1)], 1).reshape(B * (Lk + Lk2), 2 * inner)
    _hold(f'attention {dtype} Lq={Lq} Lk={Lk} Lk2={Lk2} head_dim={hd}', out, _sdpa64(q, kv[:, :inner], kv[:, inner:], B, heads, hd, 0.125), dtype)
