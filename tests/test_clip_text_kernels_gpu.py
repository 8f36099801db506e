"""The CLIP text tower's kernels (csrc/clip_text.hip) through ctypes against float64 torch computations on the same 16-bit-rounded inputs.

mve_attention_causal: fp16 is held to the per-kernel bar of 1e-3 rel-L2, bf16 to TOL of tests/test_unet_ops.py (8e-3) on rel-L2 and on
max|err| / max|ref| (measured on an MI355X: see the docstring of test_causal_attention_against_float64); the hard input families and the bound per
16-row block are in tests/test_attention_stress_gpu.py.  The structural properties are bit-exact: row 0 is V[0], rows <= p do not depend
on keys / values > p, two runs agree, an item does not depend on the batch."""
import ctypes

import pytest
import torch

from test_unet_ops import TOL

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 2, 16), (2, 3, 17), (3, 2, 77), (1, 20, 77), (1, 2, 128)]
DT = {torch.float16: 1, torch.bfloat16: 2}


def _qkv(B, heads, L, dtype, seed=0):
    """packed [B*L, 3*heads*64] projections as the engine's q|k|v GEMM leaves them; logits of a few units so that the softmax is not flat"""
    g = torch.Generator().manual_seed(seed + 1000 * L + heads)
    qkv = torch.randn(B * L, 3 * heads * 64, generator=g) * 1.5
    return qkv.to(dtype).cuda()


def _causal(lib, qkv, B, heads, L):
    C = heads * 64
    out = torch.full((B * L, C), float('nan'), dtype=qkv.dtype, device=qkv.device)
    lib.call('mve_attention_causal', DT[qkv.dtype], lib.ptr(qkv), 3 * C, lib.ptr(qkv[:, C:]), 3 * C, lib.ptr(qkv[:, 2 * C:]), 3 * C, lib.ptr(out), C, B, L, heads, 64,
             ctypes.c_float(0.125), lib.stream_ptr(qkv.device))
    torch.cuda.synchronize()
    return out


def _reference(qkv, B, heads, L):
    C = heads * 64
    x = qkv.double().cpu().reshape(B, L, 3, heads, 64)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) * 0.125
    s = s.masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(), float('-inf'))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * L, C)


def _rel(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm())


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('B,heads,L', SHAPES)
def test_causal_attention_against_float64(lib, B, heads, L, dtype):
    """fp16: rel-L2 <= 1e-3.  bf16: rel-L2 and max|err| / max|ref| <= 8e-3 (TOL).  Measured on an MI355X over the six shapes: fp16 2.07e-4 ...
    2.22e-4 and bf16 1.62e-3 ... 1.76e-3 rel-L2 (both exactly 0 at L = 1, where the output is V[0])."""
    qkv = _qkv(B, heads, L, dtype)
    out = _causal(lib, qkv, B, heads, L)
    assert torch.isfinite(out.float()).all()
    ref = _reference(qkv, B, heads, L)
    rel, rmax = _rel(out, ref), float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f'causal attention {dtype} B={B} heads={heads} L={L}: rel-L2 {rel:.3e}, max|err| / max|ref| {rmax:.3e}')
    if dtype == torch.float16:
        assert rel <= 1e-3, rel
    else:
        assert rel <= TOL[dtype] and rmax <= TOL[dtype], (rel, rmax)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_causal_attention_bit_exact_properties(lib, dtype):
    B, heads, L, C = 3, 2, 77, 128
    qkv = _qkv(B, heads, L, dtype, seed=3)
    out = _causal(lib, qkv, B, heads, L)
    # softmax over one key: row 0 of every head is V[0]
    assert torch.equal(out.reshape(B, L, C)[:, 0], qkv.reshape(B, L, 3 * C)[:, 0, 2 * C:])
    # two runs agree
    assert torch.equal(out, _causal(lib, qkv, B, heads, L))
    # rows <= p do not see K / V rows > p
    for p in (0, 15, 16, 40):
        other = qkv.clone().reshape(B, L, 3 * C)
        other[:, p + 1:, C:] = (torch.randn(B, L - p - 1, 2 * C, generator=torch.Generator().manual_seed(p)) * 3).to(dtype).cuda()
        got = _causal(lib, other.reshape(B * L, 3 * C), B, heads, L).reshape(B, L, C)
        assert torch.equal(got[:, :p + 1], out.reshape(B, L, C)[:, :p + 1]), p
        assert not torch.equal(got[:, p + 1:], out.reshape(B, L, C)[:, p + 1:]), p
    # an item's output does not depend on the batch
    for b in range(B):
        assert torch.equal(_causal(lib, qkv[b * L:(b + 1) * L].contiguous(), 1, heads, L), out[b * L:(b + 1) * L]), b


def test_causal_attention_refuses_bad_shapes(lib):
    x, o = torch.zeros(128, 192, dtype=torch.float16, device='cuda'), torch.zeros(128, 64, dtype=torch.float16, device='cuda')
    f = lib.raw('mve_attention_causal')
    P = lib.ptr

    def rc(L, hd):
        return f(1, P(x), 192, P(x[:, 64:]), 192, P(x[:, 128:]), 192, P(o), 64, 1, L, 1, hd, ctypes.c_float(0.125), None)
    assert rc(0, 64) == -1 and ' L ' in lib.last_error()
    assert rc(129, 64) == -1 and ' L ' in lib.last_error()
    assert rc(16, 40) == -1 and 'head_dim' in lib.last_error()
    assert rc(16, 64) == 0


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_embed_is_bit_exact(lib, dtype):
    g = torch.Generator().manual_seed(5)
    vocab, max_pos, C, B, L = 97, 77, 136, 3, 19
    tok, pos = torch.randn(vocab, C, generator=g).to(dtype).cuda(), torch.randn(max_pos, C, generator=g).to(dtype).cuda()
    ids = torch.randint(0, vocab, (B, L), generator=g, dtype=torch.int32)
    ids[0, 0], ids[1, 3], ids[2, L - 1] = 0, vocab - 1, vocab - 1
    ids = ids.cuda()
    out = torch.empty(B, L, C, dtype=dtype, device='cuda')
    lib.call('mve_clip_embed', DT[dtype], lib.ptr(ids), lib.ptr(tok), lib.ptr(pos), lib.ptr(out), B, L, C, vocab, max_pos, lib.stream_ptr(out.device))
    torch.cuda.synchronize()
    want = (tok[ids.long()].float() + pos[:L].float()).to(dtype)
    assert torch.equal(out, want)
    assert lib.raw('mve_clip_embed')(DT[dtype], lib.ptr(ids), lib.ptr(tok), lib.ptr(pos), lib.ptr(out), B, max_pos + 1, C, vocab, max_pos, None) == -1
    assert 'max_pos' in lib.last_error()


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_pool_gathers_the_row_of_both_rules(lib, dtype):
    B, L, C = 4, 21, 72
    x = torch.randn(B, L, C, generator=torch.Generator().manual_seed(7)).to(dtype).cuda()
    ids = torch.randint(3, 50, (B, L), generator=torch.Generator().manual_seed(8), dtype=torch.int32)
    ids[0, 4] = 99                         # the maximum, once
    ids[1, 6] = ids[1, 13] = 99            # a tie: the first position wins
    ids[2, L - 1] = 99                     # at the end
    ids[3, 0] = 99                         # at the start
    dev = ids.cuda()
    out = torch.empty(B, C, dtype=dtype, device='cuda')

    def pool(eos):
        lib.call('mve_clip_pool', DT[dtype], lib.ptr(x), lib.ptr(dev), lib.ptr(out), B, L, C, eos, lib.stream_ptr(x.device))
        torch.cuda.synchronize()
        return out.clone()
    want = ids.argmax(-1)
    assert want.tolist() == [4, 6, L - 1, 0]
    assert torch.equal(pool(2), x[torch.arange(B), want.cuda()])
    # first-match rule: ids above the end token in front of it must not win; item 3 has no end token at all -> position 0
    eos = 60
    ids2 = ids.clone()
    ids2[0, 9] = ids2[0, 15] = eos
    ids2[1, 0] = eos
    ids2[2, L - 1] = eos
    dev.copy_(ids2)
    want2 = (ids2 == eos).int().argmax(-1)
    assert want2.tolist() == [9, 0, L - 1, 0] and not bool((ids2[3] == eos).any())
    assert torch.equal(pool(eos), x[torch.arange(B), want2.cuda()])


@pytest.mark.parametrize('kind,name', [(0, 'quick_gelu'), (1, 'gelu')])
def test_activation(lib, kind, name):
    x = torch.cat([torch.linspace(-8, 8, 4097), torch.zeros(3)]).half().cuda()
    assert bool((x == 0).any()) and float(x.min()) == -8 and float(x.max()) == 8
    y = torch.empty_like(x)
    lib.call('mve_act', 1, kind, lib.ptr(x), lib.ptr(y), x.numel(), lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    xd = x.double().cpu()
    want = xd * torch.sigmoid(1.702 * xd) if kind == 0 else 0.5 * xd * (1 + torch.erf(xd / 2 ** 0.5))
    rel = _rel(y, want)
    print(f'{name}: rel-L2 {rel:.3e}')
    assert rel <= 1e-3, rel
    assert bool((y[x == 0] == 0).all())
    z = x.clone()                          # in place
    lib.call('mve_act', 1, kind, lib.ptr(z), lib.ptr(z), z.numel(), lib.stream_ptr(z.device))
    torch.cuda.synchronize()
    assert torch.equal(z, y)
