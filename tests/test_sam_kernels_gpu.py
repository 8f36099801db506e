"""The SAM image encoder's kernels (csrc/sam.hip) through ctypes, against the numpy rule of tests/sam_rule.py.

mve_attention_relpos: fp16 is held to the per-kernel bar of 1e-3 rel-L2 against the float64 einsum statement of

    softmax_k( scale q.k + q.Rh[qh - kh + gh - 1] + q.Rw[qw - kw + gw - 1] ) v

on the same 16-bit-rounded inputs; bf16 is held to TOL of tests/test_unet_ops.py (8e-3) on rel-L2 and on max|err| / max|ref| (as the other attention
kernels; the hard input families and the bound per 16-row block are in tests/test_attention_stress_gpu.py).  mve_sam_window_partition /
mve_sam_window_unpartition move data and mve_sam_pos_add rounds one fp32 sum: bit-exact.

Measured on an MI355X (rel-L2 against float64):

    NS x (gh x gw), heads, head_dim      fp16          bf16
    3 x (14 x 14), 2, 64                 2.246e-04     1.778e-03
    1 x (20 x 20), 2, 80                 2.232e-04     1.772e-03
    2 x ( 6 x 10), 1, 64                 2.253e-04     1.779e-03
    1 x (64 x 64), 1, 80                 2.228e-04     1.783e-03
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sam_rule as R  # noqa: E402
from test_unet_ops import TOL  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {torch.float16: 1, torch.bfloat16: 2}


def _inputs(NS, gh, gw, heads, hd, dtype):
    g = torch.Generator().manual_seed(1000 * gh + 10 * gw + hd + NS)
    C = heads * hd
    qkv = (torch.randn(NS * gh * gw, 3 * C, generator=g) * 1.5).to(dtype)
    rel_h = (torch.randn(2 * gh - 1, hd, generator=g) * 0.1).to(dtype)       # q . R of order 1: next to logits of order 1.5^2, the bias decides the argmax often
    rel_w = (torch.randn(2 * gw - 1, hd, generator=g) * 0.1).to(dtype)
    return qkv, rel_h, rel_w


def _run(lib, dtype, qkv, rel_h, rel_w, NS, gh, gw, heads, hd):
    C = heads * hd
    out = torch.full((NS * gh * gw, C), float('nan'), dtype=dtype, device='cuda')
    lib.call('mve_attention_relpos', DT[dtype], lib.ptr(qkv), 3 * C, lib.ptr(qkv[:, C:]), 3 * C, lib.ptr(qkv[:, 2 * C:]), 3 * C, lib.ptr(rel_h), lib.ptr(rel_w),
             lib.ptr(out), C, NS, gh, gw, heads, hd, ctypes.c_float(hd ** -0.5), lib.stream_ptr(out.device))
    torch.cuda.synchronize()
    return out


def _reference(qkv, rel_h, rel_w, NS, gh, gw, heads, hd):
    C = heads * hd
    q, k, v = (qkv[:, i * C:(i + 1) * C].double().numpy().reshape(NS, gh * gw, heads, hd) for i in range(3))
    return R.relpos_attention(q, k, v, rel_h.double().numpy(), rel_w.double().numpy(), gh, gw, hd ** -0.5).reshape(NS * gh * gw, C)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('NS,gh,gw,heads,hd', [(3, 14, 14, 2, 64), (1, 20, 20, 2, 80), (2, 6, 10, 1, 64), (1, 64, 64, 1, 80)])
def test_attention_relpos_against_the_float64_rule(lib, NS, gh, gw, heads, hd, dtype):
    """The production window (196 keys: three full 64-key tiles and a tail of 4), 400 keys at head_dim 80, a non-square grid (k / gw against k % gw)
    and the production global grid (4096 keys, 127-row tables).  fp16: rel-L2 <= 1e-3.  bf16: rel-L2 and max|err| / max|ref| <= 8e-3 (TOL).  In
    both types the output is far from the same attention without the two bias terms, which itself is far from the rule."""
    qkv, rel_h, rel_w = _inputs(NS, gh, gw, heads, hd, dtype)
    d = [t.cuda() for t in (qkv, rel_h, rel_w)]
    out = _run(lib, dtype, *d, NS, gh, gw, heads, hd)
    assert torch.isfinite(out.float()).all()
    ref = _reference(qkv, rel_h, rel_w, NS, gh, gw, heads, hd)
    got = out.double().cpu().numpy()
    rel, rmax = float(np.linalg.norm(got - ref) / np.linalg.norm(ref)), float(np.abs(got - ref).max() / np.abs(ref).max())
    # the same inputs without the two bias terms are a different function: the bar is not met by a kernel that drops them
    flat = R.relpos_attention(*(qkv[:, i * heads * hd:(i + 1) * heads * hd].double().numpy().reshape(NS, gh * gw, heads, hd) for i in range(3)),
                              np.zeros((2 * gh - 1, hd)), np.zeros((2 * gw - 1, hd)), gh, gw, hd ** -0.5).reshape(ref.shape) if gh * gw <= 400 else None
    print(f'attention_relpos {dtype} NS={NS} grid={gh}x{gw} heads={heads} head_dim={hd}: rel-L2 {rel:.3e}, max|err| / max|ref| {rmax:.3e}')
    if flat is not None:
        assert np.linalg.norm(flat - ref) / np.linalg.norm(ref) > 0.1
        assert np.linalg.norm(got - flat) / np.linalg.norm(flat) > 0.1         # in both types: the kernel does not compute the bias-free function
    if dtype == torch.float16:
        assert rel <= 1e-3, rel
    else:
        assert rel <= TOL[dtype] and rmax <= TOL[dtype], (rel, rmax)
    assert torch.equal(out, _run(lib, dtype, *d, NS, gh, gw, heads, hd))                  # two runs give the same bits


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_attention_relpos_sequence_does_not_depend_on_ns(lib, dtype):
    NS, gh, gw, heads, hd = 3, 14, 14, 2, 64
    qkv, rel_h, rel_w = (t.cuda() for t in _inputs(NS, gh, gw, heads, hd, dtype))
    out = _run(lib, dtype, qkv, rel_h, rel_w, NS, gh, gw, heads, hd)
    L = gh * gw
    for s in range(NS):
        alone = _run(lib, dtype, qkv[s * L:(s + 1) * L], rel_h, rel_w, 1, gh, gw, heads, hd)
        assert torch.equal(alone, out[s * L:(s + 1) * L]), s
    two = _run(lib, dtype, qkv[L:], rel_h, rel_w, 2, gh, gw, heads, hd)
    assert torch.equal(two, out[L:])


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('G,w', [(16, 14), (20, 14), (28, 14)])
def test_window_partition_and_unpartition_are_bit_exact(lib, G, w, dtype):
    """(16, 14) and (20, 14) pad to 28 (2 x 2 windows, the right and bottom ones mostly padding); (28, 14) has no padding.  Pad rows are exactly
    zero whatever the buffer held; un-partition restores the map bit for bit and never reads a pad row (they are poisoned with NaN first)."""
    B, C = 2, 24
    nw = -(-G // w)
    x = torch.randn(B, G, G, C, generator=torch.Generator().manual_seed(G)).to(dtype)
    want = torch.from_numpy(R.window_partition(x.view(torch.int16).numpy(), w))          # the rule on the bit patterns: +0.0 is the all-zero pattern
    win = torch.full((B * nw * nw, w * w, C), float('nan'), dtype=dtype, device='cuda')
    dx = x.cuda()
    lib.call('mve_sam_window_partition', DT[dtype], lib.ptr(dx), B, G, C, w, lib.ptr(win), lib.stream_ptr(win.device))
    torch.cuda.synchronize()
    assert torch.equal(win.cpu().view(torch.int16), want)
    pad = torch.from_numpy(R.window_partition(np.ones((B, G, G, 1)), w))[..., 0] == 0       # [windows, w * w]: True on the pad rows
    assert int(pad.sum()) == B * ((nw * w) ** 2 - G * G) and not win.cpu().view(torch.int16)[pad].any()
    poisoned = win.clone()
    poisoned[pad.cuda()] = float('nan')
    back = torch.full((B, G, G, C), float('nan'), dtype=dtype, device='cuda')
    lib.call('mve_sam_window_unpartition', DT[dtype], lib.ptr(poisoned), B, G, C, w, lib.ptr(back), lib.stream_ptr(back.device))
    torch.cuda.synchronize()
    assert torch.equal(back.cpu().view(torch.int16), x.view(torch.int16))
    assert np.array_equal(R.window_unpartition(want.numpy(), B, G, w), x.view(torch.int16).numpy())


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_pos_add_is_one_rounded_fp32_sum(lib, dtype):
    B, HW, C = 3, 20, 136
    g = torch.Generator().manual_seed(7)
    x, pos = torch.randn(B, HW, C, generator=g).to(dtype).cuda(), torch.randn(HW, C, generator=g).to(dtype).cuda()
    out = torch.full((B, HW, C), float('nan'), dtype=dtype, device='cuda')
    lib.call('mve_sam_pos_add', DT[dtype], lib.ptr(x), lib.ptr(pos), lib.ptr(out), B, HW, C, lib.stream_ptr(out.device))
    torch.cuda.synchronize()
    assert torch.equal(out, (x.float() + pos.float()).to(dtype))
