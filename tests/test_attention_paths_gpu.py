"""The fused attention at head dims 64 / 80 / 160 on every situation test_attention_d40_transposed_v_kernel puts the d = 40 kernel in.

csrc/attention.hip: one KV segment runs the swizzled instantiations of k_attention2 (V^T store swizzle for d = 64, K + V^T swizzles for d = 80 / 160);
two KV segments run k_attention2<Tag, D, /*SEG2=*/true>, a separate, un-swizzled instantiation (reference-only attention at SD-2.1 head size and at
levels 1 and 2 of SD-1.5).  For d % 16 == 0 the softmax denominator is a separate fp32 chain (l_run), not the ones-row of d = 40.  The executors call
mve_attention_prescaled on column views of packed QKV buffers; so do these tests, next to the plain entry point.

B = 2, heads = 2.  Q | K | V are column views of one packed [B L, 3C] buffer, K2 | V2 of one packed [B Lk2, 2C] buffer.  Lq = 200 leaves 72 rows in the last
128-row query block (a wave with a half-filled fragment); Lk = 200 and Lk2 = 77 put the segment boundary and the tail inside a key fill.  Reference:
float64 softmax attention over the concatenated keys (tests/hard_stats.py); bar: check() of test_unet_ops.py."""
import math

import pytest
import torch

import hard_stats as H
from test_unet_ops import check, rnd

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DIMS = [64, 80, 160]
B, HEADS = 2, 2


def _cat_keys(a, a2, nb, La, La2):
    C = a.shape[1]
    return torch.cat([a.reshape(nb, La, C), a2.reshape(nb, La2, C)], 1).reshape(-1, C)


def _both_forms(name, qb, kvb, kv2, nb, Lq, Lk, Lk2, d, dtype):
    """qb [nb Lq, 3C] (Q = its first C columns), kvb [nb Lk, 3C] (K, V = its columns C:2C, 2C:3C; may be qb itself), kv2 [nb Lk2, 2C] or None --
    CPU tensors of `dtype`.  Runs mve_attention and, with the scale folded into Q, mve_attention_prescaled on the strided views; checks both."""
    from mvedit_amd import ops
    C = HEADS * d
    c = d ** -0.5 * math.log2(math.e)
    q, k, v = qb[:, :C], kvb[:, C:2 * C], kvb[:, 2 * C:]
    kc, vc, Lkc = k, v, Lk
    if Lk2:
        kc, vc, Lkc = _cat_keys(k, kv2[:, :C], nb, Lk, Lk2), _cat_keys(v, kv2[:, C:], nb, Lk, Lk2), Lk + Lk2
    qp = (q.float() * c).to(dtype)
    qpb = qb.clone()
    qpb[:, :C] = qp
    gq, gqp, gkv = qb.cuda(), qpb.cuda(), kvb.cuda()
    g2 = kv2.cuda() if Lk2 else None
    seg2 = dict(k2=g2[:, :C], v2=g2[:, C:], Lk2=Lk2) if Lk2 else {}
    out = ops.attention(gq[:, :C], gkv[:, C:2 * C], gkv[:, 2 * C:], nb, Lq, Lk, HEADS, d, **seg2)
    check(f'{name} d={d}', out, H.attention_ref(q, kc, vc, nb, Lq, Lkc, HEADS, d), dtype, f'{(nb, Lq, Lk, Lk2)}')
    out = ops.attention(gqp[:, :C], gkv[:, C:2 * C], gkv[:, 2 * C:], nb, Lq, Lk, HEADS, d, prescaled=True, **seg2)
    check(f'{name} prescaled d={d}', out, H.attention_ref(qp.float() / c, kc, vc, nb, Lq, Lkc, HEADS, d), dtype, f'{(nb, Lq, Lk, Lk2)}')


def _buffers(Lq, Lk, Lk2, d, dtype, seed=1):
    C = HEADS * d
    qb = rnd((B * Lq, 3 * C), dtype, seed)
    kvb = qb if Lk == Lq else rnd((B * Lk, 3 * C), dtype, seed + 1)
    kv2 = rnd((B * Lk2, 2 * C), dtype, seed + 2) if Lk2 else None
    return qb, kvb, kv2


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('Lq,Lk,Lk2', [(200, 200, 77), (200, 77, 16), (256, 256, 256)])
def test_two_segments_on_packed_views(lib, dtype, d, Lq, Lk, Lk2):
    _both_forms('two segments', *_buffers(Lq, Lk, Lk2, d, dtype), B, Lq, Lk, Lk2, d, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('Lk', [200, 77, 16])
def test_one_segment_swizzled_kernels_on_packed_views(lib, dtype, d, Lk):
    _both_forms('one segment', *_buffers(200, Lk, 0, d, dtype), B, 200, Lk, 0, d, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('Lk2', [0, 77])
def test_spike_forces_a_late_rescale(lib, dtype, d, Lk2):
    """one query scaled x 6 and a key copied from it in the last ragged tile (of segment 2 when there is one): the running maximum jumps there"""
    L, C = 200, HEADS * d
    qb, kvb, kv2 = _buffers(L, L, Lk2, d, dtype)
    qb[5, :C] *= 6
    if Lk2:
        kv2[70, :C] = qb[5, :C]
    else:
        qb[197, C:2 * C] = qb[5, :C]
    _both_forms('spike', qb, kvb, kv2, B, L, L, Lk2, d, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('Lk2', [0, 77])
def test_large_logits_and_offset_values(lib, dtype, d, Lk2):
    """q and k x 3 (sharp rows), V offset by +2: an error of the l_run denominator shows in every output element"""
    L, C = 200, HEADS * d
    qb, kvb, kv2 = _buffers(L, L, Lk2, d, dtype)
    qb[:, :2 * C] = (qb[:, :2 * C].float() * 3).to(dtype)
    qb[:, 2 * C:] = (qb[:, 2 * C:].float() + 2).to(dtype)
    if Lk2:
        kv2[:, :C] = (kv2[:, :C].float() * 3).to(dtype)
        kv2[:, C:] = (kv2[:, C:].float() + 2).to(dtype)
    _both_forms('large logits', qb, kvb, kv2, B, L, L, Lk2, d, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('Lk2', [0, 77])
def test_all_negative_logits(lib, dtype, d, Lk2):
    """every logit far below zero from the first tile on: the denominator must not underflow"""
    L, C = 200, HEADS * d
    qb, kvb, kv2 = _buffers(L, L, Lk2, d, dtype)
    qb[:, :C] = (-(qb[:, :C].float().abs() + 2)).to(dtype)
    qb[:, C:2 * C] = (qb[:, C:2 * C].float().abs() + 2).to(dtype)
    if Lk2:
        kv2[:, :C] = (kv2[:, :C].float().abs() + 2).to(dtype)
    _both_forms('negative logits', qb, kvb, kv2, B, L, L, Lk2, d, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('Lk2', [0, 77])
def test_cross_image_pairing(lib, dtype, d, Lk2):
    """[2b, L, C] viewed as [b, 2L, C] (joint attention over an image pair): 400 queries x 400 (+ 154) keys"""
    L = 200
    qb, kvb, kv2 = _buffers(L, L, Lk2, d, dtype)
    _both_forms('cross-image', qb, kvb, kv2, B // 2, 2 * L, 2 * L, 2 * Lk2, d, dtype)
