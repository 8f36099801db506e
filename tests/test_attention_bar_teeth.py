"""The bar of test_attention_stress_gpu.py has room for a correct kernel and none for a wrong one -- shown on the CPU, without a kernel.

The attention kernels of csrc/clip_text.hip, csrc/sam.hip, csrc/loftr.hip (and csrc/attention.hip for head dims 64 / 80) share one rounding design:
fp32 logits and bias, P rounded to the storage type for the P V product, the denominator summed over the unrounded p, one rounding of the output;
mve_attention_relpos and mve_attention walk the keys in tiles with the online-softmax recurrence (running maximum, alpha = exp(m_old - m_new) applied to
the sum and to the accumulator); the linear attention keeps fp32 sums of phi(k) v and phi(k) with phi(x) = x > 0 ? x + 1 : expf(x).  Here that design
is restated in plain torch fp32 and checked, like the kernels, with hard_stats.check_rows(block=16) against the float64 references on every (shape,
family, dtype) of hard_stats.attn_case:

(a) the correct emulation passes everywhere: the chosen inputs leave the design room under TOL (1e-3 fp16, 8e-3 bf16).  Its worst ratio is printed and
    asserted to stay under 0.75 x TOL, so that a kernel which misses the bar where this emulation does not has a defect and not an unlucky input.
    Measured: the worst of max|err| / max|ref| and rel-L2 over all cases is 0.49 x TOL in both types (linear attention, v+32: fp16 at (70, 300, 32),
    bf16 at (99, 99, 32)); the worst softmax-attention case is 0.48 x TOL.
(b) each wrong variant is over the bar on the family named for it, on every shape it applies to and in both storage types (VARIANTS below; the test
    prints the ratio of every other family as well):
      causal mask key < query            randn       every row loses its own key; row 1 is left with key 0 alone
      padded key in the sum              negative    relpos / plain: a zero-padded key has logit 0 (+ bias), far above every real one
      padded key in the maximum          negative    the maximum becomes the padded logit.  A softmax does not depend on the value subtracted until
                                                     p underflows the type P is stored in: fp16 below 6e-8 (a logit 16.6 under the maximum) -- every
                                                     shape; bf16 below 9e-41 (92 under) -- the head_dim 80 shapes, whose logits reach -100; at head_dim
                                                     64 (logits around -80) the bf16 result is right and nothing is there to be caught
      accumulator not rescaled           spike       online softmax: the maximum jumps at the copied key in the last tile (the grids of more than 64
                                                     keys: 5 x 13, 1 x 70, 14 x 14)
      both bias terms dropped            randn, tables x1
      height-table index shifted by one  tables x1
      height and width tables swapped    tables x1   non-square grids (6 x 10, 10 x 6, 5 x 13); indices clamped into the other table
      elu(x) + 1 evaluated in fp32       keys-20     phi(k) = exp(-20) is lost against the 1 of elu + 1: the output is 0
    A causal kernel that drops `key < L` is not a wrong variant: key <= query < L already implies it."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hard_stats as H  # noqa: E402
import sam_rule  # noqa: E402
from test_unet_ops import TOL  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
B, HEADS = H.ATTN_B, H.ATTN_HEADS
NEG = -3.0e38


def _split(t, L, d):
    return t.float().reshape(B, L, HEADS, d).transpose(1, 2)


def _merge(o, dtype):
    return o.to(dtype).transpose(1, 2).reshape(o.shape[0] * o.shape[2], -1)


def _pad_keys(t, n):
    return F.pad(t, (0, 0, 0, n))


def _softmax_pv(s, v, vis_max, vis_sum, dtype, tile, rescale=True):
    """s [.., Lq, Lk] fp32 logits, v [.., Lk, d] fp32; vis_max / vis_sum [Lq, Lk] or [Lk]: the keys that enter the maximum / get a probability.
    tile None: two passes (maximum, then exp and sum).  tile n: the online recurrence over n keys at a time."""
    Lk = s.shape[-1]
    vis_max, vis_sum = vis_max.expand(s.shape[-2:]), vis_sum.expand(s.shape[-2:])
    m = torch.full(s.shape[:-1], NEG)
    total = torch.zeros(s.shape[:-1])
    acc = torch.zeros(s.shape[:-1] + (v.shape[-1],))
    for k0 in range(0, Lk, tile or Lk):
        sl = slice(k0, min(Lk, k0 + (tile or Lk)))
        st = s[..., sl]
        mn = torch.maximum(m, torch.where(vis_max[:, sl], st, torch.tensor(NEG)).max(-1).values)
        alpha = torch.exp(m - mn)
        m = mn
        p = torch.where(vis_sum[:, sl], torch.exp(st - m[..., None]), torch.tensor(0.0))
        total = total * alpha + p.sum(-1)
        if rescale:
            acc = acc * alpha[..., None]
        acc = acc + p.to(dtype).float() @ v[..., sl, :]
    return acc / total[..., None]


def emulate_causal(qkv, L, dtype, variant=None):
    d, C = 64, HEADS * 64
    q, k, v = (_split(qkv[:, i * C:(i + 1) * C], L, d) for i in range(3))
    s = q @ k.transpose(-1, -2) * d ** -0.5
    i = torch.arange(L)
    vis = i[None, :] <= i[:, None]
    if variant == 'mask key < query':
        vis = (i[None, :] < i[:, None]) | (i[None, :] == 0)              # (row 0 keeps key 0: the variant is wrong, not undefined)
    return _merge(_softmax_pv(s, v, vis, vis, dtype, None), dtype)


def emulate_relpos(qkv, rel_h, rel_w, gh, gw, d, dtype, variant=None, tile=64):
    """rel_h / rel_w None: mve_attention (no bias)"""
    L, C = gh * gw, HEADS * d
    q, k, v = (_split(qkv[:, i * C:(i + 1) * C], L, d) for i in range(3))
    pad = -L % tile
    k, v = _pad_keys(k, pad), _pad_keys(v, pad)
    s = q @ k.transpose(-1, -2) * d ** -0.5
    if rel_h is not None and variant != 'no bias':
        qi, ki = torch.arange(L), torch.arange(L + pad).clamp(max=L - 1)      # a padded key takes the bias of key L - 1
        th, tw = q @ rel_h.float().t(), q @ rel_w.float().t()
        jh, jw = qi[:, None] // gw - ki[None, :] // gw + gh - 1, qi[:, None] % gw - ki[None, :] % gw + gw - 1
        if variant == 'h index + 1':
            jh = (jh + 1).clamp(max=2 * gh - 2)
        if variant == 'tables swapped':
            th, tw = tw, th
            jh, jw = (jh - gh + gw).clamp(0, 2 * gw - 2), (jw - gw + gh).clamp(0, 2 * gh - 2)
        s = s + th.gather(-1, jh.expand(B, HEADS, -1, -1)) + tw.gather(-1, jw.expand(B, HEADS, -1, -1))
    real = torch.arange(L + pad) < L
    every = torch.ones_like(real)
    vis_max, vis_sum = (every if variant == 'pad in max' else real), (every if variant == 'pad in sum' else real)
    return _merge(_softmax_pv(s, v, vis_max, vis_sum, dtype, tile, rescale=variant != 'no rescale'), dtype)


def emulate_linear(ql, ks, L, S, D, dtype, variant=None):
    C = HEADS * D
    phi = (lambda t: F.elu(t) + 1) if variant == 'elu + 1 in fp32' else (lambda t: torch.where(t > 0, t + 1, torch.exp(t)))
    Q = phi(ql[:, :C].float()).reshape(B, L, HEADS, D)
    K, V = phi(ks[:, C:2 * C].float()).reshape(B, S, HEADS, D), ks[:, 2 * C:].float().reshape(B, S, HEADS, D)
    KV = torch.einsum('nshd,nshv->nhdv', K, V)
    den = torch.einsum('nlhd,nhd->nlh', Q, K.sum(1)) + torch.tensor(1e-6)
    return (torch.einsum('nlhd,nhdv->nlhv', Q, KV) / den[..., None]).to(dtype).reshape(B * L, C)


def _cases(kind):
    """(shape, families) of a kernel"""
    return {'plain': [(s, H.PLAIN_FAMILIES) for s in H.PLAIN_SHAPES], 'causal': [(s, H.CAUSAL_FAMILIES) for s in H.CAUSAL_L],
            'relpos': [(s, H.RELPOS_FAMILIES) for s in H.RELPOS_SHAPES], 'linear': [(s, H.LINATTN_FAMILIES) for s in H.LINATTN_SHAPES]}[kind]


def _emulate(kind, shape, family, dtype, variant=None):
    """-> (emulated output, float64 reference)"""
    c = H.attn_case(kind, shape, family, dtype)
    if kind == 'plain':
        return emulate_relpos(c[0], None, None, 1, shape[0], shape[1], dtype, variant), c[1]
    if kind == 'causal':
        return emulate_causal(c[0], shape, dtype, variant), c[1]
    if kind == 'relpos':
        return emulate_relpos(c[0], c[1], c[2], *shape, dtype, variant), c[3]
    return emulate_linear(c[0], c[1], *shape, dtype, variant), c[2]


def _ratio(kind, shape, family, dtype, variant=None):
    """worst of max|err| / max|ref| and rel-L2 over the 16-row blocks, relative to TOL; inf for a non-finite output"""
    got, ref = _emulate(kind, shape, family, dtype, variant)
    try:
        return max(H.check_rows(f'{kind} {shape} {variant or "emulation"}', family, got, ref, dtype, block=16, tol=float('inf'))) / TOL[dtype]
    except AssertionError:
        return float('inf')


def test_relpos_reference_agrees_with_the_sam_rule():
    NS, gh, gw, heads, d = 2, 3, 5, 2, 8
    L, C = gh * gw, heads * d
    qkv = H.attn_qkv('randn', NS, L, heads, d, torch.float16, 3)
    rel_h, rel_w = H.relpos_tables('tables x1', gh, gw, d, torch.float16, 4)
    q, k, v = (qkv[:, i * C:(i + 1) * C] for i in range(3))
    rule = sam_rule.relpos_attention(*(t.double().numpy().reshape(NS, L, heads, d) for t in (q, k, v)), rel_h.double().numpy(), rel_w.double().numpy(),
                                     gh, gw, d ** -0.5).reshape(NS * L, C)
    ref = H.relpos_attention_ref(q, k, v, rel_h, rel_w, NS, gh, gw, heads, d).numpy()
    assert np.abs(ref - rule).max() <= 1e-12 * np.abs(rule).max()
    # and without the bias it is the plain reference
    zero = torch.zeros_like
    assert torch.equal(H.relpos_attention_ref(q, k, v, zero(rel_h), zero(rel_w), NS, gh, gw, heads, d), H.attention_ref(q, k, v, NS, L, L, heads, d))


def test_references_on_a_case_done_by_hand():
    """two keys, one head: causal row 0 is v0, row 1 the softmax mix; linear attention with k far below zero keeps exp(k)"""
    q, k, v = torch.tensor([[1.0, 0.0], [0.0, 2.0]]), torch.tensor([[1.0, 0.0], [0.0, 1.0]]), torch.tensor([[1.0, 10.0], [3.0, 30.0]])
    out = H.causal_attention_ref(q, k, v, 1, 2, 1, 2, scale=1.0)
    w = 1 / (1 + np.exp(2.0))
    assert torch.allclose(out, torch.tensor([[1.0, 10.0], [w * 1 + (1 - w) * 3, w * 10 + (1 - w) * 30]], dtype=torch.float64), rtol=1e-14)
    out, KV, Ksum = H.linear_attention_ref(torch.tensor([[0.0, 1.0]]), torch.tensor([[-20.0, -20.0]]), torch.tensor([[5.0, 7.0]]), 1, 1, 1, 1, 2, eps=0.0)
    assert torch.allclose(out, torch.tensor([[5.0, 7.0]], dtype=torch.float64), rtol=1e-14) and float(Ksum[0, 0]) == float(np.exp(-20.0))


@pytest.mark.parametrize('dtype', DTYPES)
def test_correct_emulation_passes_the_bar(dtype):
    worst = (0.0, None)
    for kind in ('plain', 'causal', 'relpos', 'linear'):
        for shape, fams in _cases(kind):
            for fam in fams:
                got, ref = _emulate(kind, shape, fam, dtype)
                r = max(H.check_rows(f'{kind} {shape} emulation', fam, got, ref, dtype, block=16)) / TOL[dtype]
                worst = max(worst, (r, (kind, shape, fam)))
    print(f'\ncorrect emulation, {dtype}: worst ratio {worst[0]:.2f} x TOL at {worst[1]}')
    assert worst[0] <= 0.75, worst


# variant -> (kernel, the families it is named for, the shapes it applies to or None for all)
NONSQUARE = tuple(s for s in H.RELPOS_SHAPES if s[0] != s[1] and min(s[:2]) > 1)
D80 = tuple(s for s in H.RELPOS_SHAPES if s[2] == 80)
VARIANTS = {
    'mask key < query': ('causal', ('randn',), None),
    'pad in sum': ('relpos', ('negative',), None),
    'pad in max': ('relpos', ('negative',), {torch.float16: None, torch.bfloat16: D80}),
    'no rescale': ('relpos', ('spike',), tuple(s for s in H.RELPOS_SHAPES if s[0] * s[1] > 64)),
    'no bias': ('relpos', ('randn', 'tables x1'), None),
    'h index + 1': ('relpos', ('tables x1',), tuple(s for s in H.RELPOS_SHAPES if s[0] > 1)),
    'tables swapped': ('relpos', ('tables x1',), NONSQUARE),
    'elu + 1 in fp32': ('linear', ('keys-20',), None),
}
PLAIN_VARIANTS = {'pad in sum': ('randn',), 'no rescale': ('spike',)}       # mve_attention's families have no `negative`: see the docstring of the test


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_wrong_variant_fails_the_bar(variant, dtype):
    """on every shape the variant applies to, each family named for it is over the bar"""
    kind, named, shapes = VARIANTS[variant]
    shapes = shapes[dtype] if isinstance(shapes, dict) else shapes
    report = []
    for shape, fams in _cases(kind):
        if shapes is not None and shape not in shapes:
            continue
        caught = {fam: _ratio(kind, shape, fam, dtype, variant) for fam in fams}
        report.append(f'  {kind} {shape}: ' + ', '.join(f'{f} {r:.1f}' for f, r in caught.items()))
        for fam in named:
            assert caught[fam] > 1.0, f'{variant} / {kind} {shape} / {fam} / {dtype}: {caught[fam]:.2f} x TOL passes the bar'
    print(f'\n{variant}, {dtype}: worst ratio to TOL per family\n' + '\n'.join(report))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', list(PLAIN_VARIANTS))
def test_wrong_variant_of_the_plain_attention_fails_the_bar(variant, dtype):
    """mve_attention runs randn / spike / large+offset only (its `negative` cases are in test_attention_paths_gpu.py): a padded key in the sum shows on
    randn at both lengths (63 and 63 padded keys of logit 0 next to 65 and 257 real ones), a missing rescale on spike"""
    for shape, _ in _cases('plain'):
        for fam in PLAIN_VARIANTS[variant]:
            r = _ratio('plain', shape, fam, dtype, variant)
            assert r > 1.0, f'{variant} / plain {shape} / {fam} / {dtype}: {r:.2f} x TOL passes the bar'
