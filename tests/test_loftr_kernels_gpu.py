"""The LoFTR matcher kernels (csrc/loftr.hip) through mvedit_amd.matcher.

  stem rows, LeakyReLU, position add, unfold     move data or round one fp32 result: bit-exact against a numpy / torch restatement
  linear attention     (S, D) = (144, 32), (99, 32), (25, 16) -- the two golden token counts (neither a multiple of the 64-row tile, 144 two chunks
                       of 128) and the fine window -- plus (300, 32) (three chunks, a partial tile) against float64 einsum of the formula on the same
                       16-bit inputs.  fp16 <= 1e-3 rel-L2 (the per-kernel bar); bf16 <= 8e-3 (TOL of test_unet_ops.py) on rel-L2 and on
                       max|err| / max|ref|.  Two runs are bit-identical (fixed summation order, no float atomics).  The hard input families
                       (keys far below zero, offsets, outlier channels) and the bound per 16-row block: test_attention_stress_gpu.py.
  dual softmax         on the golden's float64 sim_matrix cast to fp32, against the float64 softmax product.  Bar: 4 x the error of torch's own fp32
                       CPU dual softmax (golden `dsmax_fp32_err`) -- the device exp is another approximation and the sums run in another order.
                       Case B (S = 99) runs in a buffer with leading dimension 104 whose padding holds +1e30 and must give the same bits as the
                       compact buffer.
  selection            crafted fp32 matrices, exact against tests/loftr_rule.py
  fine match           the golden's fine windows rounded to the dtype, against the float64 formula; bar 4 x torch's fp32 error (`fine_fp32_err`)

Measured on an MI355X (rel-L2):
  linear attention (L, S, D)     (144, 144, 32)   (99, 99, 32)   (25, 25, 16)   (70, 300, 32)
    fp16 (bar 1e-3)                2.073e-4         2.122e-4       2.099e-4       2.079e-4
    bf16 (bar 8e-3)                1.672e-3         1.678e-3       1.687e-3       1.644e-3
    KV | Ksum, fp32                1.4e-7           1.3e-7         7.5e-8         1.1e-7
  dual softmax                   case A 5.914e-6 (bar 2.361e-5)      case B 5.580e-6 (bar 2.233e-5)
  fine match, expec_f            A fp16 5.38e-7 (bar 3.31e-6)  A bf16 4.63e-7 (2.88e-6)  B fp16 5.35e-7 (2.48e-6)  B bf16 4.64e-7 (2.97e-6)
  fine match, offsets            A fp16 2.02e-6 (bar 1.21e-5)  A bf16 1.86e-6 (1.01e-5)  B fp16 1.87e-6 (8.01e-6)  B bf16 1.27e-6 (8.99e-6)
(The fine-match dot product is a compensated sum: with a plain fp32 chain over the 128 channels case A fp16 measured 3.34e-6 / 1.23e-5, just past
both bars -- the logits reach 100, where every rounding of the dot product moves exp() by 1e-5.)
"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loftr_rule                                      # noqa: E402
from test_unet_ops import TOL                          # noqa: E402

_spec = importlib.util.spec_from_file_location('make_loftr_golden', os.path.join(HERE, 'golden', 'make_loftr_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope='module')
def mt(lib):
    from mvedit_amd import matcher
    return matcher


@pytest.fixture(scope='module')
def golden():
    return G.load()


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,H,W', [(2, 24, 40), (1, 10, 6)])
def test_stem_rows_are_unfold_of_the_padded_image(mt, B, H, W, dtype):
    px = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(H * W)).to(dtype)
    want = torch.zeros(B * (H // 2) * (W // 2), 56, dtype=dtype)
    want[:, :49] = F.unfold(px.float(), kernel_size=7, stride=2, padding=3).transpose(1, 2).reshape(-1, 49).to(dtype)
    got = mt.stem_rows(px.cuda())
    assert torch.equal(_bits(got.cpu()), _bits(want))


@pytest.mark.parametrize('dtype', DTYPES)
def test_leaky_relu_and_position_add_round_once(mt, dtype):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 1000, 8, generator=g).to(dtype)
    got = mt.leaky_relu(x.cuda().reshape(-1)).cpu()
    want = torch.where(x.float() >= 0, x.float(), x.float() * np.float32(0.01)).to(dtype).reshape(-1)
    assert torch.equal(_bits(got), _bits(want))
    for (h, w, fix) in ((9, 11, False), (12, 12, True)):
        table = mt.position_table(256, h, w, fix).float()                 # float64 on the host, one rounding to the fp32 the kernel adds
        tok = (2 * torch.randn(2, h * w, 256, generator=g)).to(dtype)
        got = mt.pos_add(tok.cuda(), table.cuda()).cpu()
        want = (tok.float() + table[None]).to(dtype)
        assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,L,S,D', [(2, 144, 144, 32), (2, 99, 99, 32), (5, 25, 25, 16), (1, 70, 300, 32)])
def test_linear_attention_against_float64_einsum(mt, B, L, S, D, dtype):
    heads, g = 8, torch.Generator().manual_seed(S + D)
    C = heads * D
    # q | k | v as column blocks of one buffer (leading dimension 3C): the layout a fused projection gives
    qkv_l = torch.randn(B, L, 3 * C, generator=g).to(dtype)
    qkv_s = torch.randn(B, S, 3 * C, generator=g).to(dtype)
    q, k, v = qkv_l[..., :C], qkv_s[..., C:2 * C], qkv_s[..., 2 * C:]
    phi = lambda t: F.elu(t.double()) + 1
    Q, K, V = phi(q).view(B, L, heads, D), phi(k).view(B, S, heads, D), v.double().view(B, S, heads, D)
    KV = torch.einsum('nshd,nshv->nhdv', K, V)
    Z = 1 / (torch.einsum('nlhd,nhd->nlh', Q, K.sum(1)) + 1e-6)
    ref = torch.einsum('nlhd,nhdv,nlh->nlhv', Q, KV, Z).reshape(B, L, C)
    dl, ds = qkv_l.cuda(), qkv_s.cuda()
    run = lambda: mt.linear_attention(dl[..., :C], ds[..., C:2 * C], ds[..., 2 * C:], heads, return_kv=True)
    out, kv = run()
    out2, kv2 = run()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(kv.view(torch.int32), kv2.view(torch.int32)), 'two runs differ'
    kv_ref = torch.cat([KV.reshape(B * heads, D * D), K.sum(1).reshape(B * heads, D)], 1)
    err_kv = float((kv.double().cpu() - kv_ref).norm() / kv_ref.norm())
    err = float((out.double().cpu() - ref).norm() / ref.norm())
    err_max = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f'linear attention {dtype} B {B} L {L} S {S} D {D}: rel-L2 {err:.3e}, max|err| / max|ref| {err_max:.3e} (KV | Ksum in fp32: {err_kv:.3e})')
    assert err == err and err_kv <= 1e-5                               # the fp32 sums themselves: a few fp32 roundings
    if dtype == torch.float16:
        assert err <= 1e-3
    else:
        assert err <= TOL[dtype] and err_max <= TOL[dtype], (err, err_max)


@pytest.mark.parametrize('case', ['A', 'B'])
def test_dual_softmax_on_the_golden_similarity(mt, golden, case):
    sim64 = torch.from_numpy(golden[f'{case}/sim_matrix'])
    ref = F.softmax(sim64, 1) * F.softmax(sim64, 2)
    N, L, S = sim64.shape
    sim = sim64.float().cuda()
    conf = mt.dual_softmax(sim)
    err = float((conf.double().cpu() - ref).norm() / ref.norm())
    bar = 4 * float(golden[f'{case}/dsmax_fp32_err'])
    print(f'dual softmax case {case} [{N}, {L}, {S}]: rel-L2 {err:.3e}, bar {bar:.3e}')
    assert err <= bar
    ld = (S + 7) // 8 * 8 + (8 if S % 8 == 0 else 0)                    # a padded leading dimension, the padding poisoned
    padded = torch.full((N, L, ld), 1e30, dtype=torch.float32, device='cuda')
    padded[..., :S] = sim
    assert torch.equal(mt.dual_softmax(padded, S).view(torch.int32), conf.view(torch.int32)), 'the padded columns entered a softmax'
    # and the selection on the device's own conf_matrix is the rule's
    hw = (G.CASES[case]['H'] // 8, G.CASES[case]['W'] // 8)
    _check_selection(mt, conf, hw, hw, 0.2, 2)


def _check_selection(mt, conf, hw0, hw1, thr, border):
    got = mt.select_matches(conf, hw0, hw1, thr=thr, border=border, scale=8.0)
    b, i, j, c = loftr_rule.coarse_matches(conf.cpu().numpy(), hw0, hw1, thr, border)
    assert got['b_ids'].dtype == torch.int64 and got['mconf'].dtype == torch.float32
    assert np.array_equal(got['b_ids'].cpu().numpy(), b) and np.array_equal(got['i_ids'].cpu().numpy(), i) and np.array_equal(got['j_ids'].cpu().numpy(), j)
    assert np.array_equal(got['mconf'].cpu().numpy().view(np.int32), c.view(np.int32))
    assert np.array_equal(got['mkpts0_c'].cpu().numpy(), loftr_rule.coarse_keypoints(i, hw0[1]).reshape(-1, 2))
    assert np.array_equal(got['mkpts1_c'].cpu().numpy(), loftr_rule.coarse_keypoints(j, hw1[1]).reshape(-1, 2))
    return len(b)


def test_selection_rule_on_crafted_matrices(mt):
    hw0, hw1 = (6, 7), (7, 6)                                            # rectangular, different widths: i and j decode differently
    L, S = 42, 42
    cell0 = lambda y, x: y * hw0[1] + x
    cell1 = lambda y, x: y * hw1[1] + x
    base = torch.full((2, L, S), 0.01, dtype=torch.float32)
    thr = 0.2
    c = base.clone()
    c[0, cell0(2, 2), cell1(3, 3)] = 0.9                                  # a plain match
    c[0, cell0(2, 3), cell1(2, 2)] = thr                                  # equal to thr: not selected
    c[0, cell0(1, 3), cell1(3, 2)] = 0.8                                  # the row cell inside the 2-cell border
    c[0, cell0(3, 3), cell1(5, 3)] = 0.8                                  # the column cell inside the border
    c[0, cell0(3, 2), cell1(4, 2)] = 0.5                                  # a row winner ...
    c[0, cell0(2, 4), cell1(4, 2)] = 0.6                                  # ... that loses its column to this one (which is selected)
    c[0, cell0(3, 4), cell1(2, 3)] = 0.7                                  # an exact tie in one row: the lowest j
    c[0, cell0(3, 4), cell1(4, 3)] = 0.7
    c[1, cell0(3, 3), cell1(2, 2)] = 0.4                                  # the second pair comes after every match of the first
    c[1, cell0(2, 2), cell1(4, 3)] = float(np.nextafter(np.float32(thr), np.float32(1)))      # one step above thr: selected
    n = _check_selection(mt, c.cuda(), hw0, hw1, thr, 2)
    assert n == 5
    got = mt.select_matches(c.cuda(), hw0, hw1, thr=thr, border=2)
    assert got['b_ids'].tolist() == [0, 0, 0, 1, 1]
    assert got['i_ids'].tolist() == [cell0(2, 2), cell0(2, 4), cell0(3, 4), cell0(2, 2), cell0(3, 3)]
    assert got['j_ids'].tolist() == [cell1(3, 3), cell1(4, 2), cell1(2, 3), cell1(4, 3), cell1(2, 2)]
    # border 0: the two border cases come back; nothing above thr: count 0, empty outputs
    assert _check_selection(mt, c.cuda(), hw0, hw1, thr, 0) == 7
    none = mt.select_matches(base.cuda(), hw0, hw1, thr=thr, border=2)
    assert none['b_ids'].shape == (0,) and none['mconf'].shape == (0,) and none['mkpts1_c'].shape == (0, 2)
    assert _check_selection(mt, c.cuda(), hw0, hw1, 2.0, 2) == 0         # thr raised to 2


def test_selection_rule_on_a_random_matrix_with_more_than_one_scan_tile(mt):
    """N * L = 2 * 1200 rows: more than one 2048-row tile of the compaction's scan; many ties (values on a grid of 16 levels)."""
    hw0, hw1 = (30, 40), (10, 12)
    g = torch.Generator().manual_seed(11)
    c = torch.randint(0, 16, (2, 1200, 120), generator=g).float() / 16
    n = _check_selection(mt, c.cuda(), hw0, hw1, 0.2, 2)
    assert n > 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_unfold_gathers_the_windows_with_zeros_outside(mt, dtype):
    N, Hf, Wf, C = 2, 12, 20, 24
    Hc, Wc = Hf // 4, Wf // 4
    feat = torch.randn(N, C, Hf, Wf, generator=torch.Generator().manual_seed(2)).to(dtype)
    # the four corners, an edge and an interior cell, over both images
    b = torch.tensor([0, 0, 1, 1, 0, 1, 1])
    ids = torch.tensor([0, Wc - 1, (Hc - 1) * Wc, Hc * Wc - 1, 1, Wc + 2, 0])
    u = F.unfold(feat.float(), kernel_size=5, stride=4, padding=2).view(N, C, 25, Hc * Wc).permute(0, 3, 2, 1)      # n l ww c
    want = u[b, ids].to(dtype)
    got = mt.unfold_windows(feat.permute(0, 2, 3, 1).contiguous().cuda(), b.cuda(), ids.cuda())
    assert torch.equal(_bits(got.cpu()), _bits(want))
    assert bool((want[0, 0] == 0).all()) and bool((want[3, 24] != 0).any())       # the corner windows do reach outside
    assert mt.unfold_windows(feat.permute(0, 2, 3, 1).contiguous().cuda(), b[:0].cuda(), ids[:0].cuda()).shape == (0, 25, C)


def _fine_reference(w0, w1, mk1_c, radius):
    """FineMatching's formula in w0's dtype (float64 for the yardstick)."""
    C = w0.shape[2]
    heat = torch.softmax(torch.einsum('mc,mrc->mr', w0[:, 12], w1) / C ** .5, 1)
    lin = torch.linspace(-1, 1, 5, dtype=w0.dtype)
    gx, gy = lin.repeat(5), lin.repeat_interleave(5)                     # x fastest
    ex, ey = (heat * gx).sum(1), (heat * gy).sum(1)
    var = torch.stack([(heat * gx ** 2).sum(1) - ex ** 2, (heat * gy ** 2).sum(1) - ey ** 2], 1)
    std = torch.sqrt(var.clamp(min=1e-10)).sum(1)
    coords = torch.stack([ex, ey], 1)
    return torch.cat([coords, std[:, None]], 1), coords * radius


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', ['A', 'B'])
def test_fine_match_on_the_golden_windows(mt, golden, case, dtype):
    w0, w1 = (torch.from_numpy(golden[f'{case}/fine_in{s}']).to(dtype) for s in (0, 1))
    M = w0.shape[0]
    mk1_c = torch.from_numpy(golden[f'{case}/mkpts1_c'][:M]).float()
    radius = 2 * 2.0                                                      # (window // 2) * image / fine map
    expec64, off64 = _fine_reference(w0.double(), w1.double(), mk1_c.double(), radius)
    expec, mk1 = mt.fine_match(w0.cuda(), w1.cuda(), mk1_c.cuda(), radius)
    assert expec.dtype == torch.float32 and mk1.dtype == torch.float32
    off = mk1.double().cpu() - mk1_c.double()
    e_expec = float((expec.double().cpu() - expec64).norm() / expec64.norm())
    e_off = float((off - off64).norm() / off64.norm())
    k = DTYPES.index(dtype)
    bar_expec, bar_off = (4 * float(v) for v in golden[f'{case}/fine_fp32_err'][k])
    # mkpts1_f is a sum with the coarse key point (tens of pixels, exact in fp32): its own rounding, half an fp32 step at the key point per
    # coordinate, enters the offset's error and is no part of torch's figure, which the golden takes on the same sum
    print(f'fine match case {case} {dtype} M {M}: expec_f rel-L2 {e_expec:.3e} (bar {bar_expec:.3e}), offsets {e_off:.3e} (bar {bar_off:.3e})')
    assert e_expec <= bar_expec and e_off <= bar_off
    assert float(off.abs().max()) <= radius


@pytest.mark.parametrize('dtype', DTYPES)
def test_ln_add_on_hard_row_statistics(mt, dtype):
    """mve_loftr_ln_add (y = x + LayerNorm(o), C = 256, 70 rows: a row tail in the last block) on the row statistics of tests/hard_stats.py -- a row mean
    of up to 256 standard deviations, an outlier channel, constant rows, rows whose variance is below eps -- against float64 on the same 16-bit inputs,
    per block of 64 rows, with the per-kernel bar of test_unet_ops.py; leading dimensions wider than C."""
    import hard_stats as H
    from mvedit_amd import _lib
    from mvedit_amd.ops import dt
    M, C, ld = 70, 256, 264
    g = torch.Generator().manual_seed(9)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.2 * torch.randn(C, generator=g)).cuda()
    x = torch.randn(M, C, generator=g).to(dtype).cuda()
    failures = []
    for fam in H.families(dtype):
        o = H.make_rows(fam, M, C, dtype, 7, 'cuda')
        ob, xb = torch.zeros(M, ld, dtype=dtype, device='cuda'), torch.zeros(M, ld, dtype=dtype, device='cuda')
        ob[:, :C], xb[:, :C] = o.to(dtype), x
        y = torch.full((M, ld), 7.0, dtype=dtype, device='cuda')
        _lib.call('mve_loftr_ln_add', dt(dtype), _lib.ptr(ob), ld, _lib.ptr(xb), ld, _lib.ptr(y), ld, M, C, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, _lib.stream_ptr(y.device))
        assert bool((y[:, C:] == 7.0).all()), 'the kernel wrote outside its columns'
        try:
            H.check_rows('loftr_ln_add', fam, y[:, :C], x.double() + H.layernorm_ref(o, gamma, beta, 1e-5), dtype)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, '\n'.join(failures)
