"""mve_attention_causal, mve_attention_relpos, mve_linattn_kv / _apply and mve_attention at the vision shapes on hard statistics, fp16 and bf16.

The kernel tests of these four (test_clip_text_kernels_gpu.py, test_sam_kernels_gpu.py, test_loftr_kernels_gpu.py, test_clip_vision_kernels_gpu.py)
run `randn * 1.5` and hold one global rel-L2.  Here every (kernel, shape, family) of tests/hard_stats.py (attn_case: the families are described
there) runs in both storage types against the float64 reference of the same rounded inputs, and the bar of tests/test_unet_ops.py (TOL: 1e-3 fp16,
8e-3 bf16) is applied to max|err| / max|ref| and to the rel-L2 of every block of 16 output rows -- one wave's query tile in mve_attention_causal and
mve_attention_relpos -- through hard_stats.check_rows(block=16).  tests/test_attention_bar_teeth.py shows on the CPU that the kernels' rounding design
passes this bar on these inputs with 2 x room and that seven wrong variants of it (one of them in two forms) do not.

B (or NS) = 2, heads = 2.  Q | K | V are column views of packed [rows, 3 C] buffers (linear attention: Q of one, K | V of another).  The output goes
into a buffer with ldo = C + 8 and one guard row before and after; the guard rows and the 8 extra columns hold a sentinel that must survive.

  causal (d = 64)        L = 17 (one key in the second 16-key tile, one row in the second query tile), 77 (production; ragged tile 4),
                         128 (every wave runs both iterations, odd and even query tiles)
  rel-pos (gh x gw, d)   6 x 10, 64; 10 x 6, 80 (k / gw against k % gw, zero-padded columns 80..95); 5 x 13, 64 (65 keys: one key in the second
                         tile, one query in the second query tile); 1 x 70, 80 (a one-row height table); 14 x 14, 64 (the production window)
  linear (L, S, D)       (70, 300, 32) three chunks and a partial tile; (25, 25, 16); (99, 99, 32).  KV | Ksum, and Ksum alone, are within 1e-5
                         rel-L2 of float64
  mve_attention (L, d)   (65, 64), (257, 80) with randn, spike, large+offset

Worst max|err| / max|ref| and rel-L2 over the 16-row blocks (the larger of the two) per (kernel and shape, family, dtype), printed once per run
(pytest -s), measured on an MI355X.  Every figure is between 0.28 and 0.49 of its bar; the CPU emulation of the design measures 0.49.  Wall time of
this file: 26 tests in 2.7 s, the float64 references on the CPU included (the slowest test, 0.46 s, carries the first launch).
  path                                           dtype        randn     spike large+offset  negative      sink tables x1 tables x1 neg
  attention L=257 d=80                           bfloat16   3.3e-03   3.5e-03      3.2e-03         -         -         -             -
  attention L=257 d=80                           float16    4.5e-04   4.4e-04      3.7e-04         -         -         -             -
  attention L=65 d=64                            bfloat16   2.7e-03   3.4e-03      2.7e-03         -         -         -             -
  attention L=65 d=64                            float16    3.5e-04   4.2e-04      4.2e-04         -         -         -             -
  causal L=128                                   bfloat16   2.9e-03   3.2e-03      2.7e-03   3.3e-03   3.9e-03         -             -
  causal L=128                                   float16    3.9e-04   4.1e-04      3.3e-04   4.3e-04   4.8e-04         -             -
  causal L=17                                    bfloat16   3.2e-03   3.2e-03      2.5e-03   2.9e-03   2.6e-03         -             -
  causal L=17                                    float16    3.3e-04   3.3e-04      3.2e-04   3.6e-04   3.3e-04         -             -
  causal L=77                                    bfloat16   2.6e-03   2.6e-03      2.6e-03   2.5e-03   3.1e-03         -             -
  causal L=77                                    float16    3.9e-04   3.9e-04      3.3e-04   3.2e-04   4.0e-04         -             -
  relpos 10x6 d=80                               bfloat16   3.4e-03   3.3e-03      3.7e-03   3.4e-03         -   2.6e-03       2.9e-03
  relpos 10x6 d=80                               float16    4.3e-04   4.0e-04      3.9e-04   4.4e-04         -   3.7e-04       4.0e-04
  relpos 14x14 d=64                              bfloat16   3.7e-03   3.2e-03      2.7e-03   3.6e-03         -   3.2e-03       2.8e-03
  relpos 14x14 d=64                              float16    3.9e-04   4.3e-04      3.7e-04   4.1e-04         -   4.0e-04       4.1e-04
  relpos 1x70 d=80                               bfloat16   2.4e-03   3.5e-03      2.8e-03   3.4e-03         -   3.0e-03       3.0e-03
  relpos 1x70 d=80                               float16    3.6e-04   4.5e-04      3.9e-04   4.2e-04         -   4.0e-04       3.8e-04
  relpos 5x13 d=64                               bfloat16   2.7e-03   2.5e-03      2.7e-03   3.2e-03         -   2.7e-03       3.3e-03
  relpos 5x13 d=64                               float16    3.9e-04   4.3e-04      3.4e-04   4.0e-04         -   3.6e-04       4.1e-04
  relpos 6x10 d=64                               bfloat16   2.8e-03   2.5e-03      2.9e-03   3.2e-03         -   3.2e-03       2.9e-03
  relpos 6x10 d=64                               float16    4.0e-04   4.6e-04      3.3e-04   3.8e-04         -   4.3e-04       3.8e-04

  path                                           dtype        randn   keys-12   keys-20     qkv+8      v+32   outlier
  linear (25,25,16)                              bfloat16   2.5e-03   2.5e-03   2.3e-03   3.7e-03   3.9e-03   3.0e-03
  linear (25,25,16)                              float16    3.1e-04   3.2e-04   2.8e-04   4.7e-04   4.8e-04   3.6e-04
  linear (70,300,32)                             bfloat16   3.4e-03   3.5e-03   3.5e-03   3.8e-03   2.2e-03   2.8e-03
  linear (70,300,32)                             float16    4.3e-04   4.4e-04   4.5e-04   4.8e-04   4.9e-04   3.5e-04
  linear (99,99,32)                              bfloat16   3.5e-03   3.5e-03   2.9e-03   3.8e-03   3.9e-03   2.5e-03
  linear (99,99,32)                              float16    4.3e-04   4.3e-04   4.5e-04   4.8e-04   4.9e-04   3.0e-04
"""
import pytest
import torch

import hard_stats as H

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
B, HEADS = H.ATTN_B, H.ATTN_HEADS
SENTINEL = 7.0
WORST, WORST_LINEAR = H.Worst(), H.Worst()


@pytest.fixture(scope='module', autouse=True)
def _print_worst():
    yield
    if WORST.t or WORST_LINEAR.t:
        print('\nworst ratio per (kernel and shape, family, dtype):\n' + WORST.table(H.ATTN_FAMILIES) + '\n' + WORST_LINEAR.table(H.LINATTN_FAMILIES))


def _out(rows, C, dtype):
    """-> (the whole buffer [rows + 2, C + 8] filled with the sentinel, the view [rows, C + 8] the kernel gets)"""
    buf = torch.full((rows + 2, C + 8), SENTINEL, dtype=dtype, device='cuda')
    return buf, buf[1:rows + 1]


def _take(buf, rows, C, what):
    torch.cuda.synchronize()
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[rows + 1] == SENTINEL).all()), f'{what}: a guard row was written'
    assert bool((buf[1:rows + 1, C:] == SENTINEL).all()), f'{what}: the kernel wrote outside its columns'
    return buf[1:rows + 1, :C].cpu()


def _check(path, fam, dtype, got, ref, failures, worst=WORST):
    try:
        worst.add(path, fam, dtype, H.check_rows(path, fam, got, ref, dtype, block=16))
    except AssertionError as e:
        failures.append(str(e))


def _raise_all(failures):
    if failures:
        raise AssertionError(f'{len(failures)} failure(s):\n' + '\n'.join(failures))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('L', H.CAUSAL_L)
def test_causal_attention_families(lib, dtype, L):
    from mvedit_amd.ops import dt
    d, C, failures = 64, HEADS * 64, []
    for fam in H.CAUSAL_FAMILIES:
        qkv, ref = H.attn_case('causal', L, fam, dtype)
        g = qkv.cuda()
        buf, out = _out(B * L, C, dtype)
        lib.call('mve_attention_causal', dt(dtype), lib.ptr(g), 3 * C, lib.ptr(g[:, C:]), 3 * C, lib.ptr(g[:, 2 * C:]), 3 * C, lib.ptr(out), C + 8, B, L, HEADS, d,
                 d ** -0.5, lib.stream_ptr(g.device))
        _check(f'causal L={L}', fam, dtype, _take(buf, B * L, C, f'causal L={L} / {fam}'), ref, failures)
    _raise_all(failures)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('gh,gw,d', H.RELPOS_SHAPES)
def test_relpos_attention_families(lib, dtype, gh, gw, d):
    from mvedit_amd.ops import dt
    L, C, failures = gh * gw, HEADS * d, []
    for fam in H.RELPOS_FAMILIES:
        qkv, rel_h, rel_w, ref = H.attn_case('relpos', (gh, gw, d), fam, dtype)
        g, th, tw = qkv.cuda(), rel_h.cuda(), rel_w.cuda()
        buf, out = _out(B * L, C, dtype)
        lib.call('mve_attention_relpos', dt(dtype), lib.ptr(g), 3 * C, lib.ptr(g[:, C:]), 3 * C, lib.ptr(g[:, 2 * C:]), 3 * C, lib.ptr(th), lib.ptr(tw),
                 lib.ptr(out), C + 8, B, gh, gw, HEADS, d, d ** -0.5, lib.stream_ptr(g.device))
        _check(f'relpos {gh}x{gw} d={d}', fam, dtype, _take(buf, B * L, C, f'relpos {gh}x{gw} d={d} / {fam}'), ref, failures)
    _raise_all(failures)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('L,d', H.PLAIN_SHAPES)
def test_attention_families_at_the_vision_shapes(lib, dtype, L, d):
    from mvedit_amd.ops import dt
    C, failures = HEADS * d, []
    for fam in H.PLAIN_FAMILIES:
        qkv, ref = H.attn_case('plain', (L, d), fam, dtype)
        g = qkv.cuda()
        buf, out = _out(B * L, C, dtype)
        lib.call('mve_attention', dt(dtype), lib.ptr(g), 3 * C, lib.ptr(g[:, C:]), 3 * C, lib.ptr(g[:, 2 * C:]), 3 * C, None, 0, None, 0, lib.ptr(out), C + 8,
                 B, L, L, 0, HEADS, d, d ** -0.5, lib.stream_ptr(g.device))
        _check(f'attention L={L} d={d}', fam, dtype, _take(buf, B * L, C, f'attention L={L} d={d} / {fam}'), ref, failures)
    _raise_all(failures)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('L,S,D', H.LINATTN_SHAPES)
def test_linear_attention_families(lib, dtype, L, S, D):
    from mvedit_amd.ops import dt
    C, E, failures = HEADS * D, D * D + D, []
    rel = lambda a, r: float((a.double().cpu() - r).norm() / r.norm())
    for fam in H.LINATTN_FAMILIES:
        ql, ks, ref, KV, Ksum = H.attn_case('linear', (L, S, D), fam, dtype)
        gl, gs = ql.cuda(), ks.cuda()
        kv = torch.empty(B * HEADS, E, dtype=torch.float32, device='cuda')
        nbytes = lib.raw('mve_linattn_workspace_bytes')(B, S, HEADS, D)
        assert (nbytes > 0) == (S > 128)
        ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda') if nbytes else None
        buf, out = _out(B * L, C, dtype)
        lib.call('mve_linattn_kv', dt(dtype), lib.ptr(gs[:, C:]), 3 * C, lib.ptr(gs[:, 2 * C:]), 3 * C, B, S, HEADS, D, lib.ptr(kv), lib.ptr(ws), nbytes,
                 lib.stream_ptr(gs.device))
        lib.call('mve_linattn_apply', dt(dtype), lib.ptr(gl), 3 * C, lib.ptr(kv), lib.ptr(out), C + 8, B, L, HEADS, D, 1e-6, lib.stream_ptr(gs.device))
        path = f'linear ({L},{S},{D})'
        got = _take(buf, B * L, C, f'{path} / {fam}')
        e_kv, e_ks = rel(kv, torch.cat([KV, Ksum], 1)), rel(kv[:, D * D:], Ksum)
        if not (e_kv <= 1e-5 and e_ks <= 1e-5):
            failures.append(f'{path} / {fam} / {dtype}: KV | Ksum rel-L2 {e_kv:.3e}, Ksum alone {e_ks:.3e}, bar 1e-5')
        _check(path, fam, dtype, got, ref, failures, WORST_LINEAR)
    _raise_all(failures)
