"""MXFP8 block-scaled linear on the GPU (csrc/mxfp8.hip): the quantiser byte for byte against mxfp8.quantize_host, the scaled-MFMA GEMM bit for
bit on exact data (the test that pins the operand and scale lane maps) and inside the fp32 summation bound on random data, MXFP8Linear."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U24 = 2.0 ** -24                      # unit roundoff of fp32


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. quantiser
# ----------------------------------------------------------------------------------------------------------------------------------
def _quantize_into_ff(lib, x):
    """mve_mxfp8_quantize into buffers prefilled with 0xFF (unwritten padding shows), on torch's current stream."""
    from mvedit_amd import mxfp8, ops
    R, K = x.shape
    Kp = mxfp8.packed_k(K)
    q = torch.full((R, Kp), 0xFF, dtype=torch.uint8, device=x.device)
    e = torch.full((R, Kp // 32), 0xFF, dtype=torch.uint8, device=x.device)
    lib.call('mve_mxfp8_quantize', ops.dt(x), lib.ptr(x), x.stride(0), R, K, lib.ptr(q), lib.ptr(e), lib.stream_ptr(x.device))
    return q, e


def _random_matrix(R, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    hi = 10 if dtype == torch.float16 else 30
    scale = torch.exp2(torch.randint(-hi - 6, hi, (R, K // 32, 1), generator=g).float())
    return (torch.randn(R, K // 32, 32, generator=g) * scale).reshape(R, K).to(dtype)


def _hand_built(R, K, dtype):
    """Random background with constructed blocks laid over the first blocks of the matrix (row-major block order)."""
    x = _random_matrix(R, K, dtype, 99).float().reshape(-1, 32)
    t = 2.0 ** -14                                              # amax 28 -> scale 2^-4: t lands on 2^-10, half the block's subnormal spacing
    special = [
        # amax 28: exact ties 17 -> 16, 19 -> 20, 21 -> 20; +-amax; +0 / -0; the block's subnormal range (ties at 1, 3, 5 half-steps, -t -> -0)
        [28.0, -28.0, 17.0, 19.0, 21.0, -17.0, -19.0, -21.0, 0.0, -0.0, t, -t, 3 * t, -3 * t, 5 * t, 2 * t, 1.5 * t, 0.5 * t, -0.5 * t, 7 * t,
         2.0 ** -11, -2.0 ** -10, 13 * t, 15 * t, 16 * t, 17 * t, 1.0, -1.0, 27.0, 26.0, 25.0, 3.0],
        [1e-30, -1e-30, 0.5e-30, 3e-31, -7e-31, 1e-33, -1e-33, 9.9e-31] + [0.0] * 24 if dtype == torch.float32
        else [2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -20, -2.0 ** -21] + [0.0] * 27,
        [0.0] * 32,
        [448.0, -448.0, 447.0, 449.0 if dtype != torch.bfloat16 else 450.0, 224.0, 240.0, 232.0, 0.001953125] + [0.0015] * 24,
        [-0.0] * 32,
    ]
    for b, vals in enumerate(special[:x.shape[0]]):
        x[b] = torch.tensor(vals, dtype=torch.float32)
    return x.reshape(R, K).to(dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=['f32', 'f16', 'bf16'])
@pytest.mark.parametrize('R,K', [(1, 32), (3, 96), (130, 320), (257, 2816)])
def test_quantizer_is_byte_exact(lib, R, K, dtype):
    from mvedit_amd import mxfp8
    cases = {'random': _random_matrix(R, K, dtype, 1000 + R), 'hand-built': _hand_built(R, K, dtype)}
    for name, x in cases.items():
        want_q, want_e = mxfp8.quantize_host(x)
        q, e = _quantize_into_ff(lib, x.to(DEV))
        assert torch.equal(e.cpu(), want_e), f'{name}: scale bytes differ'
        assert torch.equal(q.cpu(), want_q), f'{name}: element bytes differ'
        if name == 'hand-built':
            d = mxfp8.dequantize_host(want_q, want_e, K)[0]
            assert d[2:8].tolist() == [16.0, 20.0, 20.0, -16.0, -20.0, -20.0]          # the ties went to even
    # row-strided views: 16-byte aligned rows (the vector loads) and rows that are not (the element loads)
    for off, extra in ((8, 40), (3, 41)):
        wide = torch.zeros(R, K + extra, dtype=dtype)
        wide[:, off:off + K] = _random_matrix(R, K, dtype, 2000 + R + off)
        xv = wide.to(DEV)[:, off:off + K]
        assert xv.stride(0) == K + extra and (R == 1 or not xv.is_contiguous())
        want_q, want_e = mxfp8.quantize_host(wide[:, off:off + K])
        q, e = _quantize_into_ff(lib, xv)
        assert torch.equal(e.cpu(), want_e) and torch.equal(q.cpu(), want_q), f'row-strided view at {off}, ldx = K + {extra}'
        q2, e2 = mxfp8.quantize(xv)                             # the public wrapper, same bytes
        assert torch.equal(q2, q) and torch.equal(e2, e)
    # once more on a non-default stream
    x = cases['hand-built'].to(DEV)
    want_q, want_e = mxfp8.quantize_host(cases['hand-built'])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        q, e = _quantize_into_ff(lib, x)
    side.synchronize()
    assert torch.equal(e.cpu(), want_e) and torch.equal(q.cpu(), want_q), 'non-default stream'


def test_quantizer_rounds_like_the_host_at_every_e4m3_boundary(lib):
    """Every finite e4m3 value, every midpoint between two neighbours and the f32 values one step either side of it, both signs, in blocks
    whose first element is 448 (scale 1, so the values reach the converter as they are); and f32 subnormals / tiny values of either sign."""
    from mvedit_amd import mxfp8
    vals = torch.arange(0, 0x7f, dtype=torch.uint8).view(torch.float8_e4m3fn).float()          # 0 .. 448 ascending
    mid = (vals[1:] + vals[:-1]) / 2                                                            # exact in f32
    inf = torch.tensor(float('inf'))
    pos = torch.cat([vals, mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf),
                     torch.tensor([1e-40, 1e-45, 1e-38, 2.0 ** -10 - 2.0 ** -34, 2.0 ** -10 + 2.0 ** -33, 2.0 ** -126, 1e-20])])
    allv = torch.cat([pos, -pos])
    n = (allv.numel() + 30) // 31
    body = torch.zeros(n * 31)
    body[:allv.numel()] = allv
    x = torch.cat([torch.full((n, 1), 448.0), body.reshape(n, 31)], dim=1).reshape(1, -1)
    want_q, want_e = mxfp8.quantize_host(x)
    assert (want_e[0, :n] == 127).all()
    q, e = _quantize_into_ff(lib, x.to(DEV))
    bad = (q.cpu() != want_q).nonzero()
    assert torch.equal(e.cpu(), want_e)
    assert bad.numel() == 0, [(float(x[0, k]), int(q[0, k]), int(want_q[0, k])) for _, k in bad[:8].tolist()]


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. GEMM on exact data
# ----------------------------------------------------------------------------------------------------------------------------------
def _exact_operands(M, N, K):
    """Operands built directly in the packed format: integers in [-8, 8] that depend on both indices, differently for A and W (asymmetric: a
    transposed C write or a swapped operand changes the product), scale bytes in [124, 130] that differ from row to row and, by 0..2, from block
    to block.  With at most 2 binades between the blocks of a row, every partial sum of an output element -- in any order -- is an integer
    multiple of the element's smallest product scale below K * 64 * 2^4 <= 2^24 of it: exact in fp32 (checked by the caller)."""
    Kp = 128 * ((K + 127) // 128)
    m = torch.arange(M).reshape(M, 1)
    n = torch.arange(N).reshape(N, 1)
    k = torch.arange(K).reshape(1, K)
    kb = torch.arange(K // 32).reshape(1, K // 32)
    a = (3 * m + 5 * k + (m * k) % 7) % 17 - 8
    w = (7 * n + 2 * k + (n * k) % 5 + n // 3 + k // 32) % 17 - 8
    aq = torch.zeros(M, Kp, dtype=torch.uint8)
    wq = torch.zeros(N, Kp, dtype=torch.uint8)
    aq[:, :K] = a.float().to(torch.float8_e4m3fn).view(torch.uint8)
    wq[:, :K] = w.float().to(torch.float8_e4m3fn).view(torch.uint8)
    ae = torch.full((M, Kp // 32), 127, dtype=torch.uint8)
    we = torch.full((N, Kp // 32), 127, dtype=torch.uint8)
    ae[:, :K // 32] = (124 + m % 5 + (m + kb) % 3).to(torch.uint8)
    we[:, :K // 32] = (124 + (3 * n + 1) % 5 + (2 * n + kb + kb // 4) % 3).to(torch.uint8)
    return aq, ae, wq, we


@pytest.mark.parametrize('pad', [8, 9], ids=['ldc=N+8', 'ldc=N+9'])
@pytest.mark.parametrize('M,N,K', [(16, 16, 128), (1, 8, 32), (17, 40, 96), (130, 320, 320), (257, 136, 2816)])
def test_gemm_exact(lib, M, N, K, pad):
    from mvedit_amd import mxfp8
    aq, ae, wq, we = _exact_operands(M, N, K)
    assert ae.min() >= 124 and ae.max() <= 130 and we.min() >= 124 and we.max() <= 130
    A = mxfp8.dequantize_host(aq, ae, K)
    W = mxfp8.dequantize_host(wq, we, K)
    want = A @ W.T                                               # float64: exact
    # the precondition of bit-exactness: sum |a w| is below 2^24 units of the element's smallest product scale
    unit = torch.exp2(ae[:, :K // 32].double().amin(1) - 127).reshape(M, 1) * torch.exp2(we[:, :K // 32].double().amin(1) - 127).reshape(1, N)
    assert ((A.abs() @ W.abs().T) / unit < 2.0 ** 24).all()
    assert (want.float().double() == want).all()
    SENT = -12345.0
    buf = torch.full((M + 2, N + pad), SENT, dtype=torch.float32, device=DEV)
    out = buf[1:M + 1, :N]
    got = mxfp8.gemm(aq.to(DEV), ae.to(DEV), wq.to(DEV), we.to(DEV), K, out_dtype=torch.float32, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu()
    bad = (host[1:M + 1, :N].double() != want).nonzero()
    assert bad.numel() == 0, (f'{bad.shape[0]} of {M * N} elements differ; first: '
                              + str([(i, j, float(host[1 + i, j]), float(want[i, j])) for i, j in bad[:6].tolist()]))
    assert (host[0] == SENT).all() and (host[M + 1] == SENT).all() and (host[:, N:] == SENT).all(), 'guard rows / columns were written'


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. GEMM on random data
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case(M, N, K):
    """quantize(N(0, 1)) operands and, once per shape, the float64 reference of the DEQUANTISED operands (the GEMM's exact answer)."""
    from mvedit_amd import mxfp8
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    aq, ae = mxfp8.quantize(a.to(DEV))
    wq, we = mxfp8.quantize(w.to(DEV))
    A = mxfp8.dequantize_host(aq.cpu(), ae.cpu(), K)
    W = mxfp8.dequantize_host(wq.cpu(), we.cpu(), K)
    y = A @ W.T
    absy = A.abs() @ W.abs().T
    return dict(aq=aq, ae=ae, wq=wq, we=we, y=y, absy=absy, bias=bias, res=res)


_HALF_ULP = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
_TINY = {torch.float32: 0.0, torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}            # half the fp16 subnormal spacing


@pytest.mark.parametrize('M,N,K', [(130, 320, 640), (64, 1280, 5120)])
def test_gemm_random_is_inside_the_fp32_summation_bound(lib, M, N, K):
    from mvedit_amd import mxfp8
    c = _random_case(M, N, K)
    acc_bound = (K + 2) * U24 * c['absy']                       # any-order fp32 summation of exact products
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        out = mxfp8.gemm(c['aq'], c['ae'], c['wq'], c['we'], K, out_dtype=dtype)
        again = mxfp8.gemm(c['aq'], c['ae'], c['wq'], c['we'], K, out_dtype=dtype)
        assert out.dtype == dtype and torch.equal(out, again), 'two runs differ'
        tol = acc_bound + (c['y'].abs() + acc_bound) * _HALF_ULP[dtype] + _TINY[dtype]
        err = (out.cpu().double() - c['y']).abs()
        print(f'mxfp8 gemm {M}x{N}x{K} {dtype}: max err / bound = {float((err / tol).max()):.3f}')
        assert (err <= tol).all(), float((err / tol).max())
        # bias + residual: (acc + bias) + residual, two more fp32 roundings, then the one rounding to the output type
        bias = c['bias'].to(DEV)
        res = c['res'].to(dtype).to(DEV)
        out = mxfp8.gemm(c['aq'], c['ae'], c['wq'], c['we'], K, bias=bias, residual=res, out_dtype=dtype)
        again = mxfp8.gemm(c['aq'], c['ae'], c['wq'], c['we'], K, bias=bias, residual=res, out_dtype=dtype)
        assert torch.equal(out, again), 'two runs differ (bias + residual)'
        b64, r64 = c['bias'].double().reshape(1, N), res.cpu().double()
        want = c['y'] + b64 + r64
        t1 = c['y'].abs() + b64.abs() + acc_bound               # >= |fl(acc + bias)| up to second order
        tol32 = (acc_bound + U24 * t1 + U24 * (t1 + r64.abs())) * (1 + 2.0 ** -20)
        tol = tol32 + (want.abs() + tol32) * _HALF_ULP[dtype] + _TINY[dtype]
        err = (out.cpu().double() - want).abs()
        assert (err <= tol).all(), float((err / tol).max())
        only_bias = mxfp8.gemm(c['aq'], c['ae'], c['wq'], c['we'], K, bias=bias, out_dtype=dtype)
        tol32 = (acc_bound + U24 * t1) * (1 + 2.0 ** -20)
        tol = tol32 + ((c['y'] + b64).abs() + tol32) * _HALF_ULP[dtype] + _TINY[dtype]
        assert ((only_bias.cpu().double() - (c['y'] + b64)).abs() <= tol).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. MXFP8Linear
# ----------------------------------------------------------------------------------------------------------------------------------
def _round_trip_bound(x):
    """Elementwise bound of the quantiser's round trip (tests/test_mxfp8_host.py::test_round_trip_bound), float64, from the input alone."""
    from mvedit_amd import mxfp8
    X = torch.exp2(mxfp8.block_exponents(x).double()).repeat_interleave(32, dim=1)
    return torch.maximum(2.0 ** -4 * x.double().abs(), 2.0 ** -10 * X)


def test_mxfp8_linear(lib):
    from mvedit_amd import mxfp8
    g = torch.Generator().manual_seed(7)
    K, N = 640, 320
    x = torch.randn(2, 65, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    b = torch.randn(N, generator=g)
    lin = mxfp8.MXFP8Linear(w.to(DEV), b.to(DEV))
    y = lin(x.to(DEV))
    assert y.shape == (2, 65, N) and y.dtype == torch.float16
    x2 = x.reshape(-1, K)
    aq, ae = mxfp8.quantize(x2.to(DEV))
    direct = mxfp8.gemm(aq, ae, lin.wq, lin.we, K, bias=b.to(DEV), out_dtype=torch.float16)
    assert torch.equal(y.reshape(-1, N), direct)
    wq, we = mxfp8.quantize_host(w)
    assert torch.equal(lin.wq.cpu(), wq) and torch.equal(lin.we.cpu(), we)
    a64, w64, b64 = x2.double(), w.double(), b.double().reshape(1, N)
    want = a64 @ w64.T + b64
    ea, ew = _round_trip_bound(x2), _round_trip_bound(w)
    quant = ea @ w64.abs().T + a64.abs() @ ew.T + ea @ ew.T      # sum_k (ea |w| + ew |a| + ea ew)
    absy = (a64.abs() + ea) @ (w64.abs() + ew).T                 # >= |A_q| |W_q|^T
    acc_bound = (K + 2) * U24 * absy
    t32 = (acc_bound + U24 * (want.abs() + quant + acc_bound)) * (1 + 2.0 ** -20)
    tol = quant + t32 + (want.abs() + quant + t32) * 2.0 ** -11 + 2.0 ** -25
    err = (y.reshape(-1, N).cpu().double() - want).abs()
    rel = float((y.reshape(-1, N).cpu().double() - want).norm() / want.norm())
    print(f'MXFP8Linear [130, 640] x [320, 640]: rel-L2 against float64 = {rel:.4e}, max err / bound = {float((err / tol).max()):.3f}')
    assert (err <= tol).all(), float((err / tol).max())
    with pytest.raises(AssertionError):
        lin(x)                                                   # a CPU tensor raises
    with pytest.raises(AssertionError):
        mxfp8.MXFP8Linear(w)
