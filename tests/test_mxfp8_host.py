"""MXFP8 packed format on the host (no GPU): the properties of mxfp8.quantize_host -- the written specification of the format of
include/mvedit_amd.h section 2b -- the derived round-trip bound, and the argument validation of the C entry points."""
import ctypes

import pytest
import torch


def _constructed_blocks():
    """Blocks of 32 whose amax sits on the edges of the scale rule: exactly 448 * 2^j, one f32 step above it, and m on either side of 0.875."""
    g = torch.Generator().manual_seed(11)
    rows = []
    for j in (-140, -126, -40, -9, -1, 0, 1, 7, 40, 110):
        top = torch.tensor(448.0, dtype=torch.float64) * 2.0 ** j
        top = top.float()
        if not torch.isfinite(top) or top == 0:
            continue
        for amax in (top, torch.nextafter(top, torch.tensor(float('inf'))), torch.nextafter(top, torch.tensor(0.0))):
            blk = (torch.rand(32, generator=g) * 2 - 1) * amax
            blk[int(torch.randint(0, 32, (1,), generator=g))] = amax if j % 2 else -amax
            rows.append(blk)
    for m in (0.875, 0.875 + 2.0 ** -24, 0.875 - 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24):
        for ex in (-20, 0, 3, 30):
            amax = torch.tensor(m * 2.0 ** ex, dtype=torch.float32)
            blk = (torch.rand(32, generator=g) * 2 - 1) * amax
            blk[5] = amax
            rows.append(blk)
    return torch.stack(rows)                                   # [n, 32]


def _random_blocks(n=512):
    g = torch.Generator().manual_seed(5)
    scale = torch.exp2(torch.randint(-30, 30, (n, 1), generator=g).float())
    return torch.randn(n, 32, generator=g) * scale


@pytest.fixture(scope='module')
def blocks(lib):
    from mvedit_amd import mxfp8
    x = torch.cat([_constructed_blocks(), _random_blocks(), torch.zeros(1, 32)])
    x = x.reshape(1, -1)                                        # one row of many blocks
    q, e = mxfp8.quantize_host(x)
    return mxfp8, x, q, e


def test_scale_rule_no_element_clips_and_the_scale_is_minimal(blocks):
    mxfp8, x, q, e = blocks
    K = x.shape[1]
    s = e[:, :K // 32].to(torch.float64) - 127.0
    assert torch.equal(s.to(torch.int32), mxfp8.block_exponents(x))
    xb = x.double().reshape(1, K // 32, 32)
    amax = xb.abs().amax(-1)
    scaled = xb * torch.exp2(-s).unsqueeze(-1)                   # exact in float64
    assert (scaled.abs() <= 448.0).all(), 'an element would clip'
    live = (amax > 0) & (s > -127) & (s < 127)
    assert live.sum() >= 500
    assert (amax[live] * torch.exp2(-(s[live] - 1)) > 448.0).all(), 'a smaller scale would have done'
    # the closed form of the header: amax = m 2^ex -> ex - 9 if m <= 0.875 else ex - 8
    m, ex = torch.frexp(amax[live])
    assert torch.equal(s[live], torch.where(m <= 0.875, ex - 9, ex - 8).double())
    # clamped blocks (amax below 2^-118): s = -127 and still nothing clips
    assert (s[(amax > 0) & ~live] == -127).all() and ((amax > 0) & ~live).any()


def test_zero_block_and_constructed_amax(blocks):
    mxfp8, x, q, e = blocks
    K = x.shape[1]
    assert e[0, K // 32 - 1] == 127 and (q[0, K - 32:K] == 0).all()              # the all-zero block
    for amax, want_s in ((448.0, 0), (448.0 * 4, 2), (449.0, 1), (28.0, -4), (0.875, -9), (0.8750001, -8), (1.0, -8)):
        blk = torch.zeros(1, 32)
        blk[0, 3] = -amax
        qq, ee = mxfp8.quantize_host(blk)
        assert int(ee[0, 0]) - 127 == want_s, (amax, int(ee[0, 0]) - 127)
    qq, ee = mxfp8.quantize_host(torch.tensor([[448.0, -448.0, 28.0 * 16, 17.0 * 16, 19.0 * 16, 21.0 * 16, -0.0] + [0.0] * 25]))
    assert qq[0, :7].tolist() == [0x7e, 0xfe, 0x7e, 0x78, 0x7a, 0x7a, 0x80]      # max finite, ties to even (272 -> 256, 304 -> 320, 336 -> 320), -0


@pytest.mark.parametrize('K', [32, 96, 160])
def test_padding(lib, K):
    from mvedit_amd import mxfp8
    g = torch.Generator().manual_seed(K)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        x = torch.randn(3, K, generator=g).to(dtype)
        q, e = mxfp8.quantize_host(x)
        Kp = 128 * ((K + 127) // 128)
        assert Kp == mxfp8.packed_k(K) and q.shape == (3, Kp) and e.shape == (3, Kp // 32) and q.dtype == e.dtype == torch.uint8
        assert (q[:, K:] == 0x00).all() and (e[:, K // 32:] == 127).all()
        assert (q[:, :K] != 0).any()
        d = mxfp8.dequantize_host(q, e, K)
        assert d.shape == (3, K) and d.dtype == torch.float64


def test_round_trip_bound(blocks):
    """|dequant - x| <= max(2^-4 |x|, 2^-10 X), X = 2^s: half an ulp of a 3-bit mantissa / half the e4m3 subnormal spacing 2^-9 (derived, not measured)."""
    mxfp8, x, q, e = blocks
    K = x.shape[1]
    s = e[:, :K // 32].to(torch.float64) - 127.0
    X = torch.exp2(s).repeat_interleave(32, dim=1)
    away = ((s > -127) & (s < 127)).repeat_interleave(32, dim=1)
    d = mxfp8.dequantize_host(q, e, K)
    err = (d - x.double()).abs()
    bound = torch.maximum(2.0 ** -4 * x.double().abs(), 2.0 ** -10 * X)
    assert (err[away] <= bound[away]).all(), float((err[away] / bound[away]).max())
    assert float((err[away] / bound[away]).max()) > 0.9          # the bound is met somewhere: it is the right one, not a loose one


def test_argument_validation_through_the_c_abi(lib):
    pk = lib.raw('mve_mxfp8_packed_k')
    assert pk(96) == 128 and pk(128) == 128 and pk(40) == -1
    gemm = lib.raw('mve_mxfp8_gemm')
    p = ctypes.c_void_p(256)                                     # never dereferenced: the checks come before the device is touched
    assert gemm(p, p, p, p, 16, 16, 40, 0, p, 16, None, None, 0, None) == -1
    assert lib.last_error().startswith('mve_mxfp8_gemm: K=40')
    assert gemm(p, p, p, p, 16, 12, 64, 0, p, 16, None, None, 0, None) == -1
    assert lib.last_error().startswith('mve_mxfp8_gemm: N=12')
    assert gemm(p, p, p, p, 0, 16, 64, 0, p, 16, None, None, 0, None) == -1
    assert lib.last_error().startswith('mve_mxfp8_gemm: M=0')
    assert lib.raw('mve_mxfp8_quantize')(0, p, 40, 4, 40, p, p, None) == -1
    assert lib.last_error().startswith('mve_mxfp8_quantize: K=40')
    from mvedit_amd import mxfp8
    with pytest.raises(ValueError):
        mxfp8.packed_k(40)
    with pytest.raises(AssertionError):
        mxfp8.quantize(torch.zeros(2, 32))                       # a CPU tensor raises
