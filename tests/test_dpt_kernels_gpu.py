"""The DPT-hybrid row kernels (csrc/dpt.hip) and GroupNorm's ReLU selector through ctypes.

mve_dpt_stem_rows, mve_dpt_maxpool and mve_dpt_gather_s2 move or select data: bit-exact against `F.unfold` / `F.max_pool2d` / slicing of the padded
input.  mve_dpt_upsample2x evaluates torch's align_corners=True formula in fp32 and rounds once: against `F.interpolate` on the fp32 input, rounded
once, the two fp32 evaluations may differ in their last bits (operation order, fused multiply-add, cancellation between the four terms), which moves
a 16-bit result only when the fp32 value sits that close to a rounding boundary -- at most one 16-bit step plus 2^-21 of the largest input, on at
most 2e-2 of the values (measured: 2e-3 in fp16), equality elsewhere.
GroupNorm + ReLU (selector 2) and GroupNorm without activation: fp16 <= 1e-3 rel-L2 against float64 `F.group_norm` on the same 16-bit inputs (the
per-kernel bar); bf16 is printed without a bar.  Shapes: case A's stem map and its narrowest bottleneck (2 channels per group, both GroupNorm
paths: one launch at 24 x 24, three launches at 48 x 48), and one width of 32 channels per group."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {torch.float16: 1, torch.bfloat16: 2}
DTYPES = [torch.float16, torch.bfloat16]


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,S', [(2, 96), (1, 34)])
def test_stem_rows_are_unfold_of_the_same_padded_image(lib, B, S, dtype):
    Ho = S // 2
    px = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(S)).to(dtype)
    want = torch.zeros(B * Ho * Ho, 152, dtype=dtype)
    padded = F.pad(px.float(), (2, 3, 2, 3))                       # TF "same" for 7 x 7 / 2 over an even size: 2 before, 3 after
    want[:, :147] = F.unfold(padded, kernel_size=7, stride=2).transpose(1, 2).reshape(B * Ho * Ho, 147).to(dtype)
    rows, dpx = torch.full((B * Ho * Ho, 152), float('nan'), dtype=dtype, device='cuda'), px.cuda()
    lib.call('mve_dpt_stem_rows', DT[dtype], lib.ptr(dpx), B, S, lib.ptr(rows), 152, lib.stream_ptr(rows.device))
    torch.cuda.synchronize()
    assert torch.equal(rows.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,H,C', [(2, 48, 32), (1, 6, 264)])
def test_maxpool_is_max_pool2d_of_the_same_padded_map(lib, B, H, C, dtype):
    x = torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(H)).relu().to(dtype)          # behind a ReLU, as in the network
    want0 = F.max_pool2d(F.pad(x.float(), (0, 1, 0, 1), value=0.0), 3, 2)                             # transformers: zero padding
    wanti = F.max_pool2d(F.pad(x.float(), (0, 1, 0, 1), value=float('-inf')), 3, 2)                   # timm: -inf padding
    assert torch.equal(want0, wanti)
    dx = _nhwc(x).cuda()
    y = torch.full((B, H // 2, H // 2, C), float('nan'), dtype=dtype, device='cuda')
    lib.call('mve_dpt_maxpool', DT[dtype], lib.ptr(dx), B, H, H, C, lib.ptr(y), lib.stream_ptr(y.device))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().permute(0, 3, 1, 2).float(), want0)
    # a signed input: the taps outside the map are left out (the -inf form)
    xs = torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(H + 1)).to(dtype)
    lib.call('mve_dpt_maxpool', DT[dtype], lib.ptr(_nhwc(xs).cuda()), B, H, H, C, lib.ptr(y), lib.stream_ptr(y.device))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().permute(0, 3, 1, 2).float(), F.max_pool2d(F.pad(xs.float(), (0, 1, 0, 1), value=float('-inf')), 3, 2))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,H,C', [(2, 24, 64), (1, 6, 136)])
def test_gather_s2_is_a_strided_slice(lib, B, H, C, dtype):
    x = torch.randn(B, H, H, C, generator=torch.Generator().manual_seed(C)).to(dtype).cuda()
    y = torch.full((B, H // 2, H // 2, C), float('nan'), dtype=dtype, device='cuda')
    lib.call('mve_dpt_gather_s2', DT[dtype], lib.ptr(x), B, H, H, C, lib.ptr(y), lib.stream_ptr(y.device))
    torch.cuda.synchronize()
    assert torch.equal(y, x[:, ::2, ::2, :])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,H,W,C', [(2, 6, 6, 64), (1, 24, 24, 32), (1, 5, 3, 8), (1, 1, 1, 16)])
def test_upsample2x_is_interpolate_align_corners_rounded_once(lib, B, H, W, C, dtype):
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H * W)).to(dtype).cuda()
    want = F.interpolate(x.float(), scale_factor=2, mode='bilinear', align_corners=True).to(dtype)
    dx = _nhwc(x)
    y = torch.full((B, 2 * H, 2 * W, C), float('nan'), dtype=dtype, device='cuda')
    lib.call('mve_dpt_upsample2x', DT[dtype], lib.ptr(dx), B, H, W, C, lib.ptr(y), lib.stream_ptr(y.device))
    torch.cuda.synchronize()
    got = y.permute(0, 3, 1, 2)
    # two fp32 evaluations of the four-term formula differ by at most 2^-21 of the largest operand (a few fp32 roundings of partial sums that may
    # cancel), and the single rounding to 16 bits can then land on the neighbouring value: |got - want| <= 2^-21 max|x| + one 16-bit step at want
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    step = torch.exp2(torch.floor(torch.log2(want.float().abs().clamp_min(2.0 ** emin))) - mant)
    diff = (got.float() - want.float()).abs()
    frac = float((diff > 0).float().mean())
    print(f'upsample2x {dtype} {B}x{H}x{W}x{C}: {frac:.2e} of the values differ, max |diff| {float(diff.max()):.3e}')
    assert bool((diff <= 2.0 ** -21 * float(x.float().abs().max()) + step).all())
    # a flip needs the fp32 value within ~2^-21 max|x| of a 16-bit boundary: a share of about 2^-10 max|x| / |value| in fp16 (2^-13 in bf16), a few
    # 1e-3 for normal data; 2e-2 leaves room for the cancelling tail and still fails a kernel that rounds twice or interpolates in 16 bits
    assert frac <= 2e-2
    # the corners are copies (align_corners=True)
    assert torch.equal(got[:, :, 0, 0], x[:, :, 0, 0]) and torch.equal(got[:, :, -1, -1], x[:, :, -1, -1])


@pytest.mark.parametrize('dtype', DTYPES)
def test_add_relu_is_one_rounded_sum(lib, dtype):
    n = 3 * 1000 * 8
    g = torch.Generator().manual_seed(9)
    a, b = (torch.randn(n, generator=g).to(dtype).cuda() for _ in range(2))
    y = torch.full((n,), float('nan'), dtype=dtype, device='cuda')
    lib.call('mve_dpt_add_relu', DT[dtype], lib.ptr(a), lib.ptr(b), lib.ptr(y), n, lib.stream_ptr(y.device))
    torch.cuda.synchronize()
    assert torch.equal(y, (a.float() + b.float()).relu().to(dtype))
    a0 = a.clone()
    lib.call('mve_dpt_add_relu', DT[dtype], lib.ptr(a), None, lib.ptr(a), n, lib.stream_ptr(y.device))      # in place, no second operand
    torch.cuda.synchronize()
    assert torch.equal(a, a0.relu()) and float((a == 0).float().mean()) > 0.3


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', [2, 0])
@pytest.mark.parametrize('B,HW,C,G', [(2, 48 * 48, 32, 8), (2, 24 * 24, 16, 8), (2, 48 * 48, 16, 8), (1, 12 * 12, 256, 8)])
def test_groupnorm_relu_and_plain(lib, B, HW, C, G, act, dtype):
    """act 2 = ReLU (the new selector), 0 = none.  fp16 <= 1e-3; bf16 printed.  Measured on an MI355X over the four shapes and both selectors:
    fp16 2.06e-4 .. 2.09e-4, bf16 1.655e-3 .. 1.676e-3."""
    g = torch.Generator().manual_seed(HW + C)
    x = (torch.randn(B, HW, C, generator=g) * 1.5 + 0.3).to(dtype)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = F.group_norm(x.double().transpose(1, 2), G, gamma.double(), beta.double(), 1e-5)
    ref = (ref.relu() if act == 2 else ref).transpose(1, 2)
    dx, dg, db = x.cuda(), gamma.cuda(), beta.cuda()
    y = torch.full((B, HW, C), float('nan'), dtype=dtype, device='cuda')
    ws = torch.empty(lib.raw('mve_groupnorm_workspace_bytes')(B, HW, C, G), dtype=torch.uint8, device='cuda')
    lib.call('mve_groupnorm_silu', DT[dtype], lib.ptr(dx), C, None, 0, B, HW, G, 1e-5, lib.ptr(dg), lib.ptr(db), act, lib.ptr(y), lib.ptr(ws), lib.stream_ptr(y.device))
    torch.cuda.synchronize()
    err = float((y.double().cpu() - ref).norm() / ref.norm())
    print(f'groupnorm act {act} {dtype} B {B} HW {HW} C {C} G {G}: rel-L2 {err:.3e}')
    if act == 2:
        assert bool((y >= 0).all())
    assert err == err
    if dtype == torch.float16:
        assert err <= 1e-3
