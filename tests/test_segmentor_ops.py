"""Every exported operator of csrc/tracer.hip (the TRACER-B7 segmentor's own kernels) on its own against a float64 reference in plain torch, at
small shapes chosen for the paths the kernels take: image borders, odd sizes, partial strips / slabs / blocks, channel slices, every mode flag.
test_segmentor.py checks the whole network behind sigmoids and gates; a wrong tap, offset or index survives there and must not survive here.

The references get the SAME STORED OPERANDS: 16-bit tensors are rounded first and then widened to float64.

Tolerances (the helpers _check16 / _check32 below):
  16-bit outputs   |got - ref| <= u |ref| + a.  u = one rounding step of the type (2^-8 bf16, 2^-11 fp16: half a step for the store and half
                   for the double rounding fp32 -> 16 bit), a = the fp32 accumulation, (terms + 1) 2^-23 sum|x w| from the reference's
                   absolute-value convolution (0 for a bare activation).  fp16 adds a subnormal step 2^-24.  Never relative to the tensor's
                   maximum.  No term for the activations' fast exp: measured on an MI355X the worst err / bar of every 16-bit case is
                   0.89 ... 0.997, all of it the store's half step at the bottom of a binade (u |ref| there).
  fp32 outputs     the same operator evaluated in torch float32 on the CPU is measured against the float64 reference on the same inputs;
                   the kernel is allowed 8 x that error (fast exp, another summation order), and never more than 1e-4 of the output's scale.
                   Both errors are printed, and the figures of an MI355X run are in each test's docstring (maxima over the test's cases).
                   Where torch float32 is exact the bar is 0 and the kernel must be exact too.  That happened in 15 cases of that run, for
                   reasons that hold for any order of fp32 operations: a copied pixel (4 x 4 -> 1 x 1 with aligned corners, the rows of a
                   single-row input), HW = 1 means, nslab = 1 pooled vectors with a power-of-two scale, and three C = 8 slab sums of at most
                   221 bf16 values (8-bit significands).
  bitwise          batch invariance and untouched-sentinel checks use torch.equal.
The CPU tests (unmarked) pin the float64 references to oracle/tracer_oracle.py, which test_oracle_equals_reference_executed_golden pins to the
reference's executed modules, and check the exclusion caps on the references alone."""
import pytest
import torch
import torch.nn.functional as F

from oracle import tracer_oracle as T

BF16, FP16 = torch.bfloat16, torch.float16
DTYPES = pytest.mark.parametrize('dtype', [BF16, FP16], ids=['bf16', 'fp16'])
U = {BF16: 2.0 ** -8, FP16: 2.0 ** -11}
TINY = {BF16: 0.0, FP16: 2.0 ** -24}
EPS32 = 2.0 ** -23
ACT = {0: lambda t: t, 1: F.silu, 2: F.selu, 3: torch.relu, 4: torch.sigmoid}
DEV = 'cuda:0'


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _dt(dtype):
    from mvedit_amd.ops import dt
    return dt(dtype)


def _call(lib, name, *args):
    with torch.cuda.device(DEV):
        lib.call(name, *args, lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()


def _check16(got, ref, dtype, a, what, keep=None):
    got = got.double().cpu().reshape(ref.shape)
    err, bar = (got - ref).abs(), U[dtype] * ref.abs() + a + TINY[dtype]
    if keep is not None:
        err, bar = err[keep], bar[keep]
    print(f'{what} {dtype}: max|got - ref| {float(err.max()):.3e}, worst err / bar {float((err / bar).max()):.3f}')
    assert torch.isfinite(got).all() and bool((err <= bar).all()), (what, float(err.max()), float((err / bar).max()))


def _check32(got, ref, cpu32, what, keep=None):
    got, cpu32 = got.double().cpu().reshape(ref.shape), cpu32.double().reshape(ref.shape)
    assert torch.isfinite(got).all(), what
    eg, ec = (got - ref).abs(), (cpu32 - ref).abs()
    if keep is not None:
        eg, ec = eg[keep], ec[keep]
    e_gpu, e_cpu, scale = float(eg.max()), float(ec.max()), float(ref.abs().max())
    bar = min(8 * e_cpu, 1e-4 * scale)
    print(f'{what}: GPU max|got - f64| {e_gpu:.3e}, CPU-fp32 {e_cpu:.3e}, bar {bar:.3e}, scale {scale:.3e}')
    assert e_gpu <= bar, (what, e_gpu, e_cpu, scale)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 references (shared by the GPU tests and the CPU pinning tests)
# ---------------------------------------------------------------------------------------------------------------------------------------
def conv_ref(x, w, bias, groups, stride, pad_tl, Ho, Wo, dil, dtype64=torch.float64):
    """x [B, H, W, Cin] (any float type), w [Cout, Cin / groups, kh, kw], explicit top-left padding; the bottom / right padding is what the
    output size asks for.  -> (conv + bias, |x| * |w| + |bias|) as [B, Ho, Wo, Cout]"""
    B, H, W, _ = x.shape
    kh, kw = w.shape[2:]
    pb = (Ho - 1) * stride + (kh - 1) * dil + 1 - H - pad_tl[0]
    pr = (Wo - 1) * stride + (kw - 1) * dil + 1 - W - pad_tl[1]
    assert pb >= 0 and pr >= 0 and pb <= pad_tl[0] + stride and pr <= pad_tl[1] + stride
    xp = F.pad(x.to(dtype64).permute(0, 3, 1, 2), (pad_tl[1], pr, pad_tl[0], pb))
    wd, bd = w.to(dtype64), None if bias is None else bias.to(dtype64)
    y = F.conv2d(xp, wd, bd, stride=stride, dilation=dil, groups=groups)
    mag = F.conv2d(xp.abs(), wd.abs(), None if bd is None else bd.abs(), stride=stride, dilation=dil, groups=groups)
    assert y.shape[2:] == (Ho, Wo)
    return y.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def resize_ref(x_nchw, Ho, Wo, align, mean=None, std=None):
    y = F.interpolate(x_nchw, size=(Ho, Wo), mode='bilinear', align_corners=bool(align))
    if mean is not None:
        y = (y - mean.to(y.dtype).view(1, -1, 1, 1)) / std.to(y.dtype).view(1, -1, 1, 1)
    return y


def se_gate_ref(sums, scale, w1, b1, w2, b2):
    t = sums.dtype
    pooled = sums.sum(1) * torch.tensor(scale, dtype=torch.float32).to(t)
    hidden = F.silu(pooled @ w1.to(t).T + b1.to(t))
    return torch.sigmoid(hidden @ w2.to(t).T + b2.to(t)), pooled


def uam_channel_ref(pooled, ns, nb, wq, wk, wv, wfc, ratio, bs, bt):
    """channel tracer + confidence mask (att_modules.py:135-168) -> att, A, S, thr with BatchNorm(x * att + x) * mask = x * A + S"""
    xn = pooled * ns + nb
    q, k, v = xn @ wq.T, xn @ wk.T, xn @ wv.T                                       # [B, C]
    o = F.scaled_dot_product_attention(q[:, None, :, None], k[:, None, :, None], v[:, None, :, None], scale=1.0)[:, 0, :, 0]
    att = torch.sigmoid(o @ wfc.T)
    thr = torch.quantile(att, ratio, dim=-1, keepdim=True, interpolation='linear')
    m = torch.where(att <= thr, torch.zeros_like(att), att)
    return att, (1 + att) * bs * m, bt * m, thr


def uam_spatial_ref(qkv, H, W):
    """qkv [B, H * W, 3] -> softmax(q k^T) v + v over the rows of the H x W maps; also the mean of the row maxima of the softmax"""
    q, k, v = (qkv[..., i].reshape(-1, H, W) for i in range(3))
    p = torch.softmax(q @ k.transpose(1, 2), -1)
    return (p @ v + v).reshape(-1, H * W), float(p.max(-1).values.mean())


def object_mix_ref(d, enc):
    """d [B, HW], enc [B, HW, C] -> enc * (sigmoid(d) + edge), edge = 1 - sigmoid(d) where that is <= 0.93"""
    ob = torch.sigmoid(d)
    bg = 1 - ob
    edge = torch.where(bg > 0.93, torch.zeros_like(bg), bg)
    return enc * (ob + edge)[..., None], bg


def fuse_ref(d0, d1, d2):
    up = lambda t, s: F.interpolate(t[:, None], scale_factor=s, mode='bilinear')[:, 0]
    return torch.sigmoid((up(d2, 4) + up(d1, 8) + up(d0, 8)) / 3)


def post_ref(m, erosion, Ho, Wo, out_dtype):
    """m [B, Hs, Ws] float64 -> (mask after the failure rule, resized map before it, per-image decision); out_dtype None: fp32 output"""
    er = -F.max_pool2d(-m[:, None], 2 * erosion + 1, 1, erosion)
    pre = F.interpolate(er, size=(Ho, Wo), mode='bilinear', align_corners=False)[:, 0]
    if out_dtype is not None:
        pre = pre.to(out_dtype).to(m.dtype)
    assert not bool(((pre > 0.1) & (pre < 0.3)).any()), 'a resized pixel in (0.1, 0.3): the per-image decision would be ambiguous'
    fire = (pre > 0.2).flatten(1).all(1)
    return pre.masked_fill(fire[:, None, None] & (pre < 0.8), 0.0), pre, fire


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs (seeded, built on the host)
# ---------------------------------------------------------------------------------------------------------------------------------------
# (k, stride, H, W, pad_t = pad_l, Ho, Wo): the encoder's four (k, stride) pairs with their static SAME pads, an odd size, and a non-square
# case; Wo % 4 = 3, 0, 0, 2, 2, 1 -- every tail of the four-wide strip
DW_GEOM = [(3, 1, 19, 19, 1, 19, 19), (3, 2, 24, 24, 0, 12, 12), (3, 2, 23, 23, 1, 12, 12), (5, 2, 22, 22, 1, 10, 10), (5, 1, 10, 10, 2, 10, 10),
           (3, 1, 17, 13, 1, 17, 13)]
# C = 8: one channel lane, 256 pixel lanes (more than the 30 strips of the 10 x 10 case); 288: cw 36, pl 7, four idle threads; 536: cw 1, 67
# chunks; 1344: 3 chunks of cw 56
DW_C = [8, 288, 536, 1344]

UAM_CASES = [(224, False), (256, False), (21, False), (8, False), (224, True)]      # (C, two tied att values at the quantile position)


def uam_channel_inputs(C, tie, B=2):
    g = _gen(C, tie, 8)
    r = lambda *s: torch.randn(*s, generator=g)
    p = dict(pooled=r(B, C), ns=1 + 0.1 * r(C), nb=0.1 * r(C), wq=r(C, C) * C ** -0.5, wk=r(C, C) * C ** -0.5, wv=r(C, C) * C ** -0.5,
             wfc=r(C, C) * 3 * C ** -0.5, bs=1 + 0.1 * r(C), bt=0.1 * r(C))
    if tie:
        # the channel at sorted position floor(0.1 (C - 1)) of image 0 lends its fc row to the one above it: two equal att values, in every
        # image, and in image 0 they sit on both sides of the interpolated quantile
        att = uam_channel_ref(*(p[k].double() for k in ('pooled', 'ns', 'nb', 'wq', 'wk', 'wv', 'wfc')), 0.1, p['bs'].double(), p['bt'].double())[0]
        order = att[0].argsort()
        lo = int(0.1 * (C - 1))
        p['wfc'][order[lo + 1]] = p['wfc'][order[lo]]
    return p


def uam_exclusions(att, thr):
    """channels the masks may disagree on: within 1e-6 of the threshold but not the threshold element itself (that one must come out masked)"""
    d = (att - thr).abs()
    return (d < 1e-6) & (d > 0)


SPATIAL_HW = [(24, 24), (7, 300), (300, 5)]


def uam_spatial_inputs(H, W, B=2):
    g = _gen(H, W, 9)
    qkv = torch.randn(B, H * W, 3, generator=g)
    qkv[..., :2] *= 1.3 * W ** -0.25                 # scores q_i . k_j of standard deviation 1.7: the softmax is neither uniform nor one-hot
    return qkv


def object_mix_inputs(dtype, B=2, HW=35, C=48):
    g = _gen(HW, C, 10)
    d = 3 * torch.randn(B, HW, generator=g)
    d[:, 3], d[:, 17] = -4.0, -2.0                    # background 0.982 (> 0.93: edge term dropped) and 0.881 (kept)
    return d, torch.randn(B, HW, C, generator=g).to(dtype)


def fuse_inputs(Hs, Ws, B=2):
    g = _gen(Hs, Ws, 12)
    return (0.5 * torch.randn(B, Hs // 8, Ws // 8, generator=g) + 1.0, 2.0 * torch.randn(B, Hs // 8, Ws // 8, generator=g) - 1.0,
            4.0 * torch.randn(B, Hs // 4, Ws // 4, generator=g))


POST_SIZES = [(16, 16, 20, 28), (24, 16, 10, 12)]
POST_LOW = 0.02


def post_inputs(Hs, Ws):
    """image 0 in [0.32, 1]: the rule fires; image 1 the same map with one corner pixel low: the rule must not fire wherever the resize lets that
    pixel through, and erosion spreads it; image 2 in [0.85, 1]: nothing changes.  The corner's 8 x 8 neighbourhood is in [0.97, 1] and the low
    value is 0.02 rather than 0.05: the bilinear weights of these sizes put 0.93 and 0.7 of the low region into single output pixels, and only
    with these values does every such blend stay outside (0.1, 0.3) for erosion 0, 1 and 2 (0.05 cannot: 0.93 -> <= 0.1 needs neighbours <= 0.76,
    0.7 -> >= 0.3 needs them >= 0.88).  post_ref asserts it."""
    g = _gen(Hs, Ws, 13)
    m = torch.empty(3, Hs, Ws)
    m[0] = 0.32 + 0.68 * torch.rand(Hs, Ws, generator=g)
    m[0, :8, :8] = 0.97 + 0.03 * torch.rand(8, 8, generator=g)
    m[1] = m[0]
    m[1, 0, 0] = POST_LOW
    m[2] = 0.85 + 0.15 * torch.rand(Hs, Ws, generator=g)
    return m


def post_exclusions(pre, out_dtype):
    """pixels within one unit in the last place of the output type of the rule's 0.8 (fp32: 1e-6)"""
    return (pre - 0.8).abs() <= (1e-6 if out_dtype is None else U[out_dtype])


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the references against the oracle, and the exclusion caps on the references alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _fold(w, b, mean, var, eps):
    s = w / torch.sqrt(var + eps)
    return s, b - mean * s


def test_uam_references_equal_oracle_uam():
    """channel_mean -> uam_channel_ref -> x * A + S -> the q / k / v 1 x 1 convolutions -> uam_spatial_ref, chained in float64, against
    oracle.tracer_oracle.uam (UnionAttentionModule.forward) over a synthetic 'agg.UAM.*' parameter dict, to fp32 accuracy."""
    C, B, H, W = 24, 2, 6, 9
    g = _gen(C, H, W)
    sd = {}
    for bn in ('agg.UAM.bn', 'agg.UAM.norm.0'):
        sd[f'{bn}.weight'], sd[f'{bn}.bias'] = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        sd[f'{bn}.running_mean'], sd[f'{bn}.running_var'] = 0.1 * torch.randn(C, generator=g), 1 + 0.3 * torch.rand(C, generator=g)
    for n in ('channel_q', 'channel_k', 'channel_v', 'fc'):
        sd[f'agg.UAM.{n}.weight'] = torch.randn(C, C, 1, 1, generator=g) * C ** -0.5 * (4 if n == 'fc' else 1)
    for n in ('spatial_q', 'spatial_k', 'spatial_v'):
        sd[f'agg.UAM.{n}.weight'] = torch.randn(1, C, 1, 1, generator=g) * C ** -0.5
    x = torch.randn(B, C, H, W, generator=g) + 0.5
    with torch.no_grad():
        want = T.uam(sd, x, lambda t: t)
    d = {k: v.double() for k, v in sd.items()}
    ns, nb = _fold(*(d[f'agg.UAM.norm.0.{p}'] for p in ('weight', 'bias', 'running_mean', 'running_var')), T.BN_EPS_DEC)
    bs, bt = _fold(*(d[f'agg.UAM.bn.{p}'] for p in ('weight', 'bias', 'running_mean', 'running_var')), T.BN_EPS_DEC)
    xs = x.double().permute(0, 2, 3, 1).reshape(B, H * W, C)
    att, A, S, thr = uam_channel_ref(xs.mean(1), ns, nb, *(d[f'agg.UAM.channel_{n}.weight'][:, :, 0, 0] for n in 'qkv'), d['agg.UAM.fc.weight'][:, :, 0, 0],
                                     0.1, bs, bt)
    assert not bool(uam_exclusions(att, thr).any())
    assert int((A == 0).sum()) == B * 3                              # 0.1 * 23 = 2.3: the three smallest of 24 are masked
    xd = xs * A[:, None] + S[:, None]
    wqkv = torch.cat([d[f'agg.UAM.spatial_{n}.weight'][:, :, 0, 0] for n in 'qkv'], 0)
    got, _ = uam_spatial_ref(xd @ wqkv.T, H, W)
    err = float((got.reshape(want.shape) - want.double()).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), err


@pytest.mark.parametrize('C,tie', UAM_CASES)
def test_uam_channel_reference_excludes_nothing(C, tie):
    p = {k: v.double() for k, v in uam_channel_inputs(C, tie).items()}
    att, A, S, thr = uam_channel_ref(p['pooled'], p['ns'], p['nb'], p['wq'], p['wk'], p['wv'], p['wfc'], 0.1, p['bs'], p['bt'])
    assert not bool(uam_exclusions(att, thr).any())
    assert 0.02 < float(att.max() - att.min())                       # the quantile has something to order
    on = att == thr                                                  # threshold elements: C = 21 (0.1 * 20 = 2) and the tied pair
    assert int(on[0].sum()) == (1 if C == 21 else 2 if tie else 0)
    assert bool((A[on] == 0).all())


@pytest.mark.parametrize('H,W', SPATIAL_HW)
def test_uam_spatial_reference_is_neither_uniform_nor_one_hot(H, W):
    _, pmax = uam_spatial_ref(uam_spatial_inputs(H, W).double(), H, W)
    assert 0.05 < pmax < 0.95, pmax


def test_object_mix_reference_equals_module_lines_and_excludes_nothing():
    """oracle.tracer_oracle.object_attention runs the whole stage (seven convolutions behind the mix) and cannot be cut at the mix without
    rewriting it, so the reference is pinned to the tensor ops the module calls there (att_modules.py:277-282, oracle lines 243-248): sigmoid,
    the cloned background with `edge[edge > .93] = 0`, and the two products, in fp32 on NCHW tensors."""
    d, enc = object_mix_inputs(FP16)
    ref, bg = object_mix_ref(d.double(), enc.double())
    assert not bool(((bg - 0.93).abs() < 1e-5).any())
    dm, em = d.float()[:, None, :, None], enc.float().permute(0, 2, 1)[..., None]
    mask_ob = torch.sigmoid(dm)
    edge = (1 - mask_ob).clone()
    edge[edge > .93] = 0
    want = (mask_ob * em + edge * em)[..., 0].permute(0, 2, 1)
    assert float((ref - want.double()).abs().max()) <= 1e-5 * float(want.abs().max())
    assert float(bg[0, 3]) > 0.93 > float(bg[0, 17]) > 0.8


@pytest.mark.parametrize('Hs,Ws', [(16, 24), (8, 8)])
def test_fuse_reference_equals_oracle_decoder(monkeypatch, Hs, Ws):
    """fuse_ref against the last lines of oracle.tracer_oracle.decoder itself (tracer.py:86-97): the stages in front of them (rfb, aggregation,
    the two object attentions) are replaced by the three synthetic maps, so which map gets the x 8 and which the x 4 upsample is the oracle's
    own assignment.  d0 and d1 enter the sum alike (swapping them changes nothing), so what the scales must tell apart is each of them from
    d2 and the x 4 from the x 8 factor: d2 has another size and another spread, and leaving any one map out moves the result by more than
    1e-2."""
    d0, d1, d2 = fuse_inputs(Hs, Ws)
    ref = fuse_ref(d0.double(), d1.double(), d2.double())
    monkeypatch.setattr(T, 'rfb', lambda sd, name, x, q: x)
    monkeypatch.setattr(T, 'aggregation', lambda sd, e4, e3, e2, q: d0[:, None])
    monkeypatch.setattr(T, 'object_attention', lambda sd, name, dm, em, q: {'ObjectAttention2': d1, 'ObjectAttention1': d2}[name][:, None])
    with torch.no_grad():
        want = T.decoder({}, [None] * 4, lambda t: t)[:, 0]
    assert want.shape == ref.shape
    assert float((ref - want.double()).abs().max()) <= 1e-5
    z = [torch.zeros_like(t).double() for t in (d0, d1, d2)]
    for i in range(3):
        maps = [d0.double(), d1.double(), d2.double()]
        maps[i] = z[i]
        assert float((fuse_ref(*maps) - ref).abs().max()) > 1e-2


@pytest.mark.parametrize('erosion', [0, 1, 2])
@pytest.mark.parametrize('Hs,Ws,Ho,Wo', POST_SIZES)
def test_post_reference_equals_oracle_forward_and_cap(monkeypatch, Hs, Ws, Ho, Wo, erosion):
    """post_ref against oracle.tracer_oracle.forward (erosion, resize, failure rule) with the network replaced by the synthetic map; the
    exclusion cap (2 % of the pixels within one unit in the last place of 0.8) for every output type; and the per-image decisions."""
    m = post_inputs(Hs, Ws)
    monkeypatch.setattr(T, 'model', lambda sd, img, q: m[:, None])
    with torch.no_grad():
        want = T.forward({}, torch.zeros(3, 3, Ho, Wo), input_image_size=(Hs, Ws), erosion=erosion, batch_size=8)[:, 0]
    ref, pre, fire = post_ref(m.double(), erosion, Ho, Wo, None)
    keep = ~post_exclusions(pre, None)
    assert float((ref - want.double()).abs()[keep].max()) <= 1e-6
    for od in (None, BF16, FP16):
        ref, pre, fire = post_ref(m.double(), erosion, Ho, Wo, od)
        assert float(post_exclusions(pre, od).float().mean()) <= 0.02
        # image 1: the low corner reaches the output (and stops the rule) except through the 24 x 16 -> 10 x 12 resize without erosion, where
        # no output pixel takes more than a quarter of it
        assert fire.tolist() == [True, (Hs, erosion) == (24, 0), True]
        assert int((ref[0] == 0).sum()) > 0.3 * Ho * Wo and bool((ref[2] == pre[2]).all())
        if not fire[1]:
            assert int((pre[1] < 0.1).sum()) >= ((1 + erosion) ** 2 if Hs == 16 else 1) and bool((ref[1] == pre[1]).all())     # erosion spreads the low value


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize('C', DW_C)
@pytest.mark.parametrize('k,stride,H,W,pad,Ho,Wo', DW_GEOM)
def test_dwconv_pool_strips(lib, dtype, C, k, stride, H, W, pad, Ho, Wo):
    """mve_seg_dwconv_pool (k_seg_dwconv_strip): (a) the output against the float64 depthwise convolution + swish; (b) the slab sums against
    the float64 per-channel sums of the kernel's own rounded output, to fp32-summation accuracy; (c) the slab count of mve_seg_dwconv_slabs is
    the one the kernel writes (NaN-filled buffer: all of [B][nslab][C] written, the guard behind it untouched); (d) the last image alone:
    bit-identical output and sums.
    MI355X: output worst err / bar 0.996 (bf16), 0.994 (fp16).  Slab sums, 48 cases: GPU max|sum - f64| 4.0e-5 = 2.0e-7 of the scale,
    CPU-fp32 2.7e-5 = 1.5e-7 of the scale; worst GPU / bar 0.62 (k3 s1 19x19 C8 fp16: GPU 3.8e-5, CPU 7.6e-6)."""
    B = 2
    g = _gen(k, stride, H, W, C)
    x = torch.randn(B, H, W, C, generator=g).to(dtype)
    w = torch.randn(k, k, C, generator=g) / k
    bias = 0.3 * torch.randn(C, generator=g)
    y, mag = conv_ref(x, w.permute(2, 0, 1)[:, None], bias, C, stride, (pad, pad), Ho, Wo, 1)
    ref = F.silu(y)
    a = (k * k + 1) * EPS32 * mag
    nslab = lib.raw('mve_seg_dwconv_slabs')(B, Ho, Wo, C, k, stride)
    assert nslab >= 1 and nslab == lib.raw('mve_seg_dwconv_slabs')(1, Ho, Wo, C, k, stride)
    wd, bd = w.to(DEV), bias.to(DEV)

    def run(xb, nb):
        out = torch.full((nb, Ho, Wo, C), float('nan'), dtype=dtype, device=DEV)
        sums = torch.full((nb * nslab * C + C,), float('nan'), dtype=torch.float32, device=DEV)
        _call(lib, 'mve_seg_dwconv_pool', _dt(dtype), lib.ptr(xb), nb, H, W, C, C, lib.ptr(wd), lib.ptr(bd), lib.ptr(out), Ho, Wo, C, k, k, stride, pad,
              pad, 1, lib.ptr(sums))
        assert bool(torch.isnan(sums[nb * nslab * C:]).all()), 'the kernel wrote more slabs than mve_seg_dwconv_slabs reports'
        return out.cpu(), sums[:nb * nslab * C].reshape(nb, nslab, C).cpu()

    out, sums = run(x.to(DEV), B)
    _check16(out, ref, dtype, a, f'dwconv k{k} s{stride} {H}x{W} C{C}')
    assert torch.isfinite(sums).all(), 'a slab of mve_seg_dwconv_slabs was not written'
    _check32(sums.double().sum(1), out.double().sum((1, 2)), out.float().sum((1, 2)), f'dwconv slab sums k{k} s{stride} {H}x{W} C{C} {dtype}')
    one, sums1 = run(x[B - 1:].contiguous().to(DEV), 1)
    assert torch.equal(_bits(one[0]), _bits(out[B - 1])) and torch.equal(_bits(sums1[0]), _bits(sums[B - 1]))


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize('k,dil', [(1, 1), (3, 3), (3, 5)])
def test_conv2d_depthwise_generic(lib, dtype, k, dil):
    """mve_seg_conv2d, depthwise = 1, the generic kernel (1 x 1 and dilated 3 x 3 of ObjectAttention) with SELU at 12 x 9, input and output
    channel slices of wider tensors (C = 24 of ldx = 40 and of ldo = 32); the other columns of the output keep their sentinel bitwise.
    MI355X: worst err / bar 0.996 (bf16), 0.989 (fp16), both at 1 x 1."""
    B, H, W, C, ldx, ldo, xo, oo = 2, 12, 9, 24, 40, 32, 8, 8
    pad = dil * (k // 2)
    g = _gen(k, dil, 2)
    xw = torch.randn(B, H, W, ldx, generator=g).to(dtype)
    w = torch.randn(k, k, C, generator=g) / k
    bias = 0.3 * torch.randn(C, generator=g)
    y, mag = conv_ref(xw[..., xo:xo + C], w.permute(2, 0, 1)[:, None], bias, C, 1, (pad, pad), H, W, dil)
    ref = F.selu(y)
    xd, wd, bd = xw.to(DEV), w.to(DEV), bias.to(DEV)
    ow = torch.full((B * H * W, ldo), 123.0, dtype=dtype, device=DEV)
    _call(lib, 'mve_seg_conv2d', _dt(dtype), lib.ptr(xd[..., xo:]), B, H, W, C, ldx, lib.ptr(wd), lib.ptr(bd), lib.ptr(ow[:, oo:]), H, W, C, ldo, k, k, 1,
          pad, pad, dil, 1, 2, None, None, 0, 0)
    ow = ow.cpu()
    _check16(ow[:, oo:oo + C], ref, dtype, (k * k + 1) * EPS32 * mag, f'dw generic k{k} dil{dil}')
    assert torch.equal(_bits(ow[:, :oo]), _bits(torch.full((B * H * W, oo), 123.0, dtype=dtype)))


# (name, Cin, Cout, k, stride, pad_tl, H, W, Ho, Wo, act, bias, out_f32, ldo, out offset, mul, add, ld2, slice offset of mul / add)
DENSE = [
    ('stem', 3, 64, 3, 2, (0, 0), 17, 21, 8, 10, 1, True, 0, 64, 0, False, False, 0, 0),       # scalar channel tail, CO = 8, 160 pixels
    ('wqkv', 224, 3, 1, 1, (0, 0), 5, 7, 5, 7, 0, False, 1, 3, 0, False, False, 0, 0),          # CO = 4, fp32 output, no bias
    ('conv1', 24, 1, 1, 1, (0, 0), 9, 11, 9, 11, 3, True, 1, 1, 0, False, True, 1, 0),          # Cout = 1, ReLU, + fp32 map
    ('slice', 40, 12, 1, 1, (0, 0), 7, 9, 7, 9, 2, True, 0, 48, 12, False, True, 48, 12),       # Cout % 8 = 4 into a slice, + 16-bit slice
    ('mul', 16, 16, 3, 1, (1, 1), 6, 23, 6, 23, 2, True, 0, 16, 0, True, True, 16, 0),          # act(conv) * mul + add, 276 pixels
]


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize('case', DENSE, ids=[c[0] for c in DENSE])
def test_conv2d_dense(lib, dtype, case):
    """mve_seg_conv2d, depthwise = 0: out = act(conv + bias) [* mul] [+ add] against float64 F.conv2d; B Ho Wo is never a multiple of 256;
    a sliced output leaves the other columns' sentinel bitwise.
    MI355X, fp32 outputs: wqkv GPU 1.3e-6, CPU-fp32 1.3e-6 (4.6e-7 of the scale); conv1 GPU 3.3e-7, CPU-fp32 2.6e-7 (7.7e-8 / 6.1e-8 of the
    scale); worst GPU / bar 0.16.  16-bit outputs: worst err / bar 0.984 (stem), 0.971 (slice), 0.953 (mul)."""
    name, Cin, Cout, k, stride, ptl, H, W, Ho, Wo, act, has_bias, out_f32, ldo, oo, has_mul, has_add, ld2, so = case
    B = 2
    assert (B * Ho * Wo) % 256
    g = _gen(Cin, Cout, k, H)
    x = torch.randn(B, H, W, Cin, generator=g).to(dtype)
    w = torch.randn(Cout, k, k, Cin, generator=g) * (k * k * Cin) ** -0.5
    bias = 0.3 * torch.randn(Cout, generator=g) if has_bias else None
    t2 = torch.float32 if out_f32 else dtype
    mul = (1 + 0.5 * torch.randn(B * Ho * Wo, ld2, generator=g)).to(t2) if has_mul else None
    add = torch.randn(B * Ho * Wo, ld2, generator=g).to(t2) if has_add else None

    def ref_in(t64):
        y, mag = conv_ref(x, w.permute(0, 3, 1, 2), bias, 1, stride, ptl, Ho, Wo, 1, t64)
        r = ACT[act](y).reshape(B * Ho * Wo, Cout)
        mag = mag.reshape(B * Ho * Wo, Cout)
        if has_mul:
            r, mag = r * mul[:, so:so + Cout].to(t64), mag * mul[:, so:so + Cout].to(t64).abs()
        if has_add:
            r = r + add[:, so:so + Cout].to(t64)
        return r, mag

    ref, mag = ref_in(torch.float64)
    xd, wd, bd = x.to(DEV), w.to(DEV), None if bias is None else bias.to(DEV)
    md, ad = None if mul is None else mul.to(DEV), None if add is None else add.to(DEV)
    ow = torch.full((B * Ho * Wo, ldo), 123.0, dtype=t2, device=DEV)
    _call(lib, 'mve_seg_conv2d', _dt(dtype), lib.ptr(xd), B, H, W, Cin, Cin, lib.ptr(wd), lib.ptr(bd), lib.ptr(ow[:, oo:]), Ho, Wo, Cout, ldo, k, k, stride,
          ptl[0], ptl[1], 1, 0, act, None if md is None else lib.ptr(md[:, so:]), None if ad is None else lib.ptr(ad[:, so:]), ld2, out_f32)
    ow = ow.cpu()
    if out_f32:
        _check32(ow[:, oo:oo + Cout], ref, ref_in(torch.float32)[0], f'dense {name} {dtype}')
    else:
        a = (k * k * Cin + 1) * EPS32 * mag + (EPS32 * ref.abs() if has_mul or has_add else 0.0)
        _check16(ow[:, oo:oo + Cout], ref, dtype, a, f'dense {name}')
    rest = torch.cat((ow[:, :oo], ow[:, oo + Cout:]), 1)
    assert torch.equal(_bits(rest), _bits(torch.full(rest.shape, 123.0, dtype=t2)))


# (H, W, Ho, Wo, align, in_mode, C, out_f32, normalise)
RESIZE = [
    (5, 7, 10, 14, 1, 0, 40, 0, False),          # the aggregation's x 2
    (5, 7, 10, 14, 1, 0, 40, 1, False),
    (10, 10, 20, 20, 0, 1, 1, 1, False),         # the decoder's x 2 of an fp32 map
    (10, 10, 20, 20, 0, 1, 1, 0, False),
    (10, 10, 20, 20, 1, 1, 3, 1, False),         # same sizes, corners aligned: half a pixel apart from the line above
    (12, 20, 9, 13, 0, 2, 3, 0, True),           # Resize + Normalize of the NCHW fp32 image
    (12, 20, 9, 13, 0, 2, 3, 1, True),
    (12, 20, 9, 13, 1, 2, 3, 1, False),
    (4, 4, 1, 1, 1, 1, 1, 1, False),             # n_out == 1
    (4, 4, 1, 1, 0, 1, 3, 1, True),
    (1, 6, 3, 6, 0, 0, 3, 1, False),             # a single input row
    (1, 6, 3, 6, 1, 0, 3, 0, False),
]


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize('H,W,Ho,Wo,align,in_mode,C,out_f32,norm', RESIZE)
def test_resize(lib, dtype, H, W, Ho, Wo, align, in_mode, C, out_f32, norm):
    """mve_seg_resize against float64 F.interpolate(bilinear) (+ Normalize): every in_mode, both output types, both align_corners.
    MI355X, fp32 outputs, 16 cases: GPU max 1.1e-5 = 1.2e-6 of the scale, CPU-fp32 1.2e-5 = 1.3e-6 of the scale (both in the Normalize cases,
    the division by std); the GPU error exceeds the CPU's in no case, worst GPU / bar 0.125.  16-bit outputs: worst err / bar 0.987."""
    B = 2
    g = _gen(H, W, Ho, align, in_mode, C)
    x = torch.randn(B, C, H, W, generator=g) + 0.5
    x = x.to(dtype) if in_mode == 0 else x
    mean, std = (torch.tensor([0.485, 0.456, 0.406])[:C], torch.tensor([0.229, 0.224, 0.225])[:C]) if norm else (None, None)
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    ref = nhwc(resize_ref(x.double(), Ho, Wo, align, mean, std))
    xd = (x if in_mode == 2 else nhwc(x)).contiguous().to(DEV)
    out = torch.full((B, Ho, Wo, C), float('nan'), dtype=torch.float32 if out_f32 else dtype, device=DEV)
    md, sd = (mean.to(DEV), std.to(DEV)) if norm else (None, None)
    _call(lib, 'mve_seg_resize', _dt(dtype), lib.ptr(xd), B, H, W, C, lib.ptr(out), Ho, Wo, align, in_mode, out_f32, lib.ptr(md), lib.ptr(sd))
    what = f'resize {H}x{W}->{Ho}x{Wo} align{align} in{in_mode} C{C} norm{int(norm)}'
    if out_f32:
        _check32(out, ref, nhwc(resize_ref(x.float(), Ho, Wo, align, mean, std)), f'{what} {dtype}')
    else:
        mag = nhwc(resize_ref(x.double().abs(), Ho, Wo, align))            # three lerps of four corners, then subtract and divide
        if norm:
            mag = (mag + mean.double()) / std.double()
        _check16(out, ref, dtype, 8 * EPS32 * mag, what)


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize('C', [8, 224])
@pytest.mark.parametrize('HW', [1, 255, 256, 257, 1000])
def test_channel_mean(lib, dtype, HW, C):
    """mve_seg_channel_mean: means of inputs with a nonzero mean (a dropped row shows), around the 256-thread stride.
    MI355X, 20 cases: GPU max 1.6e-7 = 9.8e-8 of the scale, CPU-fp32 2.8e-7 = 1.6e-7 of the scale; worst GPU / bar 0.16 (HW 1000, C 8)."""
    B = 2
    x = (torch.randn(B, HW, C, generator=_gen(HW, C)) + 1.5).to(dtype)
    out = torch.full((B, C), float('nan'), device=DEV)
    xd = x.to(DEV)
    _call(lib, 'mve_seg_channel_mean', _dt(dtype), lib.ptr(xd), B, HW, C, lib.ptr(out))
    _check32(out, x.double().mean(1), x.float().mean(1), f'channel_mean HW{HW} C{C} {dtype}')


@pytest.mark.gpu
@pytest.mark.parametrize('nslab,HW', [(1, 1), (1, 4), (5, 35), (67, 4489)])
@pytest.mark.parametrize('C,S', [(32, 8), (288, 12), (3840, 160), (100, 10)])
def test_se_gate(lib, C, S, nslab, HW):
    """mve_seg_se_gate: the gate against float64, and the pooled vector left behind hidden[B * S:] when the finalize step runs (it does not for
    nslab = 1 with scale 1: that part of the workspace keeps its sentinel).
    MI355X, 16 gates and 12 pooled vectors: GPU max 2.5e-7 of the scale, CPU-fp32 8.9e-7 of the scale; worst GPU / bar 0.21 (pooled, C 288,
    nslab 5: GPU 2.0e-7, CPU 1.2e-7)."""
    B, scale = 2, 1.0 / HW
    g = _gen(C, S, nslab)
    sums = (torch.randn(B, nslab, C, generator=g) + 0.5) * HW / nslab
    w1, b1 = torch.randn(S, C, generator=g) * C ** -0.5, 0.3 * torch.randn(S, generator=g)
    w2, b2 = torch.randn(C, S, generator=g) * 2 * S ** -0.5, 0.3 * torch.randn(C, generator=g)
    ref, pooled = se_gate_ref(sums.double(), scale, w1, b1, w2, b2)
    cpu, pooled32 = se_gate_ref(sums, scale, w1, b1, w2, b2)
    assert 0.1 < float(ref.max() - ref.min())
    dev = [t.to(DEV) for t in (sums, w1, b1, w2, b2)]
    hidden = torch.full((B * S + B * C,), 77.0, device=DEV)
    gate = torch.full((B, C), float('nan'), device=DEV)
    _call(lib, 'mve_seg_se_gate', lib.ptr(dev[0]), nslab, scale, B, C, S, *(lib.ptr(t) for t in dev[1:]), lib.ptr(hidden), lib.ptr(gate))
    _check32(gate, ref, cpu, f'se_gate C{C} S{S} nslab{nslab}')
    left = hidden[B * S:].cpu().reshape(B, C)
    if nslab == 1 and HW == 1:
        assert torch.equal(left, torch.full((B, C), 77.0))
    else:
        _check32(left, pooled, pooled32, f'se_gate pooled C{C} nslab{nslab}')


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize('with_s', [False, True])
@pytest.mark.parametrize('in_place', [False, True])
def test_scale(lib, dtype, in_place, with_s):
    """mve_seg_scale: x = src * A[b, c] (+ S[b, c]) with three images of 37 pixels (a wrong image index shows), in place and out of place.
    MI355X: worst err / bar 0.996 (both types)."""
    B, HW, C = 3, 37, 224
    g = _gen(in_place, with_s, 7)
    x = torch.randn(B, HW, C, generator=g).to(dtype)
    A, S = 1 + torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    ref = x.double() * A.double()[:, None] + (S.double()[:, None] if with_s else 0)
    mag = (x.double() * A.double()[:, None]).abs() + (S.double().abs()[:, None] if with_s else 0)
    src, Ad, Sd = x.to(DEV), A.to(DEV), S.to(DEV)
    out = src if in_place else torch.full_like(src, float('nan'))
    _call(lib, 'mve_seg_scale', _dt(dtype), lib.ptr(out), lib.ptr(src), B, HW, C, lib.ptr(Ad), lib.ptr(Sd) if with_s else None)
    _check16(out, ref, dtype, 2 * EPS32 * mag, f'scale in_place{int(in_place)} S{int(with_s)}')
    if not in_place:
        assert torch.equal(_bits(src.cpu()), _bits(x))


@pytest.mark.gpu
@pytest.mark.parametrize('C,tie', UAM_CASES)
def test_uam_channel(lib, C, tie):
    """mve_seg_uam_channel: att, A, S against the float64 channel tracer with torch.quantile(interpolation='linear').  A channel within 1e-6 of the
    threshold may differ in its mask (at most one per image; the CPU test shows the reference has none), but the threshold element itself
    (C = 21: 0.1 * 20 = 2 is an integer position; the tied pair: both sides of the interpolation are equal) must come out masked.
    MI355X, 5 cases, GPU / CPU-fp32 maxima: att 6.4e-7 / 3.7e-7, A 1.3e-6 / 7.5e-7, S 1.3e-7 / 3.6e-8 (at most 8.5e-7 / 4.8e-7 of the scale);
    worst GPU / bar 0.44 (S, C 224).  No channel was excluded."""
    B = 2
    p = uam_channel_inputs(C, tie)
    names = ('pooled', 'ns', 'nb', 'wq', 'wk', 'wv', 'wfc')
    att, A, S, thr = uam_channel_ref(*(p[k].double() for k in names), 0.1, p['bs'].double(), p['bt'].double())
    c_att, c_A, c_S, _ = uam_channel_ref(*(p[k] for k in names), 0.1, p['bs'], p['bt'])
    d = {k: v.to(DEV) for k, v in p.items()}
    got = [torch.full((B, C), float('nan'), device=DEV) for _ in range(3)]
    _call(lib, 'mve_seg_uam_channel', lib.ptr(d['pooled']), B, C, *(lib.ptr(d[k]) for k in names[1:]), 0.1, lib.ptr(d['bs']), lib.ptr(d['bt']),
          *(lib.ptr(t) for t in got))
    g_att, g_A, g_S = (t.cpu() for t in got)
    excl = uam_exclusions(att, thr)
    assert int(excl.sum(1).max()) <= 1
    on = att == thr
    assert bool((g_A[on] == 0).all()) and bool((g_S[on] == 0).all()), 'the threshold element must be masked (<=)'
    assert torch.equal(g_A[~excl] == 0, A[~excl] == 0), 'confidence mask'
    _check32(g_att, att, c_att, f'uam_channel att C{C} tie{int(tie)}')
    _check32(g_A, A, c_A, f'uam_channel A C{C} tie{int(tie)}', keep=~excl)
    _check32(g_S, S, c_S, f'uam_channel S C{C} tie{int(tie)}', keep=~excl)


@pytest.mark.gpu
@pytest.mark.parametrize('H,W', SPATIAL_HW)
def test_uam_spatial(lib, H, W):
    """mve_seg_uam_spatial: softmax(q k^T) v + v over H x W maps with H != W and both strided loops running more than once.
    MI355X: GPU max 2.3e-6 = 4.2e-7 of the scale, CPU-fp32 1.9e-6 = 3.5e-7 of the scale; worst GPU / bar 0.19 (300 x 5)."""
    B = 2
    qkv = uam_spatial_inputs(H, W)
    ref, pmax = uam_spatial_ref(qkv.double(), H, W)
    assert 0.05 < pmax < 0.95
    qd = qkv.to(DEV)
    out = torch.full((B, H * W), float('nan'), device=DEV)
    _call(lib, 'mve_seg_uam_spatial', lib.ptr(qd), B, H, W, lib.ptr(out))
    _check32(out, ref, uam_spatial_ref(qkv, H, W)[0], f'uam_spatial {H}x{W}')


@pytest.mark.gpu
@DTYPES
def test_object_mix(lib, dtype):
    """mve_seg_object_mix at C = 48, HW = 35 with planted pixels on both sides of the 0.93 rule; pixels within 1e-5 of it are left out (at
    most 1 %; the CPU test shows the reference has none).  MI355X: worst err / bar 0.955 (bf16), 0.886 (fp16)."""
    B, HW, C = 2, 35, 48
    d, enc = object_mix_inputs(dtype)
    ref, bg = object_mix_ref(d.double(), enc.double())
    keep = ((bg - 0.93).abs() >= 1e-5)
    assert float((~keep).float().mean()) <= 0.01
    dd, ed = d.to(DEV), enc.to(DEV)
    out = torch.full_like(ed, float('nan'))
    _call(lib, 'mve_seg_object_mix', _dt(dtype), lib.ptr(dd), lib.ptr(ed), lib.ptr(out), B, HW, C)
    _check16(out, ref, dtype, 2.0 ** -20 * enc.double().abs(), 'object_mix', keep=keep[..., None].expand_as(ref))


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize('n', [8, 8 * 257])
def test_mul_and_act(lib, dtype, n):
    """mve_seg_mul (two and three operands) and mve_seg_act (all four activations, SELU on negative inputs) at one vector and at a partial
    last block.  MI355X: worst err / bar 0.994 (mul), 0.969 (swish), 0.973 (SELU), 0 (ReLU), 0.997 (sigmoid, fp16)."""
    g = _gen(n, 11)
    x, y, z = (torch.randn(n, generator=g).to(dtype) for _ in range(3))
    x[:4] = torch.tensor([-3.0, -0.004, -0.5, 2.0]).to(dtype)
    xd, yd, zd = x.to(DEV), y.to(DEV), z.to(DEV)
    for third in (False, True):
        out = torch.full_like(xd, float('nan'))
        _call(lib, 'mve_seg_mul', _dt(dtype), lib.ptr(xd), lib.ptr(yd), lib.ptr(zd) if third else None, lib.ptr(out), n)
        ref = x.double() * y.double() * (z.double() if third else 1)
        _check16(out, ref, dtype, 2 * EPS32 * ref.abs(), f'mul n{n} operands{2 + third}')
    for act in (1, 2, 3, 4):
        t = xd.clone()
        _call(lib, 'mve_seg_act', _dt(dtype), lib.ptr(t), n, act)
        ref = ACT[act](x.double())
        _check16(t, ref, dtype, 0.0, f'act{act} n{n}')
    assert float(ACT[2](x.double())[0]) < -1.6


@pytest.mark.gpu
@pytest.mark.parametrize('Hs,Ws', [(16, 24), (8, 8)])
def test_fuse(lib, Hs, Ws):
    """mve_seg_fuse: sigmoid of the mean of the x 8, x 8 and x 4 bilinear upsamples of three maps on different scales.
    MI355X: GPU max 7.7e-8, CPU-fp32 7.7e-8 (output scale 1); GPU / bar 0.125 in both cases."""
    B = 2
    d0, d1, d2 = fuse_inputs(Hs, Ws)
    ref = fuse_ref(d0.double(), d1.double(), d2.double())
    dev = [t.to(DEV) for t in (d0, d1, d2)]
    out = torch.full((B, Hs, Ws), float('nan'), device=DEV)
    _call(lib, 'mve_seg_fuse', *(lib.ptr(t) for t in dev), B, Hs, Ws, lib.ptr(out))
    _check32(out, ref, fuse_ref(d0, d1, d2), f'fuse {Hs}x{Ws}')


@pytest.mark.gpu
@DTYPES
@pytest.mark.parametrize('out_f32', [0, 1])
@pytest.mark.parametrize('erosion', [0, 1, 2])
@pytest.mark.parametrize('Hs,Ws,Ho,Wo', POST_SIZES)
def test_post(lib, dtype, Hs, Ws, Ho, Wo, erosion, out_f32):
    """mve_seg_post on three images in one launch that take different branches of the failure rule (see post_inputs), against
    -max_pool2d(-m), F.interpolate and the rule in float64, the rule applied to the values rounded to the output type.  Pixels within one
    unit in the last place of 0.8 are left out (at most 2 %; the CPU test checks the cap on the reference).  The workspace starts with every
    byte set, so a per-image flag that the launch leaves uncleared shows.  In the 24 x 16 -> 10 x 12 case without erosion all three images
    fire (the resize passes on a quarter of the low pixel); the other five size / erosion pairs mix the branches.
    MI355X, fp32 outputs, 12 cases: GPU max 8.3e-7, CPU-fp32 8.3e-7 (output scale 1); worst GPU / bar 0.18 (GPU 1.9e-7, CPU 1.3e-7).
    16-bit outputs: bit-equal to the rounded reference in all 12 cases."""
    B = 3
    m = post_inputs(Hs, Ws)
    od = None if out_f32 else dtype
    ref, pre, fire = post_ref(m.double(), erosion, Ho, Wo, od)
    keep = ~post_exclusions(pre, od)
    assert float((~keep).float().mean()) <= 0.02
    md = m.to(DEV)
    # every byte set: a per-image flag that the launch does not clear reads as "not failed" and shows as an unfired rule on image 0 or 2
    ws = torch.full((lib.raw('mve_seg_post_workspace_bytes')(B, Hs, Ws, Ho, Wo),), 255, dtype=torch.uint8, device=DEV)
    out = torch.full((B, Ho, Wo), float('nan'), dtype=torch.float32 if out_f32 else dtype, device=DEV)
    _call(lib, 'mve_seg_post', _dt(dtype), lib.ptr(md), B, Hs, Ws, erosion, lib.ptr(out), Ho, Wo, out_f32, lib.ptr(ws))
    got = out.double().cpu()
    assert torch.equal((got == 0)[keep], (ref == 0)[keep]), ('failure rule', fire.tolist())
    what = f'post {Hs}x{Ws}->{Ho}x{Wo} erosion{erosion} {dtype}'
    if out_f32:
        _check32(out, ref, post_ref(m, erosion, Ho, Wo, None)[0], what, keep=keep)
    else:
        _check16(out, ref, dtype, 8 * EPS32, what, keep=keep)                  # three lerps of values <= 1
