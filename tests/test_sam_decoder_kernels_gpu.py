"""Every kernel of csrc/sam_decoder.hip alone, through its C entry point, against the float64 numpy rule (tests/sam_decoder_rule.py).

Bar: the kernel's rel-L2 against float64 is at most 4 x that of torch's fp32 CPU ops on the same inputs (computed here, on the host).  Where torch's
fp32 result is exact (copies, the zero pad) the kernel's must be too.  Masks must equal `own logits > threshold` exactly."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sam_decoder_rule as R  # noqa: E402

FACTOR = 4.0


def lib():
    from mvedit_amd import _lib
    return _lib


def dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def call(name, *args):
    L = lib()
    L.call(name, *[L.ptr(a) if torch.is_tensor(a) else a for a in args], L.stream_ptr())
    torch.cuda.synchronize()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def check(got, want, torch_fp32, what=''):
    """the bar: 4 x torch's fp32 CPU error against the float64 rule"""
    got = got.double().cpu().numpy() if torch.is_tensor(got) else got
    t32 = torch_fp32.double().numpy() if torch.is_tensor(torch_fp32) else torch_fp32
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, bar = rel_l2(got, want), FACTOR * rel_l2(t32, want)
    print(f'    {what}: kernel {err:.3e}, torch fp32 {bar / FACTOR:.3e}')
    assert err <= bar, (what, err, bar)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


# ---- attention ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Lq,Lk,hd', [(7, 7, 32), (9, 9, 32), (7, 144, 16), (9, 256, 16), (7, 4096, 16), (144, 7, 16), (4096, 9, 16), (5, 1, 16), (3, 16, 32), (3, 17, 32)])
def test_attention_f32(Lq, Lk, hd):
    """the three regimes (tokens x tokens, tokens x image with a tail that is no multiple of 256, image x tokens), Lk = 1, and both sides of the Lk = 16
    switch between the two kernels"""
    rs, N, heads = np.random.RandomState(Lq * 1000 + Lk), 2, 8
    D = heads * hd
    q, k, v = rs.standard_normal((N, Lq, D)), rs.standard_normal((N, Lk, D)), rs.standard_normal((N, Lk, D))
    want = R.attention(q, k, v, heads)
    sp = lambda t: t32(t).reshape(N, -1, heads, hd).transpose(1, 2)
    ref32 = (torch.softmax(sp(q) @ sp(k).transpose(2, 3) * hd ** -0.5, dim=-1) @ sp(v)).transpose(1, 2).reshape(N, Lq, D)
    # strided operands: q | k | v rows inside wider buffers
    pad = 8
    Q, K, V = (torch.zeros(N, L, D + pad, device='cuda') for L in (Lq, Lk, Lk))
    Q[..., :D], K[..., :D], V[..., :D] = dev(q), dev(k), dev(v)
    O = torch.full((N, Lq, D + pad), 7.0, device='cuda')
    call('mve_attention_f32', Q, D + pad, K, D + pad, V, D + pad, O, D + pad, N, Lq, Lk, heads, hd, float(hd ** -0.5))
    assert bool((O[..., D:] == 7.0).all()), 'the kernel wrote outside its columns'
    check(O[..., :D], want, ref32, f'attention {Lq} x {Lk} hd {hd}')
    # an item alone gives the same bits
    O1 = torch.empty(1, Lq, D, device='cuda')
    call('mve_attention_f32', Q[1], D + pad, K[1], D + pad, V[1], D + pad, O1, D, 1, Lq, Lk, heads, hd, float(hd ** -0.5))
    assert torch.equal(O1[0], O[1, :, :D])


@pytest.mark.parametrize('Lk', [9, 300])
def test_attention_f32_subtracts_the_maximum(Lk):
    """a logit row of +80 against -80: without the max subtraction exp(80 * ...) overflows fp32"""
    N, heads, hd, Lq = 1, 8, 16, 4
    D = heads * hd
    q = np.full((N, Lq, D), 80.0 / 4.0)
    k = np.zeros((N, Lk, D))
    k[:, ::2, ::hd] = 16.0       # logit (80 / 4 * 16) / 4 = +80 on even keys, -80 on odd ones
    k[:, 1::2, ::hd] = -16.0
    v = np.random.RandomState(5).standard_normal((N, Lk, D))
    want = R.attention(q, k, v, heads)
    O = torch.empty(N, Lq, D, device='cuda')
    call('mve_attention_f32', dev(q), D, dev(k), D, dev(v), D, O, D, N, Lq, Lk, heads, hd, float(hd ** -0.5))
    assert bool(torch.isfinite(O).all())
    sp = lambda t: t32(t).reshape(N, -1, heads, hd).transpose(1, 2)
    ref32 = (torch.softmax(sp(q) @ sp(k).transpose(2, 3) * hd ** -0.5, dim=-1) @ sp(v)).transpose(1, 2).reshape(N, Lq, D)
    check(O, want, ref32, f'attention +80 / -80, Lk {Lk}')


@pytest.mark.parametrize('Lk', [9, 300])
def test_attention_f32_on_ascending_logits(Lk):
    """logits strictly ascending along the keys (one q . k channel per head, 30 j / Lk on row 0, up to 2.5 x steeper on the rows below; inputs exact
    in fp32): every key is a new maximum, so every step of the short kernel's online softmax, every per-thread step and every level of the long
    kernel's tree merge rescales what it holds"""
    N, heads, hd, Lq = 2, 8, 16, 7
    D = heads * hd
    rs = np.random.RandomState(Lk)
    q, k = np.zeros((N, Lq, D)), np.zeros((N, Lk, D))
    q[:, :, ::hd] = 4.0 * (1 + 0.25 * np.arange(Lq))[None, :, None]          # x scale 1/4: the logit is (1 + 0.25 row) k
    k[:, :, ::hd] = (30.0 * np.arange(Lk) / Lk).astype(np.float32)[None, :, None]
    v = rs.standard_normal((N, Lk, D)).astype(np.float32).astype(np.float64)
    s = (q.reshape(N, Lq, heads, hd).transpose(0, 2, 1, 3) @ k.reshape(N, Lk, heads, hd).transpose(0, 2, 3, 1)) * hd ** -0.5
    assert (np.diff(s, axis=-1) > 0).all()
    want = R.attention(q, k, v, heads)
    O = torch.empty(N, Lq, D, device='cuda')
    call('mve_attention_f32', dev(q), D, dev(k), D, dev(v), D, O, D, N, Lq, Lk, heads, hd, float(hd ** -0.5))
    assert bool(torch.isfinite(O).all())
    sp = lambda t: t32(t).reshape(N, -1, heads, hd).transpose(1, 2)
    ref32 = (torch.softmax(sp(q) @ sp(k).transpose(2, 3) * hd ** -0.5, dim=-1) @ sp(v)).transpose(1, 2).reshape(N, Lq, D)
    check(O, want, ref32, f'attention on ascending logits, Lk {Lk}')


# ---- GEMM -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,K', [(128, 256), (256, 128), (2048, 256), (256, 2048), (256, 256), (128, 64)])
@pytest.mark.parametrize('M', [1, 7, 9, 144, 4096])
def test_gemm_f32(M, N, K):
    rs = np.random.RandomState(M + N + K)
    A, W, bias, res = rs.standard_normal((M, K)), rs.standard_normal((N, K)) * K ** -0.5, rs.standard_normal(N), rs.standard_normal((M, N))
    dA, dW, db, dr = dev(A), dev(W), dev(bias), dev(res)
    for use_b, use_r, relu in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)):
        want = R.gemm(A, W, bias if use_b else None, res if use_r else None, bool(relu))
        y32 = F.linear(t32(A), t32(W), t32(bias) if use_b else None)
        if use_r:
            y32 = y32 + t32(res)
        if relu:
            y32 = torch.relu(y32)
        out = torch.empty(M, N, device='cuda')
        call('mve_gemm_f32', dA, K, dW, K, db if use_b else None, dr if use_r else None, N, out, N, M, N, K, relu)
        check(out, want, y32, f'gemm {M} x {N} x {K} bias {use_b} res {use_r} relu {relu}')
    if M > 1:       # a row alone gives the bits it has in the matrix
        one = torch.empty(1, N, device='cuda')
        call('mve_gemm_f32', dA[M - 1:], K, dW, K, None, None, N, one, N, 1, N, K, 0)
        assert torch.equal(one[0], out[M - 1])


def test_layernorm_and_add_rows_f32():
    rs = np.random.RandomState(11)
    x, g, b, pe = rs.standard_normal((37, 256)) * 3 + 1, rs.standard_normal(256), rs.standard_normal(256), rs.standard_normal((12, 256))
    y = torch.empty(37, 256, device='cuda')
    for eps in (1e-5, 1e-6):
        call('mve_layernorm_f32', dev(x), y, 37, 256, dev(g), dev(b), eps)
        check(y, R.layernorm(x, g, b, eps), F.layer_norm(t32(x), (256,), t32(g), t32(b), eps), f'layernorm eps {eps}')
    x = x[:36]
    y = torch.empty(36, 256, device='cuda')
    call('mve_add_rows_f32', dev(x), dev(pe), y, 36, 256, 12)
    want = (x.reshape(3, 12, 256) + pe).reshape(36, 256)
    assert np.array_equal(y.cpu().numpy(), (t32(x).reshape(3, 12, 256) + t32(pe)).reshape(36, 256).numpy()) and rel_l2(y.cpu().numpy(), want) < 1e-7


# ---- upscale, token MLPs, mask product --------------------------------------------------------------------------------------------------------------
def pack_w4(w):
    """ConvTranspose2d weight [Cin, Cout, 2, 2] -> the GEMM operand [(2 ky + kx) Cout + co][Cin]"""
    return np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(4 * w.shape[1], w.shape[0]))


@pytest.mark.parametrize('G', [12, 16])
def test_upscale(G):
    """both stages: the order of the four sub-pixels (a weight that differs per (ky, kx)) and LayerNorm2d over the channels of a pixel"""
    rs, N, C = np.random.RandomState(G), 2, 256
    x = rs.standard_normal((N, G, G, C))
    w1, b1 = rs.standard_normal((C, C // 4, 2, 2)) * C ** -0.5 * np.array([[1.0, 0.5], [2.0, -1.0]]), rs.standard_normal(C // 4) * 0.1
    g, b = 1 + 0.1 * rs.standard_normal(C // 4), 0.1 * rs.standard_normal(C // 4)
    w2, b2 = rs.standard_normal((C // 4, C // 8, 2, 2)) * (C // 4) ** -0.5 * np.array([[1.0, -0.5], [0.25, 2.0]]), rs.standard_normal(C // 8) * 0.1
    u1 = R.upscale(x, w1, b1, g, b, 1e-6, 1)
    u2 = R.upscale(u1, w2, b2, mode=2)
    nchw = lambda a: t32(a).permute(0, 3, 1, 2)
    t1 = F.conv_transpose2d(nchw(x), t32(w1), t32(b1), stride=2)
    t1 = F.gelu(F.layer_norm(t1.permute(0, 2, 3, 1), (C // 4,), t32(g), t32(b), 1e-6))
    t2 = F.gelu(F.conv_transpose2d(nchw(u1), t32(w2), t32(b2), stride=2)).permute(0, 2, 3, 1)
    tmp = torch.empty(N * G * G * C, device='cuda')
    o1 = torch.empty(N, 2 * G, 2 * G, C // 4, device='cuda')
    call('mve_sam_upscale', dev(x), dev(pack_w4(w1)), dev(b1), dev(g), dev(b), 1e-6, tmp, o1, N, G, C, C // 4, 1)
    check(o1, u1, t1, f'upscale_conv1 + LayerNorm2d + GELU, G {G}')
    tmp = torch.empty(N * 4 * G * G * 4 * (C // 8), device='cuda')
    o2 = torch.empty(N, 4 * G, 4 * G, C // 8, device='cuda')
    call('mve_sam_upscale', dev(u1), dev(pack_w4(w2)), dev(b2), None, None, 0.0, tmp, o2, N, 2 * G, C // 4, C // 8, 2)
    check(o2, u2, t2, f'upscale_conv2 + GELU, G {G}')


def test_token_mlps_and_mask_product():
    rs, N, T, C, Mt = np.random.RandomState(21), 3, 9, 256, 4
    sd = {}
    heads = [f'mask_decoder.output_hypernetworks_mlps.{m}' for m in range(Mt)] + ['mask_decoder.iou_prediction_head']
    for j, h in enumerate(heads):
        for n, no in (('proj_in', C), ('layers.0', C), ('proj_out', C // 8 if j < Mt else Mt)):
            sd[f'{h}.{n}.weight'], sd[f'{h}.{n}.bias'] = rs.standard_normal((no, C)) * (2 / C) ** 0.5, rs.standard_normal(no) * 0.1
    q = rs.standard_normal((N, T, C))
    hyper, iou = R.token_mlps(sd, q, Mt)
    sd32 = {k: t32(v) for k, v in sd.items()}
    ff = lambda h, x: F.linear(torch.relu(F.linear(torch.relu(F.linear(x, sd32[h + '.proj_in.weight'], sd32[h + '.proj_in.bias'])), sd32[h + '.layers.0.weight'],
                                                              sd32[h + '.layers.0.bias'])), sd32[h + '.proj_out.weight'], sd32[h + '.proj_out.bias'])
    hyper32 = torch.stack([ff(heads[m], t32(q)[:, 1 + m]) for m in range(Mt)], dim=1)
    iou32 = ff(heads[Mt], t32(q)[:, 0])
    stack = lambda n, rows: np.stack([np.concatenate([sd[f'{h}.{n}.weight'], np.zeros((rows - sd[f'{h}.{n}.weight'].shape[0], C))]) for h in heads])
    stackb = lambda n, rows: np.stack([np.concatenate([sd[f'{h}.{n}.bias'], np.zeros(rows - sd[f'{h}.{n}.bias'].shape[0])]) for h in heads])
    dh, di = torch.empty(N, Mt, C // 8, device='cuda'), torch.empty(N, Mt, device='cuda')
    call('mve_sam_token_mlps', dev(q), N, T, C, C, C // 8, Mt, dev(stack('proj_in', C)), dev(stackb('proj_in', C)), dev(stack('layers.0', C)), dev(stackb('layers.0', C)),
         dev(stack('proj_out', C // 8)), dev(stackb('proj_out', C // 8)), dh, di)
    check(dh, hyper, hyper32, 'hypernetwork MLPs')
    check(di, iou, iou32, 'iou head')
    up = rs.standard_normal((N, 48 * 48 + 5, C // 8))
    low = torch.empty(N, Mt, up.shape[1], device='cuda')
    call('mve_sam_mask_product', dev(hyper), dev(up), low, N, Mt, C // 8, up.shape[1])
    check(low, R.mask_product(hyper, up), t32(hyper) @ t32(up).transpose(1, 2), 'mask product')


# ---- prompt encoder -------------------------------------------------------------------------------------------------------------------------------
def prompt_sd(rs, C, Mt):
    sd = {'shared_image_embedding.positional_embedding': rs.standard_normal((2, C // 2)), 'prompt_encoder.not_a_point_embed.weight': rs.standard_normal((1, C)),
          'mask_decoder.iou_token.weight': rs.standard_normal((1, C)), 'mask_decoder.mask_tokens.weight': rs.standard_normal((Mt, C))}
    for k in range(4):
        sd[f'prompt_encoder.point_embed.{k}.weight'] = rs.standard_normal((1, C))
    return {k: v.astype(np.float32).astype(np.float64) for k, v in sd.items()}


def torch_pos_enc(coords01, gaussian):
    v = 2 * np.pi * ((2 * t32(coords01) - 1) @ t32(gaussian))
    return torch.cat([torch.sin(v), torch.cos(v)], dim=-1)


@pytest.mark.parametrize('G', [12, 16])
def test_dense_pe(G):
    g = prompt_sd(np.random.RandomState(31), 256, 4)['shared_image_embedding.positional_embedding']
    out = torch.empty(G * G, 256, device='cuda')
    call('mve_sam_dense_pe', dev(g), out, G, 256)
    c = (torch.arange(G, dtype=torch.float32) + 0.5) / G
    xy = torch.stack(torch.meshgrid(c, c, indexing='xy'), dim=-1)
    check(out, R.dense_pe(g, G), torch_pos_enc(xy.numpy(), g).reshape(G * G, 256), f'dense pe, G {G}')


@pytest.mark.parametrize('box,n_points', [(True, 0), (True, 3), (False, 3), (False, 1)])
def test_prompt_tokens(box, n_points):
    """labels -1 / 0 / 1, the box corners, and the padding point that points without a box get"""
    rs, N, C, Mt, S = np.random.RandomState(41 + n_points), 3, 256, 4, 192.0
    sd = prompt_sd(rs, C, Mt)
    boxes = np.round(rs.uniform(0, S, (N, 4)) * 4) / 4 if box else None
    points = np.round(rs.uniform(0, S, (N, n_points, 2)) * 4) / 4 if n_points else None
    labels = np.stack([np.roll(np.array([1, 0, -1])[:n_points], i) for i in range(N)]) if n_points else None
    want = R.prompt_tokens(sd, boxes, points, labels, S)
    T = want.shape[1]
    assert T == 1 + Mt + n_points + (1 if n_points and not box else 0) + (2 if box else 0)
    out = torch.empty(N, T, C, device='cuda')
    pe = np.concatenate([sd[f'prompt_encoder.point_embed.{k}.weight'] for k in range(4)])
    call('mve_sam_prompt_tokens', dev(boxes), dev(points), dev(labels, torch.int32), N, n_points, dev(sd['shared_image_embedding.positional_embedding']), dev(pe),
         dev(sd['prompt_encoder.not_a_point_embed.weight']), dev(sd['mask_decoder.iou_token.weight']), dev(sd['mask_decoder.mask_tokens.weight']), Mt, C, S, out, T)
    got = out.cpu().numpy()
    # the fp32 statement with torch ops: the same rule in float32
    sd32 = {k: v.astype(np.float32) for k, v in sd.items()}
    parts = [np.broadcast_to(np.concatenate([sd32['mask_decoder.iou_token.weight'], sd32['mask_decoder.mask_tokens.weight']]), (N, 1 + Mt, C))]
    if n_points:
        p, l = points, labels
        if not box:
            p, l = np.concatenate([p, np.zeros((N, 1, 2))], 1), np.concatenate([l, -np.ones((N, 1), l.dtype)], 1)
        e = torch_pos_enc(((t32(p) + 0.5) / S).numpy(), sd['shared_image_embedding.positional_embedding']).numpy()
        e = np.where((l == -1)[..., None], sd32['prompt_encoder.not_a_point_embed.weight'][0], e)
        e = e + np.where((l == 0)[..., None], pe[0].astype(np.float32), 0) + np.where((l == 1)[..., None], pe[1].astype(np.float32), 0)
        parts.append(e.astype(np.float32))
    if box:
        e = torch_pos_enc(((t32(boxes).reshape(N, 2, 2) + 0.5) / S).numpy(), sd['shared_image_embedding.positional_embedding']).numpy()
        parts.append((e + np.stack([pe[2], pe[3]]).astype(np.float32)).astype(np.float32))
    ref32 = np.concatenate(parts, axis=1)
    assert np.array_equal(got[:, :1 + Mt], ref32[:, :1 + Mt]), 'the output tokens are copies'
    if n_points:
        assert np.array_equal(got[:, 1 + Mt:][labels_full(labels, box, N) == -1], ref32[:, 1 + Mt:][labels_full(labels, box, N) == -1]), 'label -1 rows are not_a_point_embed'
    check(got, want, ref32, f'prompt tokens box {box} points {n_points}')


def labels_full(labels, box, N):
    """labels of every sparse token: the points', -1 for the padding point, 2 for box corners"""
    l = labels if box else np.concatenate([labels, -np.ones((N, 1), labels.dtype)], 1)
    return np.concatenate([l, np.full((N, 2), 2)], 1) if box else l


def test_sam_src():
    rs, B, P, C, G = np.random.RandomState(51), 2, 3, 256, 12
    emb, nm = rs.standard_normal((B, C, G, G)).astype(np.float16), rs.standard_normal(C)
    from mvedit_amd.ops import dt as dtcode
    for dt in (torch.float16, torch.bfloat16):
        e = torch.from_numpy(emb).to(dt)
        out = torch.empty(B * P, G * G, C, device='cuda')
        call('mve_sam_src', dtcode(dt), e.cuda(), dev(nm), out, B * P, P, C, G)
        want32 = (e.float().reshape(B, C, G * G).transpose(1, 2) + t32(nm)).repeat_interleave(P, 0)
        assert torch.equal(out.cpu(), want32), dt          # one fp32 add per element: the same bits as torch's
        assert rel_l2(out.cpu().numpy(), R.src_rows(e.double().numpy(), nm, P)) < 1e-7


# ---- pre- and post-processing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(150, 192), (192, 143), (192, 192)])
def test_preprocess(h, w):
    from mvedit_amd.sam import preprocess_image
    S = 192
    img = np.random.RandomState(h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    want = R.preprocess(img, S)
    for dt in (torch.float16, torch.bfloat16):
        out = preprocess_image(torch.from_numpy(img).cuda(), S, dt).float().cpu()
        ref32 = torch.zeros(1, 3, S, S)
        ref32[0, :, :h, :w] = ((t32(img) - torch.tensor(R.PIXEL_MEAN)) / torch.tensor(R.PIXEL_STD)).permute(2, 0, 1)
        ref = ref32.to(dt).float()
        assert not out[0, :, h:].any() and not out[0, :, :, w:].any(), 'the pad region is exactly zero'
        check(out, want, ref, f'preprocess {h} x {w} {dt}')
    custom = preprocess_image(torch.from_numpy(img).cuda(), S, torch.float16, (10.0, 20.0, 30.0), (2.0, 4.0, 8.0)).float().cpu().numpy()
    assert rel_l2(custom, R.preprocess(img, S, (10.0, 20.0, 30.0), (2.0, 4.0, 8.0))) < 1e-3


@pytest.mark.parametrize('L,S,h_in,w_in,H,W', [(64, 256, 192, 256, 150, 200), (64, 256, 256, 238, 300, 279), (48, 192, 192, 192, 192, 192)])
def test_postprocess(L, S, h_in, w_in, H, W):
    from mvedit_amd.sam import postprocess_masks
    low = np.random.RandomState(L + H).standard_normal((2, 3, L, L)) * 4
    want = R.postprocess(low, S, h_in, w_in, H, W)
    ref32 = F.interpolate(F.interpolate(t32(low), (S, S), mode='bilinear', align_corners=False)[..., :h_in, :w_in], (H, W), mode='bilinear', align_corners=False)
    for thr in (0.0, 0.75):
        masks, logits = postprocess_masks(dev(low), S, (h_in, w_in), (H, W), thr, True)
        assert masks.dtype == torch.bool and masks.shape == (2, 3, H, W)
        assert torch.equal(masks, logits > thr), 'the mask is exactly own logits > threshold'
        check(logits, want, ref32, f'postprocess {L} -> {S} -> [{h_in}, {w_in}] -> ({H}, {W})')
        only, none = postprocess_masks(dev(low), S, (h_in, w_in), (H, W), thr, False)
        assert none is None and torch.equal(only, masks)


def test_layernorm_f32_on_hard_row_statistics():
    """mve_layernorm_f32 on the row statistics of tests/hard_stats.py (unrounded fp32 inputs): a row mean of up to 256 standard deviations, an outlier
    channel, constant rows, rows whose variance is below eps.  Same bar as above: 4 x the error of torch's fp32 CPU LayerNorm against float64.
    The constant rows of the `constant` family are held to an absolute bound instead (torch's Welford mean of equal values is exact, so a bar relative to
    its error allows nothing there): the kernel's mean is 3 sequential adds per lane, 6 tree levels and a division, each rounding at most 2^-24 of the
    row's value x, and a mean off by dm moves every output of the row by |g_c| dm / sqrt(var + eps) with var = 0; the last multiply-adds round the output
    itself.  So |err[m, c]| <= 10 * 2^-24 |x_m| |g_c| / sqrt(eps) + 4 * 2^-24 |ref[m, c]|."""
    import hard_stats as H
    rs = np.random.RandomState(12)
    M, C = 37, 256
    g, b = rs.standard_normal(C), rs.standard_normal(C)
    y = torch.empty(M, C, device='cuda')
    for fam in H.FAMILIES:
        x = H.make_rows(fam, M, C, None, 8).numpy()
        const = np.zeros(M, bool)
        if fam == 'constant':
            const = (x == x[:, :1]).all(axis=1)
            assert const.sum() == (M + H.SPECIAL_EVERY - 1) // H.SPECIAL_EVERY
        for eps in (1e-5, 1e-6):
            call('mve_layernorm_f32', dev(x), y, M, C, dev(g), dev(b), eps)
            want, t = R.layernorm(x, g, b, eps), F.layer_norm(t32(x), (C,), t32(g), t32(b), eps)
            check(y[torch.from_numpy(~const).cuda()], want[~const], t[torch.from_numpy(~const)], f'layernorm {fam} eps {eps}')
            if const.any():
                err = np.abs(y.double().cpu().numpy() - want)[const]
                bound = 10 * 2.0 ** -24 * np.abs(x[const][:, :1].astype(np.float64)) * np.abs(g)[None, :] / np.sqrt(eps) + 4 * 2.0 ** -24 * np.abs(want[const])
                print(f'    layernorm constant rows eps {eps}: worst err / bound {float((err / bound).max()):.3f}')
                assert (err <= bound).all(), (fam, eps, float((err / bound).max()))
