"""The arithmetic of Segment Anything's image encoder, stated in numpy float64 -- the rule the SAM kernels and the SAM engine are held to
(tests/test_sam_kernels_gpu.py, tests/test_sam_encoder_gpu.py) and that tests/test_sam_surface.py holds against transformers' own
SamVisionEncoder through the golden (tests/golden/make_sam_encoder_golden.py).  Nothing here imports torch or transformers.

    relpos_attention   softmax_k( scale q.k + q.Rh[qh - kh + gh - 1] + q.Rw[qw - kw + gw - 1] ) v per (sequence, head), the UNSCALED q against the tables
    window_partition   [B, G, G, C] -> [B * nw * nw, w * w, C], zero-padded at the bottom and right to nw * w (nw = ceil(G / w))
    window_unpartition the inverse; the padded rows are dropped
    encoder_forward    the whole encoder from a transformers-named state dict: hidden states and the neck output
"""
import math

import numpy as np


def relpos_probabilities(q, k, rel_h, rel_w, gh, gw, scale):
    """q, k [NS, gh * gw, heads, hd]; rel_h [2 gh - 1, hd], rel_w [2 gw - 1, hd] -> the attention probabilities [NS, heads, L, L], float64."""
    q, k, rel_h, rel_w = (np.asarray(t, np.float64) for t in (q, k, rel_h, rel_w))
    NS, L, H, D = q.shape
    assert L == gh * gw and rel_h.shape == (2 * gh - 1, D) and rel_w.shape == (2 * gw - 1, D)
    Rh = rel_h[np.arange(gh)[:, None] - np.arange(gh)[None, :] + gh - 1]          # [qh, kh, D]
    Rw = rel_w[np.arange(gw)[:, None] - np.arange(gw)[None, :] + gw - 1]          # [qw, kw, D]
    q5 = q.reshape(NS, gh, gw, H, D)
    bias_h = np.einsum('nyxhd,ykd->nhyxk', q5, Rh)                                # [NS, H, qh, qw, kh]
    bias_w = np.einsum('nyxhd,xkd->nhyxk', q5, Rw)                                # [NS, H, qh, qw, kw]
    s = scale * np.einsum('nqhd,nkhd->nhqk', q, k)
    s = s.reshape(NS, H, gh, gw, gh, gw) + bias_h[..., :, None] + bias_w[..., None, :]
    s = s.reshape(NS, H, L, L)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return p


def relpos_attention(q, k, v, rel_h, rel_w, gh, gw, scale):
    """q, k, v [NS, gh * gw, heads, hd] -> [NS, gh * gw, heads, hd], float64."""
    return np.einsum('nhqk,nkhd->nqhd', relpos_probabilities(q, k, rel_h, rel_w, gh, gw, scale), np.asarray(v, np.float64))


def window_partition(x, w):
    B, G, _, C = x.shape
    nw = -(-G // w)
    pad = np.zeros((B, nw * w, nw * w, C), x.dtype)
    pad[:, :G, :G] = x
    return pad.reshape(B, nw, w, nw, w, C).transpose(0, 1, 3, 2, 4, 5).reshape(B * nw * nw, w * w, C)


def window_unpartition(win, B, G, w):
    nw = -(-G // w)
    C = win.shape[-1]
    x = win.reshape(B, nw, nw, w, w, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, nw * w, nw * w, C)
    return np.ascontiguousarray(x[:, :G, :G])


def layer_norm(x, g, b, eps):
    mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def patch_rows(px, P):
    """[B, 3, S, S] -> [B, G, G, 3 P P] in (channel, ky, kx) order: the order of weight.reshape(C, -1)."""
    B, Cin, S, _ = px.shape
    G = S // P
    return px.reshape(B, Cin, G, P, G, P).transpose(0, 2, 4, 1, 3, 5).reshape(B, G, G, Cin * P * P)


def conv3x3(x, wgt):
    """x [B, H, W, Cin] NHWC, wgt [Cout, Cin, 3, 3], padding 1, no bias -> [B, H, W, Cout]"""
    B, H, W, _ = x.shape
    pad = np.zeros((B, H + 2, W + 2, x.shape[-1]), x.dtype)
    pad[:, 1:-1, 1:-1] = x
    out = 0.0
    for ky in range(3):
        for kx in range(3):
            out = out + pad[:, ky:ky + H, kx:kx + W] @ wgt[:, :, ky, kx].T
    return out


def block_forward(sd, cfg, k, x, keep=None):
    """One SamVisionLayer on x [B, G, G, C]; keep: a dict that receives the block's q, k, v and attention output ([NS, L, heads, hd])."""
    B, G, _, C = x.shape
    H = cfg['num_attention_heads']
    D = C // H
    p = f'layers.{k}.'
    w = 0 if k in cfg['global_attn_indexes'] else cfg['window_size']
    n = layer_norm(x, sd[p + 'layer_norm1.weight'], sd[p + 'layer_norm1.bias'], cfg['layer_norm_eps'])
    seq = window_partition(n, w) if w else n.reshape(B, G * G, C)
    g = w if w else G
    qkv = seq @ sd[p + 'attn.qkv.weight'].T + sd[p + 'attn.qkv.bias']
    NS, L, _ = qkv.shape
    q, kk, v = (qkv[..., i * C:(i + 1) * C].reshape(NS, L, H, D) for i in range(3))
    a = relpos_attention(q, kk, v, sd[p + 'attn.rel_pos_h'], sd[p + 'attn.rel_pos_w'], g, g, D ** -0.5)
    if keep is not None:
        keep.update(q=q, k=kk, v=v, out=a, grid=g, rel_h=sd[p + 'attn.rel_pos_h'], rel_w=sd[p + 'attn.rel_pos_w'])
    a = a.reshape(NS, L, C) @ sd[p + 'attn.proj.weight'].T + sd[p + 'attn.proj.bias']
    a = window_unpartition(a, B, G, w) if w else a.reshape(B, G, G, C)
    x = x + a
    m = layer_norm(x, sd[p + 'layer_norm2.weight'], sd[p + 'layer_norm2.bias'], cfg['layer_norm_eps'])
    m = gelu(m @ sd[p + 'mlp.lin1.weight'].T + sd[p + 'mlp.lin1.bias']) @ sd[p + 'mlp.lin2.weight'].T + sd[p + 'mlp.lin2.bias']
    return x + m


def encoder_forward(sd, cfg, px):
    """-> (hidden_states: num_hidden_layers + 1 arrays [B, G, G, C], neck output [B, O, G, G]) in float64; sd under transformers' names."""
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    C = cfg['hidden_size']
    x = patch_rows(np.asarray(px, np.float64), cfg['patch_size']) @ sd['patch_embed.projection.weight'].reshape(C, -1).T + sd['patch_embed.projection.bias']
    x = x + sd['pos_embed']
    hs = [x]
    for k in range(cfg['num_hidden_layers']):
        x = block_forward(sd, cfg, k, x)
        hs.append(x)
    y = x @ sd['neck.conv1.weight'].reshape(cfg['output_channels'], C).T
    y = layer_norm(y, sd['neck.layer_norm1.weight'], sd['neck.layer_norm1.bias'], 1e-6)
    y = conv3x3(y, sd['neck.conv2.weight'])
    y = layer_norm(y, sd['neck.layer_norm2.weight'], sd['neck.layer_norm2.bias'], 1e-6)
    return hs, np.ascontiguousarray(y.transpose(0, 3, 1, 2))
