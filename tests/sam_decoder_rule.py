"""float64 numpy statement of the SAM prompt encoder, two-way mask decoder and mask post-processing (transformers' SamPromptEncoder / SamMaskDecoder /
SamPositionalEmbedding, models/sam/modeling_sam.py; `Sam.preprocess` / `Sam.postprocess_masks` of segment_anything): the rule each kernel of
csrc/sam_decoder.hip is tested against, one function per kernel, and `decoder_forward` for the whole plan.  tests/test_sam_predictor_surface.py asserts
that `decoder_forward` reproduces transformers' float64 module to 1e-9.  State-dict names are transformers' (`SamModel.state_dict()`)."""
import numpy as np
import torch

PIXEL_MEAN, PIXEL_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(f64(x)))).numpy()


def gelu(x):
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def pos_enc(coords01, gaussian):
    """coords01 [..., 2] in [0, 1] (x, y), gaussian [2, C/2] -> [..., C] = [sin | cos] of 2 pi ((2 c - 1) @ gaussian)"""
    v = 2.0 * np.pi * ((2.0 * f64(coords01) - 1.0) @ f64(gaussian))
    return np.concatenate([np.sin(v), np.cos(v)], axis=-1)


def dense_pe(gaussian, G):
    """-> [G * G, C]: cell (i, j) at ((j + 0.5) / G, (i + 0.5) / G)"""
    c = (np.arange(G) + 0.5) / G
    xy = np.stack(np.meshgrid(c, c, indexing='xy'), axis=-1)      # [i, j] = (x_j, y_i)
    return pos_enc(xy, gaussian).reshape(G * G, -1)


def prompt_tokens(sd, boxes, points, labels, image_size):
    """boxes [N, 4] | None, points [N, n, 2] | None, labels [N, n] -> [N, T, C]: iou token, mask tokens, points (+ padding point without a box), corners"""
    g = f64(sd['shared_image_embedding.positional_embedding'])
    pe = [f64(sd[f'prompt_encoder.point_embed.{k}.weight'])[0] for k in range(4)]
    nap = f64(sd['prompt_encoder.not_a_point_embed.weight'])[0]
    out_tokens = np.concatenate([f64(sd['mask_decoder.iou_token.weight']), f64(sd['mask_decoder.mask_tokens.weight'])], axis=0)
    N = len(boxes) if boxes is not None else len(points)
    parts = [np.broadcast_to(out_tokens, (N,) + out_tokens.shape)]
    if points is not None:
        points, labels = f64(points), np.asarray(labels)
        if boxes is None:
            points = np.concatenate([points, np.zeros((N, 1, 2))], axis=1)
            labels = np.concatenate([labels, -np.ones((N, 1), labels.dtype)], axis=1)
        e = pos_enc((points + 0.5) / image_size, g)
        e = np.where((labels == -1)[..., None], nap, e)
        e = e + np.where((labels == 0)[..., None], pe[0], 0.0) + np.where((labels == 1)[..., None], pe[1], 0.0)
        parts.append(e)
    if boxes is not None:
        e = pos_enc((f64(boxes).reshape(N, 2, 2) + 0.5) / image_size, g)
        e[:, 0] += pe[2]
        e[:, 1] += pe[3]
        parts.append(e)
    return np.concatenate(parts, axis=1)


def src_rows(embedding, no_mask, P):
    """embedding [B, C, G, G] -> [B * P, G * G, C] rows of image n // P, + no_mask_embed"""
    B, C = embedding.shape[:2]
    rows = f64(embedding).reshape(B, C, -1).transpose(0, 2, 1) + f64(no_mask).reshape(1, 1, C)
    return np.repeat(rows, P, axis=0)


def gemm(A, W, bias=None, res=None, relu=False):
    y = f64(A) @ f64(W).T
    if bias is not None:
        y = y + f64(bias)
    if res is not None:
        y = y + f64(res)
    return np.maximum(y, 0.0) if relu else y


def attention(q, k, v, heads):
    """q [N, Lq, D], k / v [N, Lk, D] -> [N, Lq, D]: softmax(q k^T hd^-1/2) v per head"""
    N, Lq, D = q.shape
    hd = D // heads
    split = lambda t: f64(t).reshape(N, -1, heads, hd).transpose(0, 2, 1, 3)
    qh, kh, vh = split(q), split(k), split(v)
    s = qh @ kh.transpose(0, 1, 3, 2) * hd ** -0.5
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=-1, keepdims=True)
    return (p @ vh).transpose(0, 2, 1, 3).reshape(N, Lq, D)


def layernorm(x, g, b, eps):
    x = f64(x)
    m = x.mean(axis=-1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * f64(g) + f64(b)


def upscale(x, w, bias, g=None, b=None, eps=1e-6, mode=1):
    """ConvTranspose2d(k 2, s 2) on channels-last x [N, Gi, Gi, Cin] with w [Cin, Cout, 2, 2] -> [N, 2 Gi, 2 Gi, Cout]; mode 1: LayerNorm2d over the
    channels then GELU, mode 2: GELU"""
    N, Gi, _, Cin = x.shape
    Co = w.shape[1]
    y = np.einsum('nijc,cokl->nikjlo', f64(x), f64(w)).reshape(N, 2 * Gi, 2 * Gi, Co) + f64(bias)
    if mode == 1:
        y = layernorm(y, g, b, eps)
    return gelu(y)


def feed_forward(sd, p, x):
    h = gemm(x, sd[p + '.proj_in.weight'], sd[p + '.proj_in.bias'], relu=True)
    h = gemm(h, sd[p + '.layers.0.weight'], sd[p + '.layers.0.bias'], relu=True)
    return gemm(h, sd[p + '.proj_out.weight'], sd[p + '.proj_out.bias'])


def token_mlps(sd, queries, Mt):
    """queries [N, T, C] -> (hyper_in [N, Mt, C/8], iou [N, Mt])"""
    hyper = np.stack([feed_forward(sd, f'mask_decoder.output_hypernetworks_mlps.{m}', queries[:, 1 + m]) for m in range(Mt)], axis=1)
    return hyper, feed_forward(sd, 'mask_decoder.iou_prediction_head', queries[:, 0])


def mask_product(hyper, up):
    """hyper [N, Mt, c], up [N, pixels, c] -> [N, Mt, pixels]"""
    return f64(hyper) @ f64(up).transpose(0, 2, 1)


def preprocess(image_u8, S, mean=PIXEL_MEAN, std=PIXEL_STD):
    h, w = image_u8.shape[:2]
    out = np.zeros((1, 3, S, S))
    out[0, :, :h, :w] = ((f64(image_u8) - f64(mean)) / f64(std)).transpose(2, 0, 1)
    return out


def _axis(n_out, n_in):
    """ATen's source index and weight, in ITS arithmetic: the scale, the index and the weight are fp32 (area_pixel_compute_source_index on `float`) -- at
    index 190 an fp32 rounding is 1.5e-5 of a pixel, so a float64 index would be another interpolation; the data stay float64"""
    f = np.float32
    scale = f(n_in) / f(n_out)
    src = np.maximum((np.arange(n_out, dtype=f) + f(0.5)) * scale - f(0.5), f(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), np.clip(src - i0.astype(f), f(0), f(1)).astype(np.float64)


def resize_bilinear(x, H, W):
    """[..., h, w] -> [..., H, W], F.interpolate(mode='bilinear', align_corners=False) as ATen states it"""
    y0, y1, ly = _axis(H, x.shape[-2])
    x0, x1, lx = _axis(W, x.shape[-1])
    x = f64(x)
    top = x[..., y0, :][..., x0] * (1 - lx) + x[..., y0, :][..., x1] * lx
    bot = x[..., y1, :][..., x0] * (1 - lx) + x[..., y1, :][..., x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def postprocess(low, S, h_in, w_in, H, W):
    return resize_bilinear(resize_bilinear(low, S, S)[..., :h_in, :w_in], H, W)


def attention_block(sd, p, q_in, k_in, v_in, heads, keep=None):
    lin = lambda n, x: gemm(x, sd[f'{p}.{n}.weight'], sd[f'{p}.{n}.bias'])
    q, k = lin('q_proj', q_in), lin('k_proj', k_in)
    if keep is not None:
        hd = q.shape[-1] // heads
        keep[p] = float(np.std((q.reshape(q.shape[0], -1, heads, hd).transpose(0, 2, 1, 3) @ k.reshape(k.shape[0], -1, heads, hd).transpose(0, 2, 3, 1)) * hd ** -0.5))
    return lin('out_proj', attention(q, k, lin('v_proj', v_in), heads))


def decoder_forward(sd, cfg, embedding, boxes=None, points=None, labels=None, keep=None):
    """sd: transformers names -> arrays; cfg: hidden_size, num_hidden_layers, num_attention_heads, num_multimask_outputs, layer_norm_eps,
    final_layer_norm_eps, image_embedding_size, image_size; embedding [B, C, G, G]; boxes [B, P, 4] | None; points [B, P, n, 2] | None, labels [B, P, n]
    -> {tap name: float64 array} with the names of SamMaskDecoderEngine.tap_names() plus low_res_masks [N, Mt, 4G, 4G] and iou [N, Mt] (all mask
    tokens).  keep: receives the standard deviation of every attention's logits."""
    sd = {k: f64(v) for k, v in sd.items()}
    C, L, heads, Mt, G = cfg['hidden_size'], cfg['num_hidden_layers'], cfg['num_attention_heads'], cfg['num_multimask_outputs'] + 1, cfg['image_embedding_size']
    eps, eps_f = cfg['layer_norm_eps'], cfg['final_layer_norm_eps']
    B = embedding.shape[0]
    P = (boxes if boxes is not None else points).shape[1]
    N = B * P
    flat = lambda t, *s: None if t is None else np.asarray(t).reshape(N, *s)
    n_pts = 0 if points is None else points.shape[2]
    taps = {}
    key_pe = taps['dense_pe'] = dense_pe(sd['shared_image_embedding.positional_embedding'], G)
    pe = taps['tokens'] = prompt_tokens(sd, flat(boxes, 4), flat(points, n_pts, 2), flat(labels, n_pts), cfg['image_size'])
    keys = src_rows(embedding, sd['prompt_encoder.no_mask_embed.weight'], P)
    queries = pe
    tf = 'mask_decoder.transformer.'
    norm = lambda p, x, e: layernorm(x, sd[p + '.weight'], sd[p + '.bias'], e)
    for k in range(L):
        b = f'{tf}layers.{k}.'
        if k == 0:
            queries = attention_block(sd, b + 'self_attn', queries, queries, queries, heads, keep)
        else:
            q = queries + pe
            queries = queries + attention_block(sd, b + 'self_attn', q, q, queries, heads, keep)
        queries = norm(b + 'layer_norm1', queries, eps)
        queries = norm(b + 'layer_norm2', queries + attention_block(sd, b + 'cross_attn_token_to_image', queries + pe, keys + key_pe, keys, heads, keep), eps)
        h = gemm(queries, sd[b + 'mlp.lin1.weight'], sd[b + 'mlp.lin1.bias'], relu=True)
        queries = norm(b + 'layer_norm3', gemm(h, sd[b + 'mlp.lin2.weight'], sd[b + 'mlp.lin2.bias'], res=queries), eps)
        keys = norm(b + 'layer_norm4', keys + attention_block(sd, b + 'cross_attn_image_to_token', keys + key_pe, queries + pe, queries, heads, keep), eps)
        taps[f'queries.{k}'], taps[f'keys.{k}'] = queries, keys
    queries = norm(tf + 'layer_norm_final_attn', queries + attention_block(sd, tf + 'final_attn_token_to_image', queries + pe, keys + key_pe, keys, heads, keep), eps_f)
    taps['queries.final'] = queries
    md = 'mask_decoder.'
    up = upscale(keys.reshape(N, G, G, C), sd[md + 'upscale_conv1.weight'], sd[md + 'upscale_conv1.bias'], sd[md + 'upscale_layer_norm.weight'],
                 sd[md + 'upscale_layer_norm.bias'], 1e-6, 1)
    up = upscale(up, sd[md + 'upscale_conv2.weight'], sd[md + 'upscale_conv2.bias'], mode=2).reshape(N, 16 * G * G, C // 8)
    taps['upscaled'] = up
    taps['hyper_in'], taps['iou'] = token_mlps(sd, queries, Mt)
    taps['low_res_masks'] = mask_product(taps['hyper_in'], up).reshape(N, Mt, 4 * G, 4 * G)
    return taps
