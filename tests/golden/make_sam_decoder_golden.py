"""Golden for the SAM mask decoder engine: transformers' own `SamModel` pieces -- `prompt_encoder`, `mask_decoder` and
`get_image_wide_positional_embeddings` (models/sam/modeling_sam.py; the arithmetic of segment_anything's `PromptEncoder` / `MaskDecoder`, which is
not installed here) -- in float64 on the CPU (attention through torch's scaled_dot_product_attention: transformers' eager path takes its softmax
in float32 whatever the module's dtype).

    python tests/golden/make_sam_decoder_golden.py        (needs `transformers`; writes tests/golden/sam_decoder_ref.npz)

The decoder is at production widths (256, 8 heads, mlp 2048, 2 layers, 3 + 1 mask tokens); the vision tower of the `SamModel` is a one-block stub
that never runs.  Per case and tap the file holds the float64 reference STORED AS float32 (tensors above SAMPLE values on a seeded sample of SAMPLE
flat positions, `sample_index`), the rel-L2 of torch's fp32 CPU module against float64 on the same positions (`err_fp32.<tap>`: the engine's bar is 4 x
that, floor 2e-6), the standard deviation of every attention's logits, and the sha256 of weights and inputs, which `make_weights` / `make_inputs`
regenerate from numpy's frozen `RandomState` stream.  Weights are float32-representable, the image embedding fp16-representable (the engine reads
the encoder's 16-bit output).  Every bias, LayerNorm affine term, token and embedding is seeded to nonzero values.

  case A   G = 16 (S = 256), B = 2, P = 2, box only (T = 7), LayerNorm eps 1e-6 / 1e-5 (transformers' pair)
  case B   G = 12 (144 keys: no multiple of 64), B = 1, P = 2, box + 2 points (T = 9), eps 1e-5 / 1e-5 (segment_anything's pair)
  case C   G = 12, B = 1, P = 1, 3 points without a box (padding point, T = 9), one label 0, eps 1e-6 / 1e-5

`low_res_masks` / `iou` hold ALL mask tokens: the module is run with multimask_output=False (token 0) and True (tokens 1..3) and the two are joined.

Taps: dense_pe, tokens, queries.k / keys.k after each layer, queries.final, upscaled, hyper_in, low_res_masks, iou.

Conditioning (asserted here, on the CPU): with the image embedding perturbed by 1e-3 relative, float64 `low_res_masks` moves by at most 1e-2
relative, and torch's fp32 module sits within 1e-5 of float64 on it.  Weights are drawn at 1 / sqrt(fan_in) -- unit-variance rows in, unit-variance
rows out -- so that the attention logits q.k / sqrt(hd) are of order 1; QK_GAIN scales the q / k projections on top of that and is recorded, as are
the logit standard deviations that result.

Two weight variants per case that has the input they touch, each stored as its own float64 `low_res_masks` with its own fp32 error: `no_mask_zero`
(no_mask_embed zeroed) and `corner_swap` (point_embed.2 <-> point_embed.3; cases with a box).  The generator asserts that each moves the masks.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, 'sam_decoder_ref.npz')
SAMPLE = 8192
QK_GAIN = 1.0

CASES = {
    'A': dict(grid=16, B=2, P=2, box=True, n_points=0, layer_norm_eps=1e-6, final_layer_norm_eps=1e-5, seed=4101),
    'B': dict(grid=12, B=1, P=2, box=True, n_points=2, layer_norm_eps=1e-5, final_layer_norm_eps=1e-5, seed=4102),
    'C': dict(grid=12, B=1, P=1, box=False, n_points=3, layer_norm_eps=1e-6, final_layer_norm_eps=1e-5, seed=4103),
}
VARIANTS = ('no_mask_zero', 'corner_swap')


def config_dict(case):
    c = CASES[case]
    return dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=8, mlp_dim=2048, num_multimask_outputs=3, iou_head_depth=3, iou_head_hidden_dim=256,
                attention_downsample_rate=2, layer_norm_eps=c['layer_norm_eps'], final_layer_norm_eps=c['final_layer_norm_eps'], image_embedding_size=c['grid'],
                image_size=16 * c['grid'])


def tap_names(case):
    L = config_dict(case)['num_hidden_layers']
    return ['dense_pe', 'tokens'] + [f'{n}.{k}' for k in range(L) for n in ('queries', 'keys')] + ['queries.final', 'upscaled', 'hyper_in', 'low_res_masks', 'iou']


def variants(case):
    return [v for v in VARIANTS if v != 'corner_swap' or CASES[case]['box']]


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _f16(a):
    return a.astype(np.float16).astype(np.float64)


def make_weights(case, variant=None):
    """-> {transformers SamModel state-dict name: float64 array of float32-representable values} for the prompt encoder, the mask decoder and the shared
    positional embedding, from the frozen RandomState stream of the case's seed."""
    cfg, rs = config_dict(case), np.random.RandomState(CASES[case]['seed'])
    C, I, L, Mt = cfg['hidden_size'], cfg['mlp_dim'], cfg['num_hidden_layers'], cfg['num_multimask_outputs'] + 1
    sd = {}

    def put(name, shape, std, mean=0.0):
        sd[name] = _f32(mean + std * rs.standard_normal(shape))

    def linear(p, n_out, n_in, gain=1.0):
        put(p + '.weight', (n_out, n_in), gain * n_in ** -0.5)
        put(p + '.bias', (n_out,), 0.1)

    def norm(p, n):
        put(p + '.weight', (n,), 0.1, 1.0)
        put(p + '.bias', (n,), 0.1)

    def attn(p, inner):
        linear(p + '.q_proj', inner, C, QK_GAIN)
        linear(p + '.k_proj', inner, C, QK_GAIN)
        linear(p + '.v_proj', inner, C)
        linear(p + '.out_proj', C, inner)

    put('shared_image_embedding.positional_embedding', (2, C // 2), 1.0)          # SamVisionConfig.scale: segment_anything's default of 1.0
    for k in range(4):
        put(f'prompt_encoder.point_embed.{k}.weight', (1, C), 0.5)
    put('prompt_encoder.not_a_point_embed.weight', (1, C), 0.5)
    put('prompt_encoder.no_mask_embed.weight', (1, C), 0.5)
    put('mask_decoder.iou_token.weight', (1, C), 1.0)
    put('mask_decoder.mask_tokens.weight', (Mt, C), 1.0)
    tf = 'mask_decoder.transformer.'
    for k in range(L):
        b = f'{tf}layers.{k}.'
        attn(b + 'self_attn', C)
        norm(b + 'layer_norm1', C)
        attn(b + 'cross_attn_token_to_image', C // 2)
        norm(b + 'layer_norm2', C)
        linear(b + 'mlp.lin1', I, C)
        linear(b + 'mlp.lin2', C, I)
        norm(b + 'layer_norm3', C)
        norm(b + 'layer_norm4', C)
        attn(b + 'cross_attn_image_to_token', C // 2)
    attn(tf + 'final_attn_token_to_image', C // 2)
    norm(tf + 'layer_norm_final_attn', C)
    put('mask_decoder.upscale_conv1.weight', (C, C // 4, 2, 2), C ** -0.5)
    put('mask_decoder.upscale_conv1.bias', (C // 4,), 0.1)
    put('mask_decoder.upscale_conv2.weight', (C // 4, C // 8, 2, 2), (C // 4) ** -0.5)
    put('mask_decoder.upscale_conv2.bias', (C // 8,), 0.1)
    norm('mask_decoder.upscale_layer_norm', C // 4)
    for p, n_out in [(f'mask_decoder.output_hypernetworks_mlps.{m}', C // 8) for m in range(Mt)] + [('mask_decoder.iou_prediction_head', Mt)]:
        linear(p + '.proj_in', C, C, 2 ** 0.5)
        linear(p + '.layers.0', C, C, 2 ** 0.5)
        linear(p + '.proj_out', n_out, C, 2 ** 0.5)
    if variant == 'no_mask_zero':
        sd['prompt_encoder.no_mask_embed.weight'] = np.zeros((1, C))
    elif variant == 'corner_swap':
        a, b = 'prompt_encoder.point_embed.2.weight', 'prompt_encoder.point_embed.3.weight'
        sd[a], sd[b] = sd[b], sd[a]
    else:
        assert variant is None, variant
    return sd


def segment_anything_keys(sd):
    """The same tensors under segment_anything's `Sam` key layout (restated from its published source; the package is not installed)."""
    up = {'upscale_conv1.': 'output_upscaling.0.', 'upscale_layer_norm.': 'output_upscaling.1.', 'upscale_conv2.': 'output_upscaling.3.'}
    mlp = {'.proj_in.': '.layers.0.', '.layers.0.': '.layers.1.', '.proj_out.': '.layers.2.'}
    out = {}
    for k, v in sd.items():
        if k == 'shared_image_embedding.positional_embedding':
            k = 'prompt_encoder.pe_layer.positional_encoding_gaussian_matrix'
        k = k.replace('prompt_encoder.point_embed.', 'prompt_encoder.point_embeddings.').replace('.layer_norm_final_attn.', '.norm_final_attn.')
        for n in '1234':
            k = k.replace(f'.layer_norm{n}.', f'.norm{n}.')
        for a, b in up.items():
            k = k.replace('mask_decoder.' + a, 'mask_decoder.' + b)
        if 'mlps.' in k or 'iou_prediction_head' in k:
            for a, b in mlp.items():
                if a in k:
                    k = k.replace(a, b)
                    break
        out[k] = v
    return out


def make_inputs(case):
    """-> dict(embedding [B, 256, G, G] fp16-representable float64, boxes [B, P, 4] | None, points [B, P, n, 2] | None, labels [B, P, n] int64 | None); prompt
    coordinates in input-image pixels, multiples of 1 / 4"""
    c = CASES[case]
    rs = np.random.RandomState(c['seed'] * 10)
    G, S, B, P, n = c['grid'], 16 * c['grid'], c['B'], c['P'], c['n_points']
    ramp = np.linspace(-1.0, 1.0, G)
    emb = rs.standard_normal((B, 256, G, G)) + 0.5 * ramp[None, None, :, None] * (1 + np.arange(B))[:, None, None, None] - 0.5 * ramp[None, None, None, :]
    out = dict(embedding=_f16(emb), boxes=None, points=None, labels=None)
    if c['box']:
        lo = np.round(rs.uniform(0.05, 0.45, (B, P, 2)) * S * 4) / 4
        hi = np.round(rs.uniform(0.55, 0.95, (B, P, 2)) * S * 4) / 4
        out['boxes'] = np.concatenate([lo, hi], axis=-1)
    if n:
        out['points'] = np.round(rs.uniform(0.1, 0.9, (B, P, n, 2)) * S * 4) / 4
        labels = np.ones((B, P, n), np.int64)
        labels[..., 0] = 0
        out['labels'] = labels
    return out


def digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        if sd[k] is None:
            continue
        h.update(k.encode())
        h.update(np.ascontiguousarray(np.asarray(sd[k], np.float32)).tobytes())
    return h.hexdigest()


def sample_index(case, name, n):
    """The flat positions of a tensor of n values that are stored: all of them up to SAMPLE, else SAMPLE sorted positions drawn without replacement from the
    case's seed and the tap's number."""
    if n <= SAMPLE:
        return np.arange(n)
    rs = np.random.RandomState(CASES[case]['seed'] * 100 + tap_names(case).index(name))
    return np.sort(rs.choice(n, SAMPLE, replace=False))


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def build_module(case, dtype, variant=None):
    import torch
    from transformers import SamConfig, SamMaskDecoderConfig, SamModel, SamPromptEncoderConfig, SamVisionConfig
    cfg = config_dict(case)
    S, G = cfg['image_size'], cfg['image_embedding_size']
    vision = SamVisionConfig(hidden_size=32, output_channels=256, num_hidden_layers=1, num_attention_heads=2, image_size=S, patch_size=16, mlp_dim=32,
                             global_attn_indexes=[0], window_size=0, num_pos_feats=128, scale=1.0)
    prompt = SamPromptEncoderConfig(hidden_size=256, image_size=S, patch_size=16, num_point_embeddings=4)
    decoder = SamMaskDecoderConfig(hidden_size=256, mlp_dim=cfg['mlp_dim'], num_hidden_layers=cfg['num_hidden_layers'], num_attention_heads=cfg['num_attention_heads'],
                                   attention_downsample_rate=2, num_multimask_outputs=cfg['num_multimask_outputs'], iou_head_depth=3, iou_head_hidden_dim=256,
                                   layer_norm_eps=cfg['layer_norm_eps'])
    config = SamConfig(vision_config=vision, prompt_encoder_config=prompt, mask_decoder_config=decoder)
    # NOT 'eager': transformers' eager attention takes its softmax in float32 whatever the module's dtype, which would leave a 6e-8 error in the
    # "float64" reference.  torch's scaled_dot_product_attention computes in the dtype it is given.
    for c in (config, config.vision_config, config.prompt_encoder_config, config.mask_decoder_config):
        c._attn_implementation = 'sdpa'
    m = SamModel(config)
    assert m.prompt_encoder.image_embedding_size[0] == G
    m.mask_decoder.transformer.layer_norm_final_attn.eps = cfg['final_layer_norm_eps']
    sd = {k: torch.from_numpy(v) for k, v in make_weights(case, variant).items()}
    sd['prompt_encoder.shared_embedding.positional_embedding'] = sd['shared_image_embedding.positional_embedding']      # transformers' tied copy
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith(('vision_encoder.', 'prompt_encoder.mask_embed.')) for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


def run_module(m, inputs):
    """-> {tap: float64 array}, laid out as the engine's taps (channels last)"""
    import torch
    dt = next(m.parameters()).dtype
    t = lambda a, d=None: None if a is None else torch.from_numpy(np.asarray(a)).to(d or dt)
    emb, boxes, points, labels = t(inputs['embedding']), t(inputs['boxes']), t(inputs['points']), t(inputs['labels'], torch.int64)
    B, C, G = emb.shape[0], emb.shape[1], emb.shape[2]
    md = m.mask_decoder
    layers, finals, acts, hyper, iou = [], [], [], {}, []
    hooks = [layer.register_forward_hook(lambda mod, a, out: layers.append((out[0], out[1]))) for layer in md.transformer.layers]
    hooks.append(md.transformer.register_forward_hook(lambda mod, a, out: finals.append(out[0])))
    hooks.append(md.activation.register_forward_hook(lambda mod, a, out: acts.append(out)))
    for i, mlp in enumerate(md.output_hypernetworks_mlps):
        hooks.append(mlp.register_forward_hook(lambda mod, a, out, i=i: hyper.__setitem__(i, out)))
    hooks.append(md.iou_prediction_head.register_forward_hook(lambda mod, a, out: iou.append(out)))
    res = {}
    with torch.no_grad():
        pe = m.get_image_wide_positional_embeddings()
        res['dense_pe'] = pe[0].permute(1, 2, 0).reshape(G * G, C)
        sparse, dense = m.prompt_encoder(points, labels, boxes, None)
        P = sparse.shape[1]
        N = B * P
        out_tokens = torch.cat([md.iou_token.weight, md.mask_tokens.weight], dim=0)
        res['tokens'] = torch.cat([out_tokens.expand(B, P, -1, -1), sparse], dim=2).reshape(N, -1, C)
        masks = {}
        for multi in (False, True):
            del layers[:], finals[:], acts[:], iou[:]
            masks[multi], _ = md(image_embeddings=emb, image_positional_embeddings=pe.repeat(B, 1, 1, 1), sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense,
                                 multimask_output=multi)
    for h in hooks:
        h.remove()
    for k, (q, kk) in enumerate(layers):
        res[f'queries.{k}'], res[f'keys.{k}'] = q.reshape(N, -1, C), kk.reshape(N, G * G, C)
    res['queries.final'] = finals[0].reshape(N, -1, C)
    res['upscaled'] = acts[-1].permute(0, 2, 3, 1).reshape(N, 16 * G * G, C // 8)
    res['hyper_in'] = torch.stack([hyper[i] for i in range(len(hyper))], dim=2).reshape(N, len(hyper), C // 8)
    res['low_res_masks'] = torch.cat([masks[False], masks[True]], dim=2).reshape(N, -1, 4 * G, 4 * G)
    res['iou'] = iou[0].reshape(N, -1)
    return {k: v.double().numpy() for k, v in res.items()}


def logit_stds(case):
    """Standard deviation of the logits of every attention, by the numpy rule (tests/sam_decoder_rule.py)"""
    sys.path.insert(0, os.path.dirname(HERE))
    import sam_decoder_rule as R
    keep, inp = {}, make_inputs(case)
    R.decoder_forward(make_weights(case), config_dict(case), inp['embedding'], inp['boxes'], inp['points'], inp['labels'], keep)
    return keep


def generate(case):
    import torch
    out, inp = {}, make_inputs(case)
    out[f'{case}.weights_sha256'] = np.array(digest(make_weights(case)))
    out[f'{case}.inputs_sha256'] = np.array(digest(inp))
    m64, m32 = build_module(case, torch.float64), build_module(case, torch.float32)
    ref, low = run_module(m64, inp), run_module(m32, inp)
    assert sorted(ref) == sorted(tap_names(case)), sorted(ref)
    for n in tap_names(case):
        idx = sample_index(case, n, ref[n].size)
        out[f'{case}.{n}'] = ref[n].reshape(-1)[idx].astype(np.float32)
        out[f'{case}.{n}.shape'] = np.array(ref[n].shape)
        out[f'{case}.err_fp32.{n}'] = np.array(rel_l2(low[n].reshape(-1)[idx], ref[n].reshape(-1)[idx]))
    # attention logits of order 1
    stds = logit_stds(case)
    out[f'{case}.qk_gain'] = np.array(QK_GAIN)
    out[f'{case}.logit_std'] = np.array([stds[k] for k in sorted(stds)])
    out[f'{case}.logit_std.names'] = np.array(sorted(stds))
    assert 0.2 < min(stds.values()) and max(stds.values()) < 5.0, (case, stds, 'attention logits are not of order 1')
    # conditioning
    rs = np.random.RandomState(CASES[case]['seed'] * 1000)
    emb = inp['embedding']
    pert = dict(inp, embedding=emb + 1e-3 * np.linalg.norm(emb) / np.sqrt(emb.size) * rs.standard_normal(emb.shape))
    moved = rel_l2(run_module(m64, pert)['low_res_masks'], ref['low_res_masks'])
    fp32 = rel_l2(low['low_res_masks'], ref['low_res_masks'])
    out[f'{case}.conditioning.moved_by_1e-3'] = np.array(moved)
    out[f'{case}.conditioning.fp32_module'] = np.array(fp32)
    assert moved <= 1e-2, (case, moved, 'a 1e-3 perturbation of the embedding moves the masks by more than 1e-2')
    assert fp32 <= 1e-5, (case, fp32, "torch's fp32 module is further than 1e-5 from float64 on the masks")
    # weight variants
    idx = sample_index(case, 'low_res_masks', ref['low_res_masks'].size)
    for v in variants(case):
        r64 = run_module(build_module(case, torch.float64, v), inp)['low_res_masks']
        r32 = run_module(build_module(case, torch.float32, v), inp)['low_res_masks']
        out[f'{case}.{v}.low_res_masks'] = r64.reshape(-1)[idx].astype(np.float32)
        out[f'{case}.{v}.err_fp32'] = np.array(rel_l2(r32.reshape(-1)[idx], r64.reshape(-1)[idx]))
        out[f'{case}.{v}.change'] = np.array(rel_l2(r64, ref['low_res_masks']))
        assert float(out[f'{case}.{v}.change']) > 1e-3, (case, v, 'the variant does not move the masks')
    return out


def main():
    out = {}
    for case in CASES:
        out.update(generate(case))
    np.savez_compressed(REF, **out)
    for k in sorted(out):
        if out[k].ndim == 0:
            print(f'{k:44s} {out[k]}')
        elif 'logit_std' in k and 'names' not in k:
            print(f'{k:44s} {np.array2string(out[k], precision=3)}')
    print(REF, os.path.getsize(REF), 'bytes')
    assert os.path.getsize(REF) < (1 << 20), 'a committed file may not exceed 1 MiB'


if __name__ == '__main__':
    sys.exit(main())
