"""Golden for the SAM image encoder engine: transformers' own `SamVisionEncoder` (models/sam/modeling_sam.py -- the arithmetic of
segment_anything's `ImageEncoderViT`, which is not installed here) in float64 on the CPU with eager attention.

    python tests/golden/make_sam_encoder_golden.py        (needs `transformers`; writes tests/golden/sam_encoder_ref.npz)

  tests/golden/sam_encoder_ref.npz   per case: every hidden state ([B, G, G, C]: patch embedding + pos_embed, then the output of every block) and the
                                     neck output ([B, 256, G, G]), the rel-L2 of the 16-bit CPU modules (.half() / .bfloat16()) against float64 per
                                     hidden state and for the neck output (the engine's bar is 1.5 x these), the largest attention probability of
                                     block 0, and the sha256 of the case's weights and pixels

One committed file may not exceed 1 MiB, so the float64 references are STORED AS float32 (a relative 6e-8, four orders below the 16-bit errors
they are compared with), and a tensor of more than SAMPLE values is stored -- and its 16-bit errors are measured -- on a fixed pseudo-random
subset of SAMPLE flat positions (`sample_index`, regenerated from the case's seed by the readers).  Neither weights nor pixels are stored:
`make_weights(case)` / `make_pixels(case)` regenerate them from numpy's frozen `RandomState` stream and the readers check the sha256 recorded
here.  All of them are rounded to fp16-representable values.

transformers initialises `rel_pos_h`, `rel_pos_w` and `pos_embed` to ZERO: a golden made from a freshly initialised module would be blind to the
relative-position kernel.  Here the tables, pos_embed, every bias and every LayerNorm affine term are seeded to nonzero values.

Both cases use patch 16 and window 14 -- the production window, whose 196 keys are not a multiple of the kernel's key tile:

  case A   hidden 128 / 2 heads (head_dim 64), image 256 -> G = 16, padded to 28: 2 x 2 windows, three of them mostly padding; 3 blocks, block 1
           global (256 keys); B = 2
  case B   hidden 160 / 2 heads (head_dim 80), image 320 -> G = 20, padded to 28; 4 blocks, block 3 global (400 keys); B = 1

Hidden states are taken with forward hooks (the input of block 0 and the output of every block), so that the generator does not depend on how a
transformers release spells `output_hidden_states` for this model.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, 'sam_encoder_ref.npz')
SAMPLE = 8192

CASES = {
    'A': dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=3, image_size=256, global_attn_indexes=(1,), B=2, seed=3101),
    'B': dict(hidden_size=160, num_attention_heads=2, num_hidden_layers=4, image_size=320, global_attn_indexes=(3,), B=1, seed=3102),
}


def config_dict(case):
    c = CASES[case]
    return dict(hidden_size=c['hidden_size'], num_hidden_layers=c['num_hidden_layers'], num_attention_heads=c['num_attention_heads'], image_size=c['image_size'],
                patch_size=16, mlp_dim=4 * c['hidden_size'], window_size=14, global_attn_indexes=tuple(c['global_attn_indexes']), output_channels=256,
                layer_norm_eps=1e-6, hidden_act='gelu', qkv_bias=True, use_rel_pos=True, use_abs_pos=True, num_channels=3)


def grid(case):
    return CASES[case]['image_size'] // 16


def tensor_names(case):
    """hidden_states.0 .. hidden_states.<layers>, then `neck`"""
    return [f'hidden_states.{k}' for k in range(CASES[case]['num_hidden_layers'] + 1)] + ['neck']


def _fp16(a):
    return a.astype(np.float16).astype(np.float64)


def make_weights(case):
    """-> {transformers SamVisionEncoder state-dict name: float64 array of fp16-representable values}, from the frozen RandomState stream of the case's seed."""
    cfg, rs = config_dict(case), np.random.RandomState(CASES[case]['seed'])
    C, I, nl, P, O, G, w = cfg['hidden_size'], cfg['mlp_dim'], cfg['num_hidden_layers'], cfg['patch_size'], cfg['output_channels'], grid(case), cfg['window_size']
    hd = C // cfg['num_attention_heads']
    sd = {}

    def put(name, shape, std, mean=0.0):
        sd[name] = _fp16(mean + std * rs.standard_normal(shape))

    # the CLIP vision golden's scaling: a unit-variance image gives patch rows of 0.2, pos_embed 0.2, linear weights x 4 over transformers'
    # initialisation widths; biases and LayerNorm affine terms random.  The tables: q has entries of order 1, so a table of 0.3 / sqrt(hd) gives a
    # bias of order 0.3 per axis -- next to logits of order 1, large enough that a wrong index or a dropped term moves the output by percents.
    put('patch_embed.projection.weight', (C, 3, P, P), 0.2 * (3 * P * P) ** -0.5)
    put('patch_embed.projection.bias', (C,), 0.1)
    put('pos_embed', (1, G, G, C), 0.2)
    w_attn, w_fc1 = 4.0 * C ** -0.5 * (2 * nl) ** -0.5, 4.0 * (2 * C) ** -0.5
    for k in range(nl):
        b = f'layers.{k}.'
        n = G if k in cfg['global_attn_indexes'] else w
        for nm in ('layer_norm1', 'layer_norm2'):
            put(b + nm + '.weight', (C,), 0.1, 1.0)
            put(b + nm + '.bias', (C,), 0.1)
        put(b + 'attn.qkv.weight', (3 * C, C), w_attn)
        put(b + 'attn.qkv.bias', (3 * C,), 0.1)
        put(b + 'attn.rel_pos_h', (2 * n - 1, hd), 0.3 * hd ** -0.5)
        put(b + 'attn.rel_pos_w', (2 * n - 1, hd), 0.3 * hd ** -0.5)
        put(b + 'attn.proj.weight', (C, C), w_attn)
        put(b + 'attn.proj.bias', (C,), 0.1)
        put(b + 'mlp.lin1.weight', (I, C), w_fc1)
        put(b + 'mlp.lin1.bias', (I,), 0.1)
        put(b + 'mlp.lin2.weight', (C, I), w_attn)
        put(b + 'mlp.lin2.bias', (C,), 0.1)
    put('neck.conv1.weight', (O, C, 1, 1), C ** -0.5)
    put('neck.layer_norm1.weight', (O,), 0.1, 1.0)
    put('neck.layer_norm1.bias', (O,), 0.1)
    put('neck.conv2.weight', (O, O, 3, 3), (9 * O) ** -0.5)
    put('neck.layer_norm2.weight', (O,), 0.1, 1.0)
    put('neck.layer_norm2.bias', (O,), 0.1)
    return sd


def segment_anything_keys(sd):
    """The same tensors under segment_anything's `ImageEncoderViT` key layout (restated from its published source; the package is not installed)."""
    neck = {'neck.conv1.': 'neck.0.', 'neck.layer_norm1.': 'neck.1.', 'neck.conv2.': 'neck.2.', 'neck.layer_norm2.': 'neck.3.'}
    out = {}
    for k, v in sd.items():
        for a, b in neck.items():
            if k.startswith(a):
                k = b + k[len(a):]
        k = k.replace('patch_embed.projection.', 'patch_embed.proj.').replace('.layer_norm1.', '.norm1.').replace('.layer_norm2.', '.norm2.')
        if k.startswith('layers.'):
            k = 'blocks.' + k[len('layers.'):]
        out[k] = v
    return out


def make_pixels(case):
    """float64 [B, 3, S, S] of fp16-representable values: unit-variance noise over a per-image gradient (a normalised image's range)."""
    c = CASES[case]
    rs = np.random.RandomState(c['seed'] * 10)
    S = c['image_size']
    ramp = np.linspace(-1.0, 1.0, S)
    px = rs.standard_normal((c['B'], 3, S, S)) + 0.5 * ramp[None, None, :, None] * (1 + np.arange(c['B']))[:, None, None, None] - 0.5 * ramp[None, None, None, :]
    return _fp16(px)


def digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].astype(np.float16)).tobytes())
    return h.hexdigest()


def sample_index(case, name, n):
    """The flat positions of a tensor of n values that are stored: all of them up to SAMPLE, else SAMPLE sorted positions drawn without replacement
    from the case's seed and the tensor's number."""
    if n <= SAMPLE:
        return np.arange(n)
    rs = np.random.RandomState(CASES[case]['seed'] * 100 + tensor_names(case).index(name))
    return np.sort(rs.choice(n, SAMPLE, replace=False))


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def build_module(case, dtype):
    import torch
    from transformers import SamVisionConfig
    from transformers.models.sam.modeling_sam import SamVisionEncoder
    cfg = config_dict(case)
    cfg['global_attn_indexes'] = list(cfg['global_attn_indexes'])
    config = SamVisionConfig(**cfg)
    config._attn_implementation = 'eager'
    m = SamVisionEncoder(config)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in make_weights(case).items()}, strict=True)
    assert not missing and not unexpected
    return m.to(dtype).eval()


def run_module(m, pixels):
    """-> {name: float64 array}: every hidden state [B, G, G, C] and the neck output [B, O, G, G]"""
    import torch
    hs, hooks = [], []
    hooks.append(m.layers[0].register_forward_pre_hook(lambda mod, args: hs.append(args[0])))
    for layer in m.layers:
        hooks.append(layer.register_forward_hook(lambda mod, args, out: hs.append(out[0] if isinstance(out, tuple) else out)))
    with torch.no_grad():
        out = m(torch.from_numpy(pixels).to(next(m.parameters()).dtype)).last_hidden_state
    for h in hooks:
        h.remove()
    res = {f'hidden_states.{k}': h.double().numpy() for k, h in enumerate(hs)}
    res['neck'] = out.double().numpy()
    return res


def max_softmax_probability(case):
    """Largest attention probability of block 0, by the numpy rule (tests/sam_rule.py): the fixture must not have a flat softmax, or a wrong key
    range or bias index would not show."""
    sys.path.insert(0, os.path.dirname(HERE))
    import sam_rule as R
    sd, cfg = make_weights(case), config_dict(case)
    hs, _ = R.encoder_forward(sd, dict(cfg, num_hidden_layers=0), make_pixels(case))
    keep = {}
    R.block_forward({k: np.asarray(v, np.float64) for k, v in sd.items()}, cfg, 0, hs[0], keep)
    p = R.relpos_probabilities(keep['q'], keep['k'], keep['rel_h'], keep['rel_w'], keep['grid'], keep['grid'], keep['q'].shape[-1] ** -0.5)
    return float(p.max())


def generate(case):
    import torch
    out = {}
    pixels = make_pixels(case)
    out[f'{case}.weights_sha256'] = np.array(digest(make_weights(case)))
    out[f'{case}.pixels_sha256'] = np.array(digest({'pixel_values': pixels}))
    ref = run_module(build_module(case, torch.float64), pixels)
    assert sorted(ref) == sorted(tensor_names(case)), sorted(ref)
    pmax = max_softmax_probability(case)
    assert pmax > 0.2, (case, pmax, 'the softmax is too flat to tell a wrong key range')
    out[f'{case}.max_softmax_probability'] = np.array(pmax)
    idx = {n: sample_index(case, n, ref[n].size) for n in ref}
    for n in tensor_names(case):
        out[f'{case}.{n}'] = ref[n].reshape(-1)[idx[n]].astype(np.float32)
        out[f'{case}.{n}.shape'] = np.array(ref[n].shape)
    for tag, dtype in (('fp16', torch.float16), ('bf16', torch.bfloat16)):
        low = run_module(build_module(case, dtype), pixels)
        errs = {n: rel_l2(low[n].reshape(-1)[idx[n]], ref[n].reshape(-1)[idx[n]]) for n in tensor_names(case)}
        out[f'{case}.err_{tag}.hidden_states'] = np.array([errs[n] for n in tensor_names(case)[:-1]])
        out[f'{case}.err_{tag}.neck'] = np.array(errs['neck'])
        if tag == 'fp16':
            assert max(errs.values()) < 5e-3, (case, errs, 'the fixture is too hot to discriminate')
    # the bias is live in the reference: with both tables zeroed the neck output moves by far more than any 16-bit error
    m = build_module(case, torch.float64)
    with torch.no_grad():
        for layer in m.layers:
            layer.attn.rel_pos_h.zero_()
            layer.attn.rel_pos_w.zero_()
    out[f'{case}.neck_change_without_tables'] = np.array(rel_l2(run_module(m, pixels)['neck'], ref['neck']))
    assert float(out[f'{case}.neck_change_without_tables']) > 1e-2, (case, 'the tables barely move the output')
    return out


def main():
    out = {}
    for case in CASES:
        out.update(generate(case))
    np.savez_compressed(REF, **out)
    for k in sorted(out):
        if out[k].ndim == 0:
            print(f'{k:44s} {out[k]}')
        elif 'err_' in k:
            print(f'{k:44s} {np.array2string(out[k], precision=3)}')
    print(REF, os.path.getsize(REF), 'bytes')
    assert os.path.getsize(REF) < (1 << 20), 'a committed file may not exceed 1 MiB'


if __name__ == '__main__':
    sys.exit(main())
