"""Golden for the CLIP vision engine and the IP-Adapter image projection engines: transformers' own `CLIPVisionModelWithProjection` /
`CLIPVisionModel` and the reference's `Resampler` / `ImageProjModel`, all in float64 on the CPU.

    python tests/golden/make_clip_vision_golden.py --reference <root of the reference tree>     (needs `transformers`; writes the two files below)

  tests/golden/clip_vision_ref.npz          the outputs the engines are held to (image_embeds, last_hidden_state, hidden_states[-2], pooler_output;
                                            the Resampler's and the ImageProjModel's tokens), the rel-L2 of the 16-bit CPU modules (.half() /
                                            .bfloat16()) against float64 per output and per hidden state (the engines' bar is 1.5 x these), and
                                            the sha256 of every case's weights and pixels
  tests/golden/clip_vision_hidden_ref.npz   the other entries of hidden_states (a fault is located by layer); hidden_states[-1] is
                                            last_hidden_state itself (transformers applies post_layernorm to the pooled row only)

Two files because one committed file may not exceed 1 MiB.  For the same reason the float64 references are STORED AS float32 (a relative 6e-8,
four orders below the 16-bit errors they are compared with; every recorded error was measured against the float64 values before the cast), and
neither weights nor pixels are stored: `make_weights(case)` / `make_pixels(case)` regenerate them from numpy's frozen `RandomState` stream and
the readers check the sha256 recorded here.  All of them are rounded to fp16-representable values: a 16-bit engine that loads them starts from
exactly the numbers the float64 reference used (fp16), and from their one rounding (bf16).

  case A   CLIPVisionModelWithProjection, quick_gelu, hidden 128 / 2 heads (head_dim 64), 2 layers, image 112 / patch 14 -> 65 tokens (one past a
           64-key tile), projection 64, B = 3
  case B   CLIPVisionModelWithProjection, gelu, hidden 160 / 2 heads (head_dim 80), 3 layers, image 224 / patch 14 -> 257 tokens (the real
           length), projection 96, B = 1
  case C   CLIPVisionModel (plain: pooler_output, no image_embeds), quick_gelu, hidden 128 / 2 heads, 2 layers, image 32 / patch 16 -> 5 tokens,
           B = 2; K = 3 * 16 * 16 = 768 needs no padding (the patchify kernel's vector branch)

  R        the reference's Resampler (dim 128, depth 2, dim_head 64, heads 2, 16 queries, embedding_dim 160, output_dim 192, ff_mult 4), fed case
           B's hidden_states[-2] as stored (float32) [1, 257, 160]
  P        the reference's ImageProjModel (64 -> 4 x 192), fed case A's image_embeds as stored [3, 64]

The reference tree is read at generation time only (resampler.py is loaded by path -- it imports torch and math alone; ImageProjModel is cut out
of ip_adapter.py with `ast`, since that file imports packages that need not be installed).  No test reads it: they read the npz files.
"""
import argparse
import ast
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, 'clip_vision_ref.npz')
HIDDEN_REF = os.path.join(HERE, 'clip_vision_hidden_ref.npz')

CASES = {
    'A': dict(with_projection=True, hidden_act='quick_gelu', hidden_size=128, num_attention_heads=2, num_hidden_layers=2, image_size=112, patch_size=14,
              projection_dim=64, B=3, seed=2701),
    'B': dict(with_projection=True, hidden_act='gelu', hidden_size=160, num_attention_heads=2, num_hidden_layers=3, image_size=224, patch_size=14,
              projection_dim=96, B=1, seed=2702),
    'C': dict(with_projection=False, hidden_act='quick_gelu', hidden_size=128, num_attention_heads=2, num_hidden_layers=2, image_size=32, patch_size=16,
              projection_dim=64, B=2, seed=2703),
}
OUTPUTS = ('image_embeds', 'last_hidden_state', 'penultimate', 'pooler_output')
RESAMPLER = dict(dim=128, depth=2, dim_head=64, heads=2, num_queries=16, embedding_dim=160, output_dim=192, ff_mult=4)
IMAGE_PROJ = dict(cross_attention_dim=192, clip_embeddings_dim=64, clip_extra_context_tokens=4)
RESAMPLER_SEED, IMAGE_PROJ_SEED = 2711, 2712


def config_dict(case):
    c = CASES[case]
    return dict(hidden_size=c['hidden_size'], intermediate_size=4 * c['hidden_size'], num_hidden_layers=c['num_hidden_layers'],
                num_attention_heads=c['num_attention_heads'], image_size=c['image_size'], patch_size=c['patch_size'], hidden_act=c['hidden_act'],
                layer_norm_eps=1e-5, projection_dim=c['projection_dim'], num_channels=3)


def n_tokens(case):
    return (CASES[case]['image_size'] // CASES[case]['patch_size']) ** 2 + 1


def _fp16(a):
    return a.astype(np.float16).astype(np.float64)


def make_weights(case):
    """-> {transformers state-dict name: float64 array of fp16-representable values}, from the frozen RandomState stream of the case's seed."""
    cfg, rs = config_dict(case), np.random.RandomState(CASES[case]['seed'])
    C, I, nl, P = cfg['hidden_size'], cfg['intermediate_size'], cfg['num_hidden_layers'], cfg['patch_size']
    sd = {}

    def put(name, shape, std, mean=0.0):
        sd[name] = _fp16(mean + std * rs.standard_normal(shape))

    # the text golden's scaling: embeddings 0.2 (the patch weight so that a unit-variance image gives patch rows of 0.2 too), linear weights x 4
    # over transformers' initialisation widths; biases and LayerNorm affine parameters random, so that no fused bias path hides behind zeros
    em = 'vision_model.embeddings.'
    put(em + 'class_embedding', (C,), 0.2)
    put(em + 'patch_embedding.weight', (C, 3, P, P), 0.2 * (3 * P * P) ** -0.5)
    put(em + 'position_embedding.weight', (n_tokens(case), C), 0.2)
    put('vision_model.pre_layrnorm.weight', (C,), 0.1, 1.0)
    put('vision_model.pre_layrnorm.bias', (C,), 0.1)
    w_attn, w_fc1 = 4.0 * C ** -0.5 * (2 * nl) ** -0.5, 4.0 * (2 * C) ** -0.5
    for k in range(nl):
        b = f'vision_model.encoder.layers.{k}.'
        for n in ('layer_norm1', 'layer_norm2'):
            put(b + n + '.weight', (C,), 0.1, 1.0)
            put(b + n + '.bias', (C,), 0.1)
        for n in ('q_proj', 'k_proj', 'v_proj', 'out_proj'):
            put(b + 'self_attn.' + n + '.weight', (C, C), w_attn)
            put(b + 'self_attn.' + n + '.bias', (C,), 0.1)
        put(b + 'mlp.fc1.weight', (I, C), w_fc1)
        put(b + 'mlp.fc1.bias', (I,), 0.1)
        put(b + 'mlp.fc2.weight', (C, I), w_attn)
        put(b + 'mlp.fc2.bias', (C,), 0.1)
    put('vision_model.post_layernorm.weight', (C,), 0.1, 1.0)
    put('vision_model.post_layernorm.bias', (C,), 0.1)
    if CASES[case]['with_projection']:
        put('visual_projection.weight', (cfg['projection_dim'], C), 4.0 * C ** -0.5)
    return sd


def make_pixels(case):
    """float64 [B, 3, S, S] of fp16-representable values: unit-variance noise over a per-image gradient (a normalised image's range)."""
    c = CASES[case]
    rs = np.random.RandomState(c['seed'] * 10)
    S = c['image_size']
    ramp = np.linspace(-1.0, 1.0, S)
    px = rs.standard_normal((c['B'], 3, S, S)) + 0.5 * ramp[None, None, :, None] * (1 + np.arange(c['B']))[:, None, None, None] - 0.5 * ramp[None, None, None, :]
    return _fp16(px)


def make_resampler_weights():
    r, rs = RESAMPLER, np.random.RandomState(RESAMPLER_SEED)
    D, inner, F, E, O, Q = r['dim'], r['heads'] * r['dim_head'], r['dim'] * r['ff_mult'], r['embedding_dim'], r['output_dim'], r['num_queries']
    sd = {}

    def put(name, shape, std, mean=0.0):
        sd[name] = _fp16(mean + std * rs.standard_normal(shape))

    # q and k at twice the unit scale so that the softmax is not flat; to_out and the last feed-forward weight at half scale (the residual stream
    # stays within a few units and the reference's own fp16 module stays under the 5e-3 the generator asserts)
    put('latents', (1, Q, D), D ** -0.5)
    put('proj_in.weight', (D, E), E ** -0.5)
    put('proj_in.bias', (D,), 0.1)
    for k in range(r['depth']):
        a, f = f'layers.{k}.0.', f'layers.{k}.1.'
        for n in ('norm1', 'norm2'):
            put(a + n + '.weight', (D,), 0.1, 1.0)
            put(a + n + '.bias', (D,), 0.1)
        put(a + 'to_q.weight', (inner, D), 2.0 * D ** -0.5)
        put(a + 'to_kv.weight', (2 * inner, D), 2.0 * D ** -0.5)
        put(a + 'to_out.weight', (D, inner), 0.5 * inner ** -0.5)
        put(f + '0.weight', (D,), 0.1, 1.0)
        put(f + '0.bias', (D,), 0.1)
        put(f + '1.weight', (F, D), D ** -0.5)
        put(f + '3.weight', (D, F), 0.5 * F ** -0.5)
    put('proj_out.weight', (O, D), D ** -0.5)
    put('proj_out.bias', (O,), 0.1)
    put('norm_out.weight', (O,), 0.1, 1.0)
    put('norm_out.bias', (O,), 0.1)
    return sd


def make_image_proj_weights():
    p, rs = IMAGE_PROJ, np.random.RandomState(IMAGE_PROJ_SEED)
    N, K, D = p['clip_extra_context_tokens'] * p['cross_attention_dim'], p['clip_embeddings_dim'], p['cross_attention_dim']
    return {'proj.weight': _fp16(K ** -0.5 * rs.standard_normal((N, K))), 'proj.bias': _fp16(0.1 * rs.standard_normal((N,))),
            'norm.weight': _fp16(1.0 + 0.1 * rs.standard_normal((D,))), 'norm.bias': _fp16(0.1 * rs.standard_normal((D,)))}


def digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].astype(np.float16)).tobytes())
    return h.hexdigest()


def build_module(case, dtype):
    import torch
    from transformers import CLIPVisionConfig, CLIPVisionModel, CLIPVisionModelWithProjection
    cfg = CLIPVisionConfig(**config_dict(case))
    m = (CLIPVisionModelWithProjection if CASES[case]['with_projection'] else CLIPVisionModel)(cfg)
    sd = {k: torch.from_numpy(v) for k, v in make_weights(case).items()}
    if not any(k.startswith('vision_model.') for k in m.state_dict()):      # a transformers whose plain CLIPVisionModel holds embeddings / encoder itself
        sd = {k[len('vision_model.'):]: v for k, v in sd.items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith('position_ids') for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


def run_module(m, pixels, with_projection):
    import torch
    with torch.no_grad():
        px = torch.from_numpy(pixels).to(next(m.parameters()).dtype)
        out = m(pixel_values=px, output_hidden_states=True)
        # CLIPVisionModelOutput has no pooler_output: the normalised class row is what visual_projection consumed
        pooled = m.vision_model(pixel_values=px).pooler_output if with_projection else out.pooler_output
    hs = [h.double().numpy() for h in out.hidden_states]
    res = dict(last_hidden_state=out.last_hidden_state.double().numpy(), penultimate=hs[-2], hidden_states=hs, pooler_output=pooled.double().numpy())
    if with_projection:
        res['image_embeds'] = out.image_embeds.double().numpy()
    return res


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def max_softmax_probability(case, hidden0):
    """Largest attention probability of layer 0: the fixture must not have a flat softmax, or a wrong key range would not show."""
    sd, cfg = make_weights(case), config_dict(case)
    C, H = cfg['hidden_size'], cfg['num_attention_heads']
    b = 'vision_model.encoder.layers.0.'
    x = hidden0
    mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
    n = (x - mu) / np.sqrt(var + cfg['layer_norm_eps']) * sd[b + 'layer_norm1.weight'] + sd[b + 'layer_norm1.bias']
    q = n @ sd[b + 'self_attn.q_proj.weight'].T + sd[b + 'self_attn.q_proj.bias']
    k = n @ sd[b + 'self_attn.k_proj.weight'].T + sd[b + 'self_attn.k_proj.bias']
    B, L, _ = x.shape
    q, k = q.reshape(B, L, H, C // H).transpose(0, 2, 1, 3), k.reshape(B, L, H, C // H).transpose(0, 2, 1, 3)
    s = q @ k.transpose(0, 1, 3, 2) * (C // H) ** -0.5
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return float(p.max())


def generate(case):
    """-> (headline dict, hidden dict) of arrays for one case; float64 references are cast to float32 for storage."""
    import torch
    wp = CASES[case]['with_projection']
    head, hidden = {}, {}
    pixels = make_pixels(case)
    head[f'{case}.weights_sha256'] = np.array(digest(make_weights(case)))
    head[f'{case}.pixels_sha256'] = np.array(digest({'pixel_values': pixels}))
    ref = run_module(build_module(case, torch.float64), pixels, wp)
    key = f'{case}.'
    assert np.array_equal(ref['last_hidden_state'], ref['hidden_states'][-1]), 'last_hidden_state is expected to be hidden_states[-1] (no post norm)'
    pmax = max_softmax_probability(case, ref['hidden_states'][0])
    assert pmax > 0.2, (case, pmax, 'the softmax is too flat to tell a wrong key range')
    head[key + 'max_softmax_probability'] = np.array(pmax)
    head[key + 'penultimate_absmax'] = np.array(np.abs(ref['penultimate']).max())
    for o in OUTPUTS:
        if o in ref:
            head[key + o] = ref[o].astype(np.float32)
    n = len(ref['hidden_states'])
    for k, h in enumerate(ref['hidden_states']):
        if k < n - 2:                              # hidden_states[-2] is `penultimate`, hidden_states[-1] is `last_hidden_state` of the first file
            hidden[key + f'hidden_states.{k}'] = h.astype(np.float32)
    for tag, dtype in (('fp16', torch.float16), ('bf16', torch.bfloat16)):
        low = run_module(build_module(case, dtype), pixels, wp)
        for o in OUTPUTS:
            if o in ref:
                err = rel_l2(low[o], ref[o])
                head[key + f'err_{tag}.' + o] = np.array(err)
                if tag == 'fp16':
                    assert err < 5e-3, (case, o, err, 'the fixture is too hot to discriminate')
        head[key + f'err_{tag}.hidden_states'] = np.array([rel_l2(a, b) for a, b in zip(low['hidden_states'], ref['hidden_states'])])
    return head, hidden


def load_reference_modules(root):
    """-> (Resampler, ImageProjModel) classes of the reference tree at `root`, without importing its packages."""
    import torch
    d = os.path.join(root, 'lib', 'models', 'architecture', 'ip_adapter')
    spec = importlib.util.spec_from_file_location('_reference_resampler', os.path.join(d, 'resampler.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(d, 'ip_adapter.py')) as fh:
        tree = ast.parse(fh.read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'ImageProjModel']
    assert len(cls) == 1, 'ImageProjModel not found in the reference ip_adapter.py'
    ns = {'torch': torch}
    exec(compile(ast.Module(body=cls, type_ignores=[]), 'ip_adapter.py::ImageProjModel', 'exec'), ns)
    return mod.Resampler, ns['ImageProjModel']


def generate_image_proj(root, head):
    """The Resampler on case B's stored hidden_states[-2] and the ImageProjModel on case A's stored image_embeds."""
    import torch
    Resampler, ImageProjModel = load_reference_modules(root)
    out = {}
    for tag, cls, kw, sd, x in (('R', Resampler, RESAMPLER, make_resampler_weights(), head['B.penultimate']),
                                ('P', ImageProjModel, IMAGE_PROJ, make_image_proj_weights(), head['A.image_embeds'])):
        assert x.dtype == np.float32
        out[f'{tag}.weights_sha256'] = np.array(digest(sd))

        def module(dtype):
            m = cls(**kw)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            return m.to(dtype).eval()
        with torch.no_grad():
            ref = module(torch.float64)(torch.from_numpy(x).double()).numpy()
            out[f'{tag}.tokens'] = ref.astype(np.float32)
            for name, dtype in (('fp16', torch.float16), ('bf16', torch.bfloat16)):
                err = rel_l2(module(dtype)(torch.from_numpy(x).to(dtype)).double().numpy(), ref)
                out[f'{tag}.err_{name}.tokens'] = np.array(err)
                if name == 'fp16':
                    assert err < 5e-3, (tag, err, 'the fixture is too hot to discriminate')
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='root of the reference tree (read for resampler.py and ImageProjModel only)')
    args = ap.parse_args()
    head, hidden = {}, {}
    for case in CASES:
        h, hh = generate(case)
        head.update(h)
        hidden.update(hh)
    head.update(generate_image_proj(args.reference, head))
    np.savez_compressed(REF, **head)
    np.savez_compressed(HIDDEN_REF, **hidden)
    for k in sorted(head):
        if head[k].ndim == 0:
            print(f'{k:44s} {head[k]}')
        elif 'err_' in k:
            print(f'{k:44s} {np.array2string(head[k], precision=3)}')
    for p in (REF, HIDDEN_REF):
        print(p, os.path.getsize(p), 'bytes')
        assert os.path.getsize(p) < (1 << 20), 'a committed file may not exceed 1 MiB'


if __name__ == '__main__':
    sys.exit(main())
