"""One timing of the native CLIP vision tower and the IP-Adapter Resampler behind it, with no target: the full-size ViT-H/14 tower (1280 wide,
32 layers, 16 heads of 80, MLP 5120, gelu, 224 / 14 -> 257 tokens, projection 1024) with seeded synthetic fp16 weights at B = 2, and the 4-layer
Resampler of the SD 1.5 "plus" checkpoints (dim 768, 12 heads of 64, 16 queries, embedding_dim 1280, output_dim 768) fed the tower's
hidden_states[-2].  Device events around windows of at least half a second after a warm-up, three windows, the median reported; the launch
count and the per-class time come from the plan (`mve_unet_op_info`) and one profiled forward.  Where `transformers` imports, its own
half-precision CLIPVisionModelWithProjection with the same weights is timed in the same process, the windows alternating with the engine's;
otherwise the file says "not measured".  The reference's torch Resampler is not part of this repository and is not timed.  Both run once per
request, not once per denoising step.  Measured once, untuned.

    python tools/clip_vision_report.py [--out profiles/clip_vision.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvedit_amd.ip_adapter import ResamplerEngine  # noqa: E402
from mvedit_amd.vision_encoder import CLIPVisionEngine, VIT_H_14_VISION_CONFIG  # noqa: E402
from tools.clip_text_report import windows  # noqa: E402

RESAMPLER = dict(dim=768, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280, output_dim=768, ff_mult=4)
COPIES = ('hidden state -> output', 'last_hidden_state -> output', 'latents.repeat')


def synthetic_state_dict(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    C, I, nl, P = cfg['hidden_size'], cfg['intermediate_size'], cfg['num_hidden_layers'], cfg['patch_size']
    T = (cfg['image_size'] // P) ** 2 + 1
    sd = {}

    def put(name, shape, std, mean=0.0):
        sd[name] = (mean + std * torch.randn(*shape, generator=g)).half()
    em = 'vision_model.embeddings.'
    put(em + 'class_embedding', (C,), 0.02)
    put(em + 'patch_embedding.weight', (C, 3, P, P), 0.02)
    put(em + 'position_embedding.weight', (T, C), 0.02)
    put('vision_model.pre_layrnorm.weight', (C,), 0.02, 1.0)
    put('vision_model.pre_layrnorm.bias', (C,), 0.02)
    w = C ** -0.5 * (2 * nl) ** -0.5
    for k in range(nl):
        b = f'vision_model.encoder.layers.{k}.'
        for n in ('layer_norm1', 'layer_norm2'):
            put(b + n + '.weight', (C,), 0.02, 1.0)
            put(b + n + '.bias', (C,), 0.02)
        for n in ('q_proj', 'k_proj', 'v_proj', 'out_proj'):
            put(b + 'self_attn.' + n + '.weight', (C, C), w)
            put(b + 'self_attn.' + n + '.bias', (C,), 0.02)
        put(b + 'mlp.fc1.weight', (I, C), (2 * C) ** -0.5)
        put(b + 'mlp.fc1.bias', (I,), 0.02)
        put(b + 'mlp.fc2.weight', (C, I), w)
        put(b + 'mlp.fc2.bias', (C,), 0.02)
    put('vision_model.post_layernorm.weight', (C,), 0.02, 1.0)
    put('vision_model.post_layernorm.bias', (C,), 0.02)
    put('visual_projection.weight', (cfg['projection_dim'], C), C ** -0.5)
    return sd


def synthetic_resampler_state_dict(eng, seed=1):
    g = torch.Generator().manual_seed(seed)
    D, inner, F, E, O, Q = eng.dim, eng.heads * 64, eng.dim * eng.ff_mult, eng.embedding_dim, eng.output_dim, eng.num_queries
    shapes = {'latents': (1, Q, D), 'proj_in.weight': (D, E), 'proj_in.bias': (D,), 'proj_out.weight': (O, D), 'proj_out.bias': (O,), 'norm_out.weight': (O,),
              'norm_out.bias': (O,)}
    for k in range(eng.depth):
        a, f = f'layers.{k}.0.', f'layers.{k}.1.'
        shapes.update({a + 'norm1.weight': (D,), a + 'norm1.bias': (D,), a + 'norm2.weight': (D,), a + 'norm2.bias': (D,), a + 'to_q.weight': (inner, D),
                       a + 'to_kv.weight': (2 * inner, D), a + 'to_out.weight': (D, inner), f + '0.weight': (D,), f + '0.bias': (D,), f + '1.weight': (F, D),
                       f + '3.weight': (D, F)})
    sd = {}
    for n, s in shapes.items():
        if len(s) == 1:
            sd[n] = ((1.0 if n.endswith('weight') else 0.0) + 0.02 * torch.randn(*s, generator=g)).half()
        else:
            sd[n] = (s[-1] ** -0.5 * torch.randn(*s, generator=g)).half()
    return sd


def transformers_module(cfg, sd):
    try:
        from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    except Exception:
        return None
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg))
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith('position_ids') for k in missing), (missing, unexpected)
    return m.half().cuda().eval()


def per_class(table, op_ms):
    out = {}
    for (cls, _, lab), ms in zip(table, op_ms):
        if lab not in COPIES:
            out[cls] = out.get(cls, 0.0) + ms
    return ', '.join(f'{k} {v:.4f}' for k, v in sorted(out.items())) + f', sum {sum(out.values()):.4f}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_vision.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('clip_vision_report needs the GPU: nothing is measured without one')
    cfg, B = dict(VIT_H_14_VISION_CONFIG), 2
    sd = synthetic_state_dict(cfg)
    eng = CLIPVisionEngine.from_state_dict(sd, cfg, torch.float16, 'cuda', with_projection=True)
    res = ResamplerEngine(dtype=torch.float16, device='cuda', **RESAMPLER)
    res.load_state_dict(synthetic_resampler_state_dict(res))
    px = torch.randn(B, 3, cfg['image_size'], cfg['image_size'], generator=torch.Generator().manual_seed(1)).half().cuda()
    info, table = eng.plan(B), None
    table = eng.op_table()
    launches = sum(lab not in COPIES for _, _, lab in table)
    feats = eng.run(px, output_hidden_states=True)[3][-2]
    rinfo = res.plan(B, feats.shape[1])
    rtable = res.op_table()
    rlaunches = sum(lab not in COPIES for _, _, lab in rtable)
    hf = transformers_module(cfg, sd)
    fns = [lambda: eng.run(px), lambda: res.run(feats)]
    if hf is not None:
        torch.set_grad_enabled(False)
        fns.append(lambda: hf(pixel_values=px))
    (t, reps) = windows(fns)
    op_ms = eng.run(px, profile=True)[-1]
    rop_ms = res.run(feats, profile=True)[-1]
    lines = [f'# tools/clip_vision_report.py on {torch.cuda.get_device_name(0)}: CLIP ViT-H/14 vision tower (1280 wide, 32 layers, 16 heads, MLP 5120, 257 tokens), '
             f'fp16, synthetic weights, B = {B}; measured once, untuned',
             f'tower plan: {info["n_ops"]} ops, {launches} kernel launches per forward without output_hidden_states '
             f'(+ {info["n_ops"] - launches} device copies: last_hidden_state, and the hidden states when asked for), workspace {info["workspace_bytes"]} bytes',
             f'tower forward (Python call to last kernel, device events): {t[0] * 1e3:.4f} ms  (median of 3 windows of {reps[0]} calls, >= 0.5 s each)',
             'tower per-class device time of one profiled forward (events around every op, so launch gaps are included), ms: ' + per_class(table, op_ms),
             f'tower flops of the plan: linear {info["flops"]["linear"]:.4g}, attention {info["flops"]["attention"]:.4g}']
    if hf is not None:
        mine, theirs = eng(px, output_hidden_states=True), hf(pixel_values=px, output_hidden_states=True)
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
        lines.append(f'transformers CLIPVisionModelWithProjection.half() on the same weights, same process, alternating windows: {t[2] * 1e3:.4f} ms '
                     f'(median of 3 windows of {reps[2]} calls); engine vs that module, rel-L2: image_embeds {rel(mine.image_embeds, theirs.image_embeds):.3e}, '
                     f'hidden_states[-2] {rel(mine.hidden_states[-2], theirs.hidden_states[-2]):.3e}')
    else:
        lines.append('transformers CLIPVisionModelWithProjection.half(): not measured (transformers does not import here)')
    lines += [f'Resampler (dim 768, depth 4, 12 heads, 16 queries, 1280 -> 768) on hidden_states[-2] [{B}, {feats.shape[1]}, {feats.shape[2]}]: plan {rinfo["n_ops"]} ops, '
              f'{rlaunches} kernel launches (+ 1 op of {B} device copies: latents.repeat), workspace {rinfo["workspace_bytes"]} bytes',
              f'Resampler forward (Python call to last kernel, device events): {t[1] * 1e3:.4f} ms  (median of 3 windows of {reps[1]} calls); '
              f'the reference\'s torch Resampler is not in this repository: not measured',
              'Resampler per-class device time of one profiled forward, ms: ' + per_class(rtable, rop_ms)]
    print('\n'.join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
