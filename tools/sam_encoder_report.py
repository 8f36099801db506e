"""One timing of the native SAM image encoder, with no target: the full-size ViT-H encoder of `sam_vit_h` (1280 wide, 32 blocks, 16 heads of 80, MLP
5120, 1024 / 16 -> a 64 x 64 grid, 14 x 14 windows, global blocks 7 / 15 / 23 / 31, neck 256) with seeded synthetic fp16 weights at B = 1 -- what
`SamPredictor.set_image` runs once per request.  Device events around windows of at least half a second after a warm-up, three windows, the median
reported; the launch count and the per-stage time come from the plan (`mve_unet_op_info`) and one profiled forward (events around every op, so
launch gaps are included).  Where `transformers` imports, its own half-precision SamVisionEncoder with the same weights is timed in the same
process, the windows alternating with the engine's; otherwise the file says "not measured".  segment_anything is not installed here and is not
timed.  Measured once, untuned: mve_attention_relpos in particular is a first version (one block per 64 queries, 64-key tiles, three block
barriers per tile).

    python tools/sam_encoder_report.py [--out profiles/sam_encoder.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvedit_amd.sam import SAM_VIT_H_CONFIG, SamImageEncoderEngine  # noqa: E402
from tools.clip_text_report import windows  # noqa: E402

COPIES = ('hidden state -> output',)
STAGES = (('patch embedding + pos_embed', ('patchify', 'patch_embed', 'position embedding')),
          ('layernorm', ('layernorm',)),
          ('window partition / un-partition', ('window partition', 'window un-partition')),
          ('qkv GEMM', ('attn.qkv',)),
          ('rel-pos attention, 28 windowed blocks', ('rel-pos attention (windows)',)),
          ('rel-pos attention, 4 global blocks', ('rel-pos attention (global)',)),
          ('proj GEMM + residual', ('attn.proj+residual',)),
          ('MLP GEMMs + GELU', ('mlp.lin1', 'gelu', 'mlp.lin2+residual')),
          ('neck', ('neck.conv1', 'neck.conv2', 'nhwc->nchw')))


def synthetic_state_dict(cfg, seed=0):
    """transformers-named fp16 tensors; the tables and pos_embed are NOT zero (transformers' initialisation), so the bias path does real work"""
    g = torch.Generator().manual_seed(seed)
    C, I, nl, P, O, w = cfg['hidden_size'], cfg['mlp_dim'], cfg['num_hidden_layers'], cfg['patch_size'], cfg['output_channels'], cfg['window_size']
    G, hd = cfg['image_size'] // P, cfg['hidden_size'] // cfg['num_attention_heads']
    sd = {}

    def put(name, shape, std, mean=0.0):
        sd[name] = (mean + std * torch.randn(*shape, generator=g)).half()
    put('patch_embed.projection.weight', (C, 3, P, P), 0.02)
    put('patch_embed.projection.bias', (C,), 0.02)
    put('pos_embed', (1, G, G, C), 0.02)
    wa = C ** -0.5 * (2 * nl) ** -0.5
    for k in range(nl):
        b, n = f'layers.{k}.', (G if k in cfg['global_attn_indexes'] else w)
        for nm in ('layer_norm1', 'layer_norm2'):
            put(b + nm + '.weight', (C,), 0.02, 1.0)
            put(b + nm + '.bias', (C,), 0.02)
        put(b + 'attn.qkv.weight', (3 * C, C), C ** -0.5)
        put(b + 'attn.qkv.bias', (3 * C,), 0.02)
        put(b + 'attn.rel_pos_h', (2 * n - 1, hd), 0.1 * hd ** -0.5)
        put(b + 'attn.rel_pos_w', (2 * n - 1, hd), 0.1 * hd ** -0.5)
        put(b + 'attn.proj.weight', (C, C), wa)
        put(b + 'attn.proj.bias', (C,), 0.02)
        put(b + 'mlp.lin1.weight', (I, C), (2 * C) ** -0.5)
        put(b + 'mlp.lin1.bias', (I,), 0.02)
        put(b + 'mlp.lin2.weight', (C, I), wa)
        put(b + 'mlp.lin2.bias', (C,), 0.02)
    put('neck.conv1.weight', (O, C, 1, 1), C ** -0.5)
    put('neck.conv2.weight', (O, O, 3, 3), (9 * O) ** -0.5)
    for nm in ('neck.layer_norm1', 'neck.layer_norm2'):
        put(nm + '.weight', (O,), 0.02, 1.0)
        put(nm + '.bias', (O,), 0.02)
    return sd


def transformers_module(cfg, sd):
    try:
        from transformers import SamVisionConfig
        from transformers.models.sam.modeling_sam import SamVisionEncoder
    except Exception:
        return None
    m = SamVisionEncoder(SamVisionConfig(**dict(cfg, global_attn_indexes=list(cfg['global_attn_indexes']))))
    m.load_state_dict(sd, strict=True)
    return m.half().cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sam_encoder.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sam_encoder_report needs the GPU: nothing is measured without one')
    cfg, B = dict(SAM_VIT_H_CONFIG), 1
    sd = synthetic_state_dict(cfg)
    eng = SamImageEncoderEngine.from_state_dict(sd, cfg, torch.float16, 'cuda')
    px = torch.randn(B, 3, cfg['image_size'], cfg['image_size'], generator=torch.Generator().manual_seed(1)).half().cuda()
    info = eng.plan(B)
    table = eng.op_table()
    launches = sum(lab not in COPIES for _, _, lab in table)
    hf = transformers_module(cfg, sd)
    fns = [lambda: eng.run(px)]
    if hf is not None:
        torch.set_grad_enabled(False)
        fns.append(lambda: hf(px))
    (t, reps) = windows(fns)
    op_ms = eng.run(px, profile=True)[-1]
    by_label = {}
    for (_, _, lab), ms in zip(table, op_ms):
        by_label[lab] = by_label.get(lab, 0.0) + ms
    lines = [f'# tools/sam_encoder_report.py on {torch.cuda.get_device_name(0)}: SAM ViT-H image encoder (1280 wide, 32 blocks, 16 heads of 80, MLP 5120, 64 x 64 grid, '
             f'14 x 14 windows, 4 global blocks, neck 256), fp16, synthetic weights, B = {B}, 1024 x 1024; measured once, untuned, no target',
             f'plan: {info["n_ops"]} ops, {launches} kernel launches per forward without output_hidden_states (+ {info["n_ops"] - launches} device copies when the '
             f'hidden states are asked for), workspace {info["workspace_bytes"]} bytes',
             f'forward (Python call to last kernel, device events): {t[0] * 1e3:.3f} ms  (median of 3 windows of {reps[0]} calls, >= 0.5 s each)',
             f'flops of the plan: linear {info["flops"]["linear"]:.4g}, attention {info["flops"]["attention"]:.4g} (QK^T and PV; the bias products are not counted), '
             f'conv {info["flops"]["conv"]:.4g}',
             'per-stage device time of one profiled forward (events around every op, so launch gaps are included), ms:']
    total = 0.0
    for name, labels in STAGES:
        ms = sum(by_label.get(lab, 0.0) for lab in labels)
        total += ms
        lines.append(f'    {name:42s} {ms:9.3f}')
    lines.append(f'    {"sum":42s} {total:9.3f}')
    if hf is not None:
        mine, theirs = eng(px), hf(px).last_hidden_state
        rel = float((mine.double() - theirs.double()).norm() / theirs.double().norm())
        lines.append(f'transformers SamVisionEncoder.half() ({hf.config._attn_implementation} attention) on the same weights, same process, alternating windows: '
                     f'{t[1] * 1e3:.3f} ms (median of 3 windows of {reps[1]} calls); engine vs that module, rel-L2 of the neck output: {rel:.3e}')
    else:
        lines.append('transformers SamVisionEncoder.half(): not measured (transformers does not import here)')
    lines.append('not measured: segment_anything\'s ImageEncoderViT (not installed), the real sam_vit_h_4b8939.pth, SamPredictor.set_image over the engine; '
                 'the prompt encoder and the mask decoder stay torch modules and are not part of this timing')
    print('\n'.join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
