"""One timing of the native DPT-hybrid normal predictor, with no target: the full-size network (ResNetV2-50 stem and stages 3 / 4 / 9 with 32 groups,
ViT-B over 577 tokens, decoder width 256, three output channels -- `VITB_RN50_384_CONFIG`) on `DPTNormalEngine` with seeded synthetic fp16
weights, B = 2 at 384 x 384, next to transformers' own half-precision `DPTForDepthEstimation` (is_hybrid, BitBackbone; its last head convolution
widened to three channels) on the same weights in the same process, the windows alternating.  Device events around windows of at least half a
second after a warm-up, three windows, the median reported; the launch count and the per-class time come from the plan (`mve_unet_op_info`) and
one profiled forward.  The predictor runs once per request, not once per denoising step.  Measured once, untuned.

    python tools/dpt_normal_report.py [--out profiles/dpt_normal.txt]          (needs `transformers`: the synthetic weights take its module's shapes)
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvedit_amd.normal_model import DPTNormalEngine, VITB_RN50_384_CONFIG  # noqa: E402
from tools.clip_text_report import windows  # noqa: E402


def transformers_module(c, seed=0):
    """transformers' DPTForDepthEstimation of the engine config `c` with seeded weights (fan-in scaled; norms 1 +- 0.02), float32 on the CPU."""
    from transformers import BitConfig, DPTConfig, DPTForDepthEstimation
    G = c['image_size'] // 16
    bc = BitConfig(layer_type='bottleneck', global_padding='same', embedding_dynamic_padding=True, out_features=['stage1', 'stage2', 'stage3'],
                   embedding_size=c['stem_width'], hidden_sizes=list(c['stage_widths']), depths=list(c['stage_depths']), num_groups=c['num_groups'])
    cfg = DPTConfig(is_hybrid=True, readout_type='project', neck_ignore_stages=[0, 1], reassemble_factors=[1, 1, 1, 0.5], backbone_config=bc,
                    hidden_size=c['hidden_size'], num_attention_heads=c['num_heads'], num_hidden_layers=c['num_layers'], intermediate_size=c['intermediate_size'],
                    image_size=c['image_size'], patch_size=16, backbone_out_indices=[0, 0, c['tap_layers'][0], c['tap_layers'][1]],
                    neck_hidden_sizes=[c['stage_widths'][0], c['stage_widths'][1], c['neck_channels'][0], c['neck_channels'][1]],
                    fusion_hidden_size=c['features'], backbone_featmap_shape=[1, c['stage_widths'][2], G, G], layer_norm_eps=c['layer_norm_eps'], hidden_act='gelu',
                    qkv_bias=True)
    m = DPTForDepthEstimation(cfg)
    m.head.head[4] = torch.nn.Conv2d(32, c['num_channels'], kernel_size=1)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.copy_((1.0 if ('norm' in n and n.endswith('weight')) else 0.0) + 0.02 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(p[0].numel() ** -0.5 * torch.randn(p.shape, generator=g) if p.dim() > 1 and 'embeddings.cls' not in n and 'position' not in n
                        else 0.02 * torch.randn(p.shape, generator=g))
    return m.eval()


def per_class(table, op_ms):
    out = {}
    for (cls, _, lab), ms in zip(table, op_ms):
        if not lab.endswith('-> tap'):
            out[cls] = out.get(cls, 0.0) + ms
    return ', '.join(f'{k} {v:.4f}' for k, v in sorted(out.items())) + f', sum {sum(out.values()):.4f}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dpt_normal.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dpt_normal_report needs the GPU: nothing is measured without one')
    cfg, B = dict(VITB_RN50_384_CONFIG), 2
    hf = transformers_module(cfg)
    sd = {k: v.half() for k, v in hf.state_dict().items()}
    eng = DPTNormalEngine(cfg, torch.float16, 'cuda').load_state_dict(sd)
    hf = hf.half().cuda()
    torch.set_grad_enabled(False)
    S = cfg['image_size']
    px = (0.5 * torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(1))).half().cuda()
    info, table = eng.plan(B), eng.op_table()
    launches = sum(not lab.endswith('-> tap') for _, _, lab in table)

    def hf_forward():
        return hf(pixel_values=px).predicted_depth

    (t, reps) = windows([lambda: eng.run(px), hf_forward])
    op_ms = eng.run(px, profile=True)[-1]
    mine, theirs = eng(px), hf_forward()
    hf32 = transformers_module(cfg)
    hf32.load_state_dict({k: v.float() for k, v in sd.items()})                   # the same 16-bit weights, fp32 arithmetic: the yardstick of both
    ref = hf32.cuda()(pixel_values=px.float()).predicted_depth.double()
    rel = lambda a: float((a.double() - ref).norm() / ref.norm())      # noqa: E731
    fl = info['flops']
    lines = [f'# tools/dpt_normal_report.py on {torch.cuda.get_device_name(0)}: DPT-hybrid normal predictor (ResNetV2-50 3/4/9, ViT-B 12 layers over 577 tokens, decoder 256, '
             f'3 channels), fp16, synthetic weights, B = {B} at {S} x {S}; measured once, untuned',
             f'plan: {info["n_ops"]} ops, {launches} kernel launches per forward (+ {info["n_ops"] - launches} tap copies, made only with output_features=True), '
             f'workspace {info["workspace_bytes"]} bytes',
             f'engine forward (Python call to last kernel, device events): {t[0] * 1e3:.4f} ms  (median of 3 windows of {reps[0]} calls, >= 0.5 s each)',
             'per-class device time of one profiled forward (events around every op, so launch gaps are included), ms: ' + per_class(table, op_ms),
             f'flops of the plan: conv {fl["conv"]:.4g}, linear {fl["linear"]:.4g}, attention {fl["attention"]:.4g}',
             f'transformers DPTForDepthEstimation.half() (hybrid, three-channel head) on the same weights, same process, alternating windows: {t[1] * 1e3:.4f} ms '
             f'(median of 3 windows of {reps[1]} calls)',
             f'rel-L2 of the output against the same module in fp32 on the same 16-bit weights: engine {rel(mine):.3e}, transformers half module {rel(theirs):.3e}']
    print('\n'.join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
