"""One timing of the native CLIP text tower, with no target: the full-size ViT-L/14 text tower (vocab 49408, 77 positions, 768 wide, 12 layers,
12 heads, 3072, quick_gelu) with seeded synthetic weights, B = 2, L = 77.  Device events around windows of at least half a second after a
warm-up, three windows, the median reported; the launch count and the per-class time come from the plan (`mve_unet_op_info`) and one profiled
forward.  Where `transformers` imports, its own half-precision CLIPTextModel with the same weights is timed in the same process, the windows
alternating with the engine's; otherwise the file says "not measured".  The text tower runs once per request, not once per denoising step.

    python tools/clip_text_report.py [--out profiles/clip_text.txt]
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvedit_amd.text_encoder import CLIPTextEngine, VIT_L_14_TEXT_CONFIG  # noqa: E402
from tools.microbench import timeit  # noqa: E402


def synthetic_state_dict(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    C, I, nl = cfg['hidden_size'], cfg['intermediate_size'], cfg['num_hidden_layers']
    sd = {}

    def put(name, shape, std, mean=0.0):
        sd[name] = (mean + std * torch.randn(*shape, generator=g)).half()
    put('text_model.embeddings.token_embedding.weight', (cfg['vocab_size'], C), 0.02)
    put('text_model.embeddings.position_embedding.weight', (cfg['max_position_embeddings'], C), 0.02)
    w = C ** -0.5 * (2 * nl) ** -0.5
    for k in range(nl):
        b = f'text_model.encoder.layers.{k}.'
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
    put('text_model.final_layer_norm.weight', (C,), 0.02, 1.0)
    put('text_model.final_layer_norm.bias', (C,), 0.02)
    return sd


def transformers_module(cfg, sd):
    try:
        from transformers import CLIPTextConfig, CLIPTextModel
    except Exception:
        return None
    m = CLIPTextModel(CLIPTextConfig(**{k: v for k, v in cfg.items()}, pad_token_id=1, bos_token_id=0))
    own = sd if hasattr(m, 'text_model') else {k[len('text_model.'):]: v for k, v in sd.items()}
    missing, unexpected = m.load_state_dict(own, strict=False)
    assert not unexpected and all(k.endswith('position_ids') for k in missing), (missing, unexpected)
    return m.half().cuda().eval()


def windows(fns, min_seconds=0.5, n=3):
    """median per-call seconds of every fn over n alternating windows of at least min_seconds each"""
    reps = [max(10, math.ceil(min_seconds * 1.2 / timeit(f, 5, 20))) for f in fns]
    ts = [[] for _ in fns]
    for _ in range(n):
        for i, f in enumerate(fns):
            ts[i].append(timeit(f, 3, reps[i]))
    return [sorted(t)[n // 2] for t in ts], reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_text.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('clip_text_report needs the GPU: nothing is measured without one')
    cfg, B, L = dict(VIT_L_14_TEXT_CONFIG), 2, 77
    sd = synthetic_state_dict(cfg)
    eng = CLIPTextEngine.from_state_dict(sd, cfg, torch.float16, 'cuda')
    ids = torch.randint(0, cfg['vocab_size'] - 1, (B, L), generator=torch.Generator().manual_seed(1))
    ids[:, -1] = cfg['vocab_size'] - 1
    ids = ids.cuda()
    ids32 = ids.int()
    info = eng.plan(B, L)
    table = eng.op_table()
    launches = sum(lab != 'hidden state -> output' for _, _, lab in table)
    hf = transformers_module(cfg, sd)
    fns = [lambda: eng.run(ids32)]
    if hf is not None:
        torch.set_grad_enabled(False)
        fns.append(lambda: hf(input_ids=ids))
    (t, reps) = windows(fns)
    op_ms = eng.run(ids32, profile=True)[-1]
    per_class = {}
    for (cls, _, lab), ms in zip(table, op_ms):
        if lab != 'hidden state -> output':
            per_class[cls] = per_class.get(cls, 0.0) + ms
    lines = [f'# tools/clip_text_report.py on {torch.cuda.get_device_name(0)}: CLIP ViT-L/14 text tower, fp16, synthetic weights, B = {B}, L = {L}',
             f'plan: {info["n_ops"]} ops, {launches} kernel launches per forward without output_hidden_states '
             f'(+ {info["n_ops"] - launches} device copies with it), workspace {info["workspace_bytes"]} bytes',
             f'engine forward (Python call to last kernel, device events): {t[0] * 1e3:.4f} ms  (median of 3 windows of {reps[0]} calls, >= 0.5 s each)',
             'per-class device time of one profiled forward (events around every op, so launch gaps are included), ms: '
             + ', '.join(f'{k} {v:.4f}' for k, v in sorted(per_class.items())) + f', sum {sum(per_class.values()):.4f}',
             f'flops of the plan: linear {info["flops"]["linear"]:.4g}, attention {info["flops"]["attention"]:.4g}']
    if hf is not None:
        a, b = eng.run(ids32)[0].double(), hf(input_ids=ids).last_hidden_state.double()
        lines.append(f'transformers CLIPTextModel.half() on the same weights, same process, alternating windows: {t[1] * 1e3:.4f} ms '
                     f'(median of 3 windows of {reps[1]} calls); engine vs that module, last_hidden_state rel-L2 {float((a - b).norm() / b.norm()):.3e}')
    else:
        lines.append('transformers CLIPTextModel.half(): not measured (transformers does not import here)')
    print('\n'.join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
