"""One untuned timing of the SAM mask decoder engine, with no target: the full-size decoder (G = 64, one box, multimask) and `predict` end to end at
1024 x 1024, next to transformers' fp32 `SamModel` prompt encoder + mask decoder on the same weights in the same process.

    python tools/sam_decoder_report.py [--out profiles/sam_decoder.txt] [--steps 20] [--warmup 3]

Weights are seeded random (tests/golden/make_sam_decoder_golden.py's scaling); the image embedding is random fp16.  `predict` is timed without the image
encoder: the predictor's features are set by hand, so the figure is prompt scaling + decoder + mask post-processing + the copies to numpy."""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def golden_generator():
    spec = importlib.util.spec_from_file_location('make_sam_decoder_golden', os.path.join(ROOT, 'tests', 'golden', 'make_sam_decoder_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn, steps, warmup):
    """-> ms per call, by events around `steps` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def wall(fn, steps, warmup):
    """-> ms per call on the host clock (the call ends with its result on the host)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sam_decoder.txt'))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    import torch.nn.functional as F
    from mvedit_amd.sam import SAM_VIT_B_CONFIG, SamImageEncoderEngine, SamMaskDecoderEngine, SamPredictorEngine
    G = golden_generator()
    G.CASES['full'] = dict(grid=64, B=1, P=1, box=True, n_points=0, layer_norm_eps=1e-6, final_layer_norm_eps=1e-5, seed=4199)
    model = G.build_module('full', torch.float32).cuda()
    dec = SamMaskDecoderEngine.from_module(model)
    emb = torch.randn(1, 256, 64, 64, generator=torch.Generator().manual_seed(0)).half().cuda()
    box = torch.tensor([[[200.0, 150.0, 820.0, 700.0]]], device='cuda')
    lines = [f'SAM mask decoder engine, one untuned timing ({torch.cuda.get_device_name(0)}; steps {args.steps}, warmup {args.warmup}); nothing here is a target',
             'full-size decoder: hidden 256, 8 heads, mlp 2048, 2 layers, 3 + 1 mask tokens, G = 64 (S = 1024), B = 1, P = 1, one box (T = 7), multimask_output=True', '']

    def torch_decoder():
        with torch.no_grad():
            sparse, dense = model.prompt_encoder(None, None, box, None)
            pe = model.get_image_wide_positional_embeddings()
            return model.mask_decoder(image_embeddings=emb.float(), image_positional_embeddings=pe, sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense,
                                      multimask_output=True)
    low, iou, _ = dec.run(emb, box)
    ref_low, ref_iou = torch_decoder()
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    info = dec.plan(1, 1, 0, True)
    table = dec.op_table()
    n_taps = sum(1 for row in table if row[2] == 'tap -> output')
    lines += [f'engine against the torch fp32 GPU module on the same weights (rel-L2): low_res_masks {rel(low, ref_low):.3e}, iou {rel(iou, ref_iou):.3e}',
              f'plan: {info["n_ops"]} ops, of which {n_taps} are optional tap copies that launch nothing without taps; the two upscale ops launch twice (GEMM + shuffle): '
              f'{info["n_ops"] - n_taps + 2} kernel launches per forward; workspace {info["workspace_bytes"] / 2 ** 20:.1f} MiB; '
              f'{sum(info["flops"].values()) / 1e9:.2f} GFLOP ({", ".join(f"{k} {v / 1e9:.2f}" for k, v in info["flops"].items() if v)})', '']
    t_eng = timed(lambda: dec.run(emb, box), args.steps, args.warmup)
    t_torch = timed(torch_decoder, args.steps, args.warmup)
    lines += ['decoder forward (prompt encoding + two-way transformer + upscaling + masks), ms per call by events:',
              f'    engine (fp32 kernels)                         {t_eng:8.3f}', f'    transformers SamModel, fp32, eager on the GPU   {t_torch:8.3f}', '']
    ms = dec.run(emb, box, profile=True)[3]
    by_label = {}
    for (cls, fl, label), m in zip(table, ms):
        by_label.setdefault(label, [0, 0.0])
        by_label[label][0] += 1
        by_label[label][1] += m
    lines.append('per-op time of one profiled forward (events around every op; sums by label):')
    for label, (n, m) in sorted(by_label.items(), key=lambda kv: -kv[1][1]):
        lines.append(f'    {label:40s} x{n:3d} {m:8.3f} ms')
    lines.append('')
    # predict end to end at 1024 x 1024: features set by hand (the image encoder is not part of this figure)
    pred = SamPredictorEngine(SamImageEncoderEngine(SAM_VIT_B_CONFIG, torch.float16, 'cpu'), dec)
    pred.features, pred.original_size, pred.input_size, pred.is_image_set = emb, (1024, 1024), (1024, 1024), True
    npbox = np.array([200, 150, 820, 700])

    def torch_predict():
        with torch.no_grad():
            lo, io = torch_decoder()
            m = F.interpolate(lo[0], (1024, 1024), mode='bilinear', align_corners=False)[..., :1024, :1024]
            m = F.interpolate(m, (1024, 1024), mode='bilinear', align_corners=False) > 0.0
            return m[0].cpu().numpy(), io[0, 0].cpu().numpy(), lo[0, 0].cpu().numpy()
    masks, _, _ = pred.predict(box=npbox)
    tm = torch_predict()[0]
    t_pe, t_pt = wall(lambda: pred.predict(box=npbox), args.steps, args.warmup), wall(torch_predict, args.steps, args.warmup)
    lines += ['predict(box) end to end at 1024 x 1024 -> numpy (masks [3, 1024, 1024] bool, iou, low_res), ms per call on the host clock:',
              f'    SamPredictorEngine.predict                    {t_pe:8.3f}', f'    transformers modules + two F.interpolate       {t_pt:8.3f}',
              f'    binary masks: {int((masks == tm).sum())} pixels agree, {int((masks != tm).sum())} differ of {masks.size}']
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
