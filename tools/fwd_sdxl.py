"""One full-size SDXL UNet forward (BASELINE config 5 topology: 768 x 768 image = 96 x 96 latent) with its 'text_time' added conditions, B = 2,
seeded synthetic fp16 weights: finiteness, wall time over a few repeats, per-class milliseconds from profile() and the plan's TFLOP.
Measured, untuned, no target: the reference has no SDXL pipeline to compare with.  Output kept as profiles/sdxl_forward.txt."""
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvedit_amd import synthetic  # noqa: E402
from mvedit_amd.unet import OP_CLASSES, SDXL_CONFIG, UNet2DConditionEngine  # noqa: E402

dev, dtype = torch.device('cuda', 0), torch.float16
B, S, CTX_LEN, REPEATS = 2, 96, 77, 5
cfg = dict(SDXL_CONFIG)

# synthetic.make_state_dict's rule (unit-gain uniform weights, 0.1 N(0,1) biases, norm scales 1 + 0.1 N(0,1)), drawn on the device and loaded tensor by
# tensor: 2.57 G parameters never sit in host memory
t0 = time.time()
eng = UNet2DConditionEngine(cfg, dtype, dev)
g = torch.Generator(device=dev).manual_seed(1234)
n_params = 0
for name, shape in synthetic.param_shapes(cfg).items():
    if name.endswith('.bias'):
        w = 0.1 * torch.randn(shape, generator=g, device=dev)
    elif '.norm' in name or name.startswith('conv_norm_out'):
        w = 1.0 + 0.1 * torch.randn(shape, generator=g, device=dev)
    else:
        w = (torch.rand(shape, generator=g, device=dev) * 2 - 1) * math.sqrt(3.0 / math.prod(shape[1:]))
    eng.load_state_dict({name: w.to(dtype)}, strict=False)
    n_params += w.numel()
eng.load_state_dict({}, strict=True)
print(f'SDXL UNet: {n_params} parameters, {eng.weight_bytes / 2 ** 30:.2f} GiB packed, built in {time.time() - t0:.1f} s')

x = torch.randn(B, 4, S, S, generator=g, device=dev).to(dtype)
ctx = torch.randn(B, CTX_LEN, cfg['cross_attention_dim'], generator=g, device=dev).to(dtype)
ack = dict(text_embeds=torch.randn(B, 1280, generator=g, device=dev).to(dtype),
           time_ids=torch.tensor([[768., 768., 0., 0., 768., 768.]] * B, device=dev))
info = eng.plan(B, S, S, CTX_LEN)
tflop = sum(info['flops'][k] for k in ('conv3x3', 'linear', 'attention')) / 1e12
print(f'plan: B={B} {S}x{S} latent, ctx {CTX_LEN} x {cfg["cross_attention_dim"]}: {info["n_ops"]} ops, {tflop:.4f} TFLOP '
      f'({tflop / B:.4f} per image), workspace {info["workspace_bytes"] / 2 ** 20:.0f} MiB, residual_pair={eng.residual_pair}')

out = eng(x, 499, ctx, added_cond_kwargs=ack)[0]
torch.cuda.synchronize()
print(f'output {tuple(out.shape)} {out.dtype}: finite={bool(torch.isfinite(out).all())} mean|x|={out.float().abs().mean().item():.4f}')
for _ in range(2):
    eng(x, 499, ctx, added_cond_kwargs=ack)
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(REPEATS + 1)]
ev[0].record()
for i in range(REPEATS):
    eng(x, 499, ctx, added_cond_kwargs=ack)
    ev[i + 1].record()
torch.cuda.synchronize()
ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(REPEATS)]
print('forward ms:', ' '.join(f'{m:.3f}' for m in ms), f'| median {sorted(ms)[REPEATS // 2]:.3f} ms = {tflop / (sorted(ms)[REPEATS // 2] * 1e-3):.1f} TFLOP/s')

_, rows = eng.profile(x, 499, ctx, added_cond_kwargs=ack)
print('per class (profile(): every op bracketed by events, so the sum exceeds the back-to-back forward):')
for cls in OP_CLASSES:
    sel = [(fl, m) for c, _, fl, m in rows if c == cls]
    fl, m = sum(f for f, _ in sel), sum(t for _, t in sel)
    print(f'  {cls:10s} n={len(sel):4d} ms={m:8.3f} GFLOP={fl / 1e9:9.1f}' + (f' TFLOP/s={fl / m / 1e9:6.1f}' if fl and m else ''))
for lab in ('add_embedding.text_time', 'add_embedding.linear_1', 'add_embedding.linear_2'):
    print(f'  {lab}: ' + ' '.join(f'{m:.3f} ms' for _, l, _, m in rows if l == lab))
