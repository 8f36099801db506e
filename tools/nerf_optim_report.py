"""One timing, with no target, of a `nerf_optim` iteration in its exact form (two host reads of a sample count per iteration) against
the capacity form (`VolumeRenderer.forward(capacity=C)`: counts stay on the device), both run eagerly.  Graph replay: not measured
(no capture helper is shipped).

Configuration of tools/bench_parts.py's `nerf_iter`: 128^2 rays of one view, 128^3 occupancy sphere, 12-level hash grid, max_steps 512,
normal_reg_weight 0.5, entropy_weight 0.2, LPIPS patch term (bf16, synthetic VGG weights), lr 1e-2.  The exact path steps with
torch.optim.Adam as bench_parts does; the capacity paths step with the native `adam_step(skip_if=overflow)`.  A third form, the exact
path with the native `adam_step`, separates the two changes: exact (native Adam) against capacity is what the two host reads cost,
exact (torch.optim.Adam) against exact (native Adam) is the optimiser.  The capacity is 1.25 x and 2 x the marched sample count.

Both forms are also timed without the patch term: that is the part of the iteration this mode changes.

All variants run in one process, alternating (round-robin over the variants, --repeats times), --iters iterations each after a warm-up;
a host clock around the iterations and a closing device synchronise.  Launches per iteration: device activities (kernels, memsets,
copies) seen by torch.profiler over one call.  The marched total every capacity variant reports after each window is checked against
the exact path's.  Nothing here is a pass / fail bar.

    python tools/nerf_optim_report.py [--out profiles/nerf_optim_capacity.txt] [--iters 200] [--repeats 3]
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from mvedit_amd import nerf, raymarching as rm, synthetic as SY  # noqa: E402
from mvedit_amd.lpips import LPIPSEngine  # noqa: E402
from mvedit_amd.recon_loss import nerf_optim_loss  # noqa: E402
from mvedit_amd.tonemapping import Tonemapping  # noqa: E402
from tools.bench_parts import surround_poses  # noqa: E402
from scene import sphere_density_grid  # noqa: E402


def launches(fn):
    """device activities of one call, or None where the profiler is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nerf_optim_capacity.txt'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    g = torch.Generator().manual_seed(0)
    S, ps, P = 512, 128, 1
    meta, rows = nerf.grid_meta(12, 16, 320)
    table = (torch.rand(rows, 2, generator=g) * 2 - 1) * 0.1
    w1 = (torch.rand(64, 24, generator=g) * 2 - 1) * math.sqrt(6 / (64 + 24))
    w2 = (torch.rand(4, 64, generator=g) * 2 - 1) * math.sqrt(6 / (4 + 64))
    bits = rm.packbits(torch.from_numpy(sphere_density_grid(128, radius=0.5)).to(dev), 0.5)
    fl = S / (2 * math.tan(math.radians(15)))
    intr = torch.tensor([[fl, fl, S / 2, S / 2]] * P, device=dev)
    poses = surround_poses(32)[:P].to(dev)
    tm = Tonemapping(device=dev)
    lights = torch.nn.functional.normalize(torch.tensor([[0.3, -0.5, -1.0]] * P, device=dev), dim=-1)
    ro, rd, _ = nerf.camera_rays(intr * (ps / S), poses, ps, ps)
    ys, xs = torch.meshgrid(torch.arange(ps, dtype=torch.float32), torch.arange(ps, dtype=torch.float32), indexing='ij')
    flp = ps / (2 * math.tan(math.radians(15)))
    dirs = torch.stack([(xs + 0.5 - ps / 2) / flp, (ys + 0.5 - ps / 2) / flp, torch.ones_like(xs)], -1)[None].repeat(P, 1, 1, 1).to(dev)
    tgt_m = torch.rand(P, ps, ps, 1, generator=g).to(dev)
    tgt_rgb = torch.rand(P, ps, ps, 3, generator=g).to(dev)
    tgt_nchw = tgt_rgb.permute(0, 3, 1, 2)
    patch_w = torch.ones(P, device=dev)
    lp = LPIPSEngine.from_state_dict({k: v.to(torch.bfloat16).float() for k, v in SY.make_lpips_state_dict().items()}, torch.bfloat16, device=dev)

    def fresh():
        dec = nerf.INGPDecoderParams(table, w1, torch.zeros(64), w2, torch.tensor([2.0, 0.0, 0.0, 0.0]), 12, 320, device=dev)
        dec.max_steps = 512
        for t in dec.parameters().values():
            t.requires_grad_(True)
        vr = nerf.VolumeRenderer(dec)
        vr.training = True
        return vr, dec

    def loss_of(o, lpips, n_samples=None):
        res = nerf_optim_loss(o['image'], o['weights_sum'], o['depth'], o['weights'], o['ts'][0], tgt_rgb, tgt_m, dirs, patch_w, lights,
                              tonemapping=tm, shaded=True, normal_reg_weight=0.5, entropy_weight=0.2, n_samples=n_samples)
        loss = res['loss']
        if lpips:
            loss = loss + 0.3 * lp(res['out_rgbs'].permute(0, 3, 1, 2), tgt_nchw).mean()
        return loss

    def exact(lpips):
        vr, dec = fresh()
        opt = torch.optim.Adam(list(dec.parameters().values()), lr=1e-2, eps=1e-15)

        def it():
            opt.zero_grad()
            loss_of(vr.forward(ro, rd, bits, 128, dt_gamma=0.0), lpips).backward()
            opt.step()
        return it, None

    def exact_native(lpips):
        vr, dec = fresh()
        state = {}

        def it():
            for t in dec.parameters().values():
                t.grad = None
            loss_of(vr.forward(ro, rd, bits, 128, dt_gamma=0.0), lpips).backward()
            dec.adam_step({k: t.grad for k, t in dec.parameters().items()}, state, lr=1e-2)
        return it, None

    last = {}

    def capacity(C, lpips, name):
        vr, dec = fresh()
        state = dec.adam_state()

        def it():
            for t in dec.parameters().values():
                t.grad = None
            o = vr.forward(ro, rd, bits, 128, dt_gamma=0.0, capacity=C)
            loss_of(o, lpips, o['n_samples']).backward()
            dec.adam_step({k: t.grad for k, t in dec.parameters().items()}, state, lr=1e-2, skip_if=o['overflow'])
            last[name] = (o['n_samples'], o['overflow'], state['step'])
            return o['n_samples'], o['overflow']
        return it, (dec, state)

    with torch.no_grad():
        vr0, _ = fresh()
        vr0.weight_culling_th = 0
        marched = vr0.forward(ro, rd, bits, 128, dt_gamma=0.0)['ts'][0].shape[0]
        vr0.weight_culling_th = 1e-3
        kept0 = vr0.forward(ro, rd, bits, 128, dt_gamma=0.0)['ts'][0].shape[0]
    C125, C2 = int(math.ceil(1.25 * marched)), 2 * marched
    variants = [('with LPIPS', 'exact (torch.optim.Adam)', exact(True)[0]),
                ('with LPIPS', 'exact (native Adam)', exact_native(True)[0]),
                ('with LPIPS', 'capacity 1.25x, eager', capacity(C125, True, 'e125')[0]),
                ('with LPIPS', 'capacity 2x, eager', capacity(C2, True, 'e2')[0]),
                ('without LPIPS', 'exact (torch.optim.Adam)', exact(False)[0]),
                ('without LPIPS', 'exact (native Adam)', exact_native(False)[0]),
                ('without LPIPS', 'capacity 1.25x, eager', capacity(C125, False, 'n125')[0]),
                ('without LPIPS', 'capacity 2x, eager', capacity(C2, False, 'n2')[0])]
    notes = ['graph replay: not measured']
    for _, _, fn in variants:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    final = {}
    for _ in range(args.repeats):
        for i, (_, _, fn) in enumerate(variants):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) / args.iters * 1e3)
            for name, (ns, ov, step) in last.items():                      # the window's own variant: read right after it
                final[name] = (ns.tolist(), int(ov), int(step))
            last.clear()
    counts = [launches(fn) for _, _, fn in variants]
    lines = [f'nerf_optim iteration, exact against capacity form: {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'128^2 rays, 128^3 grid, max_steps 512; marched {marched} samples, kept after culling at the start {kept0}; capacities {C125} (1.25x) and {C2} (2x)',
             f'{args.iters} iterations per window after {args.warmup} warm-up, {args.repeats} windows per variant, variants alternating in one process;',
             'host clock around the window with a closing device synchronise; ms per iteration: median (min .. max over the windows); launches = device',
             'activities of one iteration seen by torch.profiler', '']
    group = None
    for (grp, name, _), ts, n in zip(variants, times, counts):
        if grp != group:
            lines.append(f'[{grp}]')
            group = grp
        lines.append(f'  {name:32s} {statistics.median(ts):7.3f} ms  ({min(ts):.3f} .. {max(ts):.3f})   launches {n if n is not None else "not measured"}')
    lines += [''] + notes
    lines.append('state after the last window (n_samples = marched, kept after culling; the kept count falls as the fit proceeds):')
    for name, (ns, ov, step) in sorted(final.items()):
        lines.append(f'  {name:6s} n_samples {ns}, overflow {ov}, optimiser steps taken {step}')
    wrong = [name for name, (ns, ov, _) in final.items() if ns[0] != marched or ov != 0]
    lines.append('every capacity variant reports the exact path\'s marched total and no overflow' if not wrong
                 else f'MISMATCH: marched total / overflow of {wrong} differ from the exact path\'s {marched}')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
