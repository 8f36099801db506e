"""A/B of the UNet executor's CFG prefix (mve_unet_tune_cfg_prefix) on one GPU, one process: the benchmark's 64-image forward
(tools/bench_parts.make_passes) with the switch on and off, for the CFG batch as the pipeline builds it (identical halves: the prefix runs once),
for a batch whose halves differ in one element (the probe says no: the price of deciding on the device), and for the `use_reference` batch
(128 images, cross-image pairs).  Rounds alternate the variants; every figure is the median over the rounds of the mean of `--iters` forwards
between two HIP events, with the min - max spread next to it.  Outputs of on and off are compared bit for bit.

usage: python tools/cfg_prefix_ab.py [--rounds 5] [--iters 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
    import bench_parts as bp
    from mvedit_amd import synthetic
    from mvedit_amd.unet import SD15_CONFIG, UNet2DConditionEngine
    dev, dtype = torch.device('cuda:0'), torch.float16
    cfg = dict(SD15_CONFIG)
    eng = UNet2DConditionEngine.from_state_dict(synthetic.make_state_dict(cfg, seed=1234, dtype=dtype), cfg, dtype, dev)
    cases = {}
    for wl in ('mvedit', 'use_reference'):
        (x, t, ctx, n_img, kw), = bp.make_passes(wl, cfg, bp.VIEWS, 0, bp.VIEWS, bp.VIEWS, 1, dev, dtype)[0]
        cases[wl + ' identical halves'] = (x, t, ctx, n_img, kw, 1)
        if wl == 'mvedit':
            x2 = x.clone()
            x2[-1, -1, -1, -1] += 1.0
            cases[wl + ' distinct halves'] = (x2, t, ctx, n_img, kw, 0)

    def run(case, on, iters):
        x, t, ctx, n_img, kw, _ = case
        eng.set_cfg_prefix(on)
        eng._set_attention(kw, x.shape[0], x.shape[2], x.shape[3])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            out = eng._run(0, x, t, ctx, n_img, None, None, None)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters, out

    report = {}
    for name, case in cases.items():
        _, off = run(case, False, 1)
        _, on = run(case, True, 1)                           # (also the warm-up of both plans)
        state = eng.cfg_prefix_state()
        assert torch.equal(on, off), name + ': switch on and off differ'
        assert state == case[5], (name, state)
        ms = {True: [], False: []}
        for r in range(a.rounds):
            for on_ in ((False, True) if r % 2 == 0 else (True, False)):
                ms[on_].append(run(case, on_, a.iters)[0])
        med = {k: statistics.median(v) for k, v in ms.items()}
        report[name] = dict(images=int(case[0].shape[0]), state=state, bit_identical=True,
                            off_ms=[round(v, 3) for v in ms[False]], on_ms=[round(v, 3) for v in ms[True]],
                            off_median=round(med[False], 3), on_median=round(med[True], 3), gain_ms=round(med[False] - med[True], 3),
                            off_spread=round(max(ms[False]) - min(ms[False]), 3), on_spread=round(max(ms[True]) - min(ms[True]), 3))
        print(name, json.dumps(report[name]), flush=True)
    print(json.dumps(report))


if __name__ == '__main__':
    main()
