"""One timing of the native LoFTR matcher, with no target: the full-size network (`default_cfg`: ResNetFPN_8_2, 8 coarse and 2 fine linear-attention
layers) on `LoFTREngine` with seeded synthetic fp16 weights, one 480 x 480 pair (3600 coarse tokens) -- the shape `elev_estimation` /
`pose5dof_estimation` run six times per request.  Seeded weights find no match at this size, so the fine stage is timed on 1024 forced matches.
Device events around windows of at least half a second after a warm-up, three windows, the
median reported; the launch count and the split over backbone / coarse transformer / matching / fine stage come from the plans
(`mve_unet_op_info`) and one profiled forward (events around every op, so launch gaps are included).  The forward includes its one host read
(the match count).  The reference's torch LoFTR needs `yacs` and `kornia`, which are not installed beside the GPU: it is not timed.  Measured once,
untuned.

    python tools/loftr_report.py [--out profiles/loftr.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvedit_amd.matcher import LoFTREngine, key_table  # noqa: E402
from tools.clip_text_report import windows  # noqa: E402


def synthetic_state_dict(seed=0):
    """The reference's initialisers (kaiming fan-out convolutions, xavier-uniform matrices) with mildly perturbed norms; the coarse norm2 gain
    is centred on 3 and FinePreprocess' matrices are scaled down, as in tests/golden/make_loftr_golden.py (matches exist, fp16 stays finite)."""
    shapes = {'backbone.conv1.weight': (128, 1, 7, 7)}
    dims, cin = (128, 196, 256), 128
    for li, c in enumerate(dims, 1):
        for b in (0, 1):
            shapes[f'backbone.layer{li}.{b}.conv1.weight'] = (c, cin if b == 0 else c, 3, 3)
            shapes[f'backbone.layer{li}.{b}.conv2.weight'] = (c, c, 3, 3)
            if b == 0 and li > 1:
                shapes[f'backbone.layer{li}.{b}.downsample.0.weight'] = (c, cin, 1, 1)
        cin = c
    shapes.update({'backbone.layer3_outconv.weight': (256, 256, 1, 1), 'backbone.layer2_outconv.weight': (256, 196, 1, 1),
                   'backbone.layer2_outconv2.0.weight': (256, 256, 3, 3), 'backbone.layer2_outconv2.3.weight': (196, 256, 3, 3),
                   'backbone.layer1_outconv.weight': (196, 128, 1, 1), 'backbone.layer1_outconv2.0.weight': (196, 196, 3, 3),
                   'backbone.layer1_outconv2.3.weight': (128, 196, 3, 3)})
    rs, sd = np.random.RandomState(seed), {}
    for key in key_table().values():
        leaf = key.rsplit('.', 1)[1]
        if key in shapes:
            s = shapes[key]
            v = (2.0 / (s[0] * s[2] * s[3])) ** 0.5 * rs.standard_normal(s)
        elif leaf == 'num_batches_tracked':
            v = np.asarray(1)
        elif 'bn' in key or 'downsample.1' in key or 'outconv2.1' in key:
            c = shapes[key.rsplit('.', 1)[0].replace('bn1', 'conv1').replace('bn2', 'conv2').replace('downsample.1', 'downsample.0').replace('outconv2.1', 'outconv2.0') + '.weight'][0]
            v = {'weight': 1 + 0.1 * rs.standard_normal(c), 'bias': 0.05 * rs.standard_normal(c), 'running_mean': 0.1 * rs.standard_normal(c),
                 'running_var': 0.6 + 0.8 * rs.random_sample(c)}[leaf]
        else:
            d = 256 if 'loftr_coarse' in key else 128
            if 'norm' in key:
                v = (3.0 if 'loftr_coarse' in key and 'norm2.weight' in key else 1.0 if leaf == 'weight' else 0.0) + (0.1 if leaf == 'weight' else 0.05) * rs.standard_normal(d)
            elif key.startswith('fine_preprocess'):
                s = {'down_proj.weight': (128, 256), 'merge_feat.weight': (128, 256)}.get(key.split('.', 1)[1])
                v = (0.1 if 'down_proj' in key else 0.25) * (2.0 / 128) ** 0.5 * rs.standard_normal(s) if s else 0.05 * rs.standard_normal(128)
            else:
                s = {'mlp.0': (2 * d, 2 * d), 'mlp.2': (d, 2 * d)}.get(key.split('.', 3)[3].rsplit('.', 1)[0], (d, d))
                v = (6.0 / (s[0] + s[1])) ** 0.5 * (2 * rs.random_sample(s) - 1)
        sd[key] = torch.from_numpy(np.asarray(v))
    return sd


def smooth_pair(H, W, seed=1):
    f = torch.randn(1, 1, H + 40, W + 40, generator=torch.Generator().manual_seed(seed))
    k = torch.exp(-0.5 * (torch.arange(-6, 7).float() / 2) ** 2)
    k = (k / k.sum())
    f = torch.nn.functional.conv2d(torch.nn.functional.conv2d(f, k.view(1, 1, -1, 1), padding=(6, 0)), k.view(1, 1, 1, -1), padding=(0, 6))
    f = (f - f.min()) / (f.max() - f.min())
    return f[..., 16:16 + H, 16:16 + W].contiguous(), f[..., 8:8 + H, 8:8 + W].contiguous()


def split(tables):
    """milliseconds of one profiled forward by stage, from the op labels of the two plans"""
    out = dict(backbone=0.0, transformer=0.0, matching=0.0, fine=0.0)
    (ct, cms), fine = tables[0], tables[1:]
    stage = 'backbone'
    for (_, _, lab), ms in zip(ct, cms):
        if lab.endswith('-> tap'):
            continue
        if lab == 'position add':
            stage = 'transformer'
        if lab == 'similarity':
            stage = 'matching'
        out[stage] += ms
    for ft, fms in fine:
        out['fine'] += sum(ms for (_, _, lab), ms in zip(ft, fms) if not lab.endswith('-> tap'))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loftr.txt'))
    ap.add_argument('--size', type=int, default=480)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('loftr_report needs the GPU: nothing is measured without one')
    torch.set_grad_enabled(False)
    eng = LoFTREngine(None, torch.float16, 'cuda').load_state_dict(synthetic_state_dict())
    S = args.size
    im0, im1 = (t.half().cuda() for t in smooth_pair(S, S))
    out = eng.run(im0, im1)
    M = int(out['b_ids'].shape[0])
    ci = eng.plan(1, S, S, 1)
    ctab = eng.op_table()
    fi = eng.plan(1, S, S, 2)
    ftab = eng.op_table()
    launches = [sum(not lab.endswith('-> tap') for _, _, lab in t) for t in (ctab, ftab)]
    # Seeded weights find no match among 3600 cells (the dual softmax is flat), so the fine stage would never run: it is timed on FORCED matches,
    # cell i of image 0 to cell i of image 1 for the first 1024 cells outside the 2-cell border -- a count a textured 480 x 480 pair gives.
    G = S // 8
    cells = torch.tensor([y * G + x for y in range(2, G - 2) for x in range(2, G - 2)][:1024])
    forced = (torch.zeros_like(cells).cuda(), cells.cuda(), cells.cuda())
    (t, reps) = windows([lambda: eng.run(im0, im1), lambda: eng.run(im0, im1, coarse_matches=forced)])
    st = split(eng.run(im0, im1, coarse_matches=forced, profile=True)[-1])
    again = eng.run(im0, im1)
    same = torch.equal(out['mkpts1_f'], again['mkpts1_f']) and torch.equal(out['conf_matrix'], again['conf_matrix'])
    lines = [f'# tools/loftr_report.py on {torch.cuda.get_device_name(0)}: LoFTR (default_cfg: ResNetFPN_8_2, 8 coarse + 2 fine linear-attention layers), fp16, synthetic '
             f'weights, one {S} x {S} pair ({(S // 8) ** 2} coarse tokens); measured once, untuned',
             f'plans: coarse {ci["n_ops"]} ops / {launches[0]} launch ops, workspace {ci["workspace_bytes"]} bytes; fine {fi["n_ops"]} ops / {launches[1]} launch ops, '
             f'workspace {fi["workspace_bytes"]} bytes (planned for {(S // 8) ** 2} matches); tap copies are made only with output_features=True',
             f'matches of this pair: {M}; conf_matrix fp32 [1, {(S // 8) ** 2}, {(S // 8) ** 2}] = {4 * (S // 8) ** 4} bytes; two forwards bit-identical: {same}',
             f'engine forward as called (coarse call, the one host read, no fine call: 0 matches), Python call to last kernel, device events: {t[0] * 1e3:.4f} ms  '
             f'(median of 3 windows of {reps[0]} calls, >= 0.5 s each)',
             f'engine forward with {len(cells)} forced matches (coarse call, id checks on the host, fine call): {t[1] * 1e3:.4f} ms  (median of 3 windows of {reps[1]} calls)',
             f'device time of one profiled forward with {len(cells)} forced matches by stage (events around every op, so launch gaps are included), ms: '
             + ', '.join(f'{k} {v:.4f}' for k, v in st.items()) + f', sum {sum(st.values()):.4f}',
             f'flops of the coarse plan: conv {ci["flops"]["conv"]:.4g}, linear {ci["flops"]["linear"]:.4g}, linear attention {ci["flops"]["attention"]:.4g}',
             "the reference's torch LoFTR is not timed: `yacs` and `kornia` are not installed beside the GPU"]
    print('\n'.join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
