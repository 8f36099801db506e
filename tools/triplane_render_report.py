"""Times the fused tri-plane render against the reference-shaped host loop on the GPU and tabulates the kernels' resource usage
(recorded, not asserted; measured once, untuned, no target exists) -> profiles/triplane_render.txt

    python tools/triplane_render_report.py timing     [--out profiles/triplane_render.txt]      (GPU)
    python tools/triplane_render_report.py resources  [--out ...] [--remarks hipcc_stderr.txt]  (no GPU: compiles csrc/triplane.hip with
                                                                                                 -Rpass-analysis=kernel-resource-usage)

timing: 6 views at 128^2 (tests/scene.py's cameras, distance 3.7, fov 30 deg) of a seeded dir-net scene inside a spherical bitfield (128^3,
radius 0.5), max_steps 1024, dt_gamma = 2 / (fx + fy) (what dt_gamma_scale=1.0 gives), at the SSDNeRF code size (3 x 6 x 128^2, H 64, no hash
grid) and the StableSSDNeRF size (3 x 16 x 80^2, 12-level hash grid, H 64): ms of `render_rays(fused=True)` (one launch) and of
`render_rays(fused=False)` (the reference's loop on the repository's own march_rays / point_decode / composite_rays / compact_alive, one host
read per chunk) on the same inputs; samples per ray.  Event timing after warm-up; median and min..max over REPS repetitions.
Each section of the output file is rewritten by its own sub-command; the other one is kept."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
MARK = '==== resource usage '
WARM, REPS = 2, 5


def timing():
    import numpy as np
    import torch
    from mvedit_amd import raymarching as rm
    from scene import camera_rays, sphere_density_grid
    from triplane_report import make

    def timed(fn):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), f'{statistics.median(ms):9.3f} ms  ({min(ms):.3f} .. {max(ms):.3f})'

    S, V, GRID = 128, 6, 128
    o, d = camera_rays(V, S, jitter=False)
    o, d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    bits = rm.packbits(torch.from_numpy(sphere_density_grid(GRID, radius=0.5)).cuda(), 0.5).reshape(-1)
    f = S / (2 * np.tan(np.deg2rad(30.0) / 2))
    dt_gamma = 2.0 / (2 * f)
    g = torch.Generator().manual_seed(0)
    lines = [f'tri-plane render, {V} views at {S}^2 = {o.shape[0]} rays, bitfield {GRID}^3 sphere r 0.5, max_steps 1024, dt_gamma {dt_gamma:.5f}, '
             f'{torch.cuda.get_device_name(0)}',
             f'median (min .. max) of {REPS} calls after {WARM} warm-up calls; measured once, untuned', '']
    for label, C, hw, ingp in (('dir-net  SSDNeRF        C  6 128^2 H 64 no hash', 6, 128, False),
                               ('dir-net  StableSSDNeRF  C 16  80^2 H 64 12-level hash', 16, 80, True)):
        dec = make('dirnet', C, 64, ingp, g)
        dec.params['density_net.0.bias'].add_(2.0)            # some rays saturate, some leave the sphere unsaturated
        dec.max_steps = 1024
        code = torch.randn(1, 3, C, hw, hw, generator=g).cuda()
        ws, _, img, cnt = dec.render_rays(o, d, code, bits, GRID, dt_gamma, return_counts=True)
        ws_l, _, img_l, cnt_l = dec.render_rays(o, d, code, bits, GRID, dt_gamma, return_counts=True, fused=False)
        hit = cnt > 0
        t_f, s_f = timed(lambda: dec.render_rays(o, d, code, bits, GRID, dt_gamma))
        t_l, s_l = timed(lambda: dec.render_rays(o, d, code, bits, GRID, dt_gamma, fused=False))
        lines += [label,
                  f'    rays that hit {int(hit.sum())} ({hit.float().mean().item():.3f}); samples decoded {int(cnt.sum())} fused / {int(cnt_l.sum())} loop '
                  f'(marched in whole chunks); per hit ray mean {cnt[hit].float().mean().item():.1f} max {int(cnt.max())}; '
                  f'saturated (ws > 0.99) {(ws[hit] > 0.99).float().mean().item():.3f} of the hit rays',
                  f'    max |fused - loop|: ws {(ws - ws_l).abs().max().item():.2e} image {(img - img_l).abs().max().item():.2e}',
                  f'    fused launch    {s_f}',
                  f'    host loop       {s_l}',
                  f'    loop / fused    {t_l / t_f:.2f}x', '']
    return '\n'.join(lines)


def resources(remarks):
    if remarks is None:
        from mvedit_amd import build as B
        src = os.path.join(B.CSRC, 'triplane.hip')
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [B._hipcc()] + B.COMMON_FLAGS + B.EXTRA_FLAGS['triplane.hip'] + ['-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', os.path.join(tmp, 't.o')]
            text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    else:
        text = open(remarks).read()
    rows = []
    for blk in re.split(r'remark: [^\n]*Function Name: ', text)[1:]:
        m = re.match(r'\S*k_triplane_render_raysILi(\d)ELi(\d+)ELi(\d+)ELi(\d+)E', blk)
        if not m:
            continue
        num = lambda k: int(re.search(re.escape(k) + r': (\d+)', blk).group(1))
        topo, H, H2, NL = (int(v) for v in m.groups())
        lds = num('LDS Size [bytes/block]')
        rows.append((topo, H, H2, NL, num('VGPRs'), num('AGPRs'), num('ScratchSize [bytes/lane]'), lds, num('Occupancy [waves/SIMD]'), (160 * 1024) // lds))
    rows.sort(key=lambda r: (-r[0], r[1], r[2], r[3]))
    out = [MARK + '(hipcc -Rpass-analysis=kernel-resource-usage, gfx950): k_triplane_render_rays, one wave per block ====',
           'topology  H   H2   NL  VGPRs AGPRs  scratch B/lane  LDS B/block  waves/SIMD (registers)  blocks/CU (LDS, 160 KiB)  waves/CU']
    for topo, H, H2, NL, v, a, sc, lds, occ, blk in rows:
        out.append(f'{"dir-net" if topo else "default":8s} {H:3d} {"-" if topo else H2:>4} {NL:4d} {v:6d} {a:5d} {sc:15d} {lds:12d} {occ:22d} {blk:25d} {min(4 * occ, blk):9d}')
    spill = [r for r in rows if r[6] > 0]
    out.append(f'{len(spill)} of {len(rows)} instantiations spill to scratch.  waves/CU = min(4 x waves/SIMD, blocks/CU): what is resident.')
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('part', choices=['timing', 'resources'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'triplane_render.txt'))
    ap.add_argument('--remarks', default=None, help='a saved stderr of the hipcc line above instead of compiling again')
    args = ap.parse_args()
    old = open(args.out).read() if os.path.exists(args.out) else ''
    head, _, tail = old.partition(MARK)
    tail = (MARK + tail) if tail else ''
    if args.part == 'timing':
        head = timing() + '\n'
    else:
        tail = resources(args.remarks) + '\n'
    text = head + tail
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
