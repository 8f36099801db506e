"""One mesh_optim iteration with the DMTet call inside (lib/pipelines/mvedit_3d_pipeline.py:745-847, :828), exact form against capacity
form, at a production-like size: the 128^3 tetrahedral grid of the reference's DMTet stage and 6 views at 512^2 (tools/bench_parts.py's
mesh_iter, which leaves the DMTet call out).  Both forms run in this one process on the same binary; device-event times, one window
each, measured once, untuned.  Writes profiles/mesh_optim_capacity.txt.

    python tools/mesh_optim_capacity_report.py [iterations per window, default 20] [output file]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from mvedit_amd.mesh_ops import DMTet, Mesh, MeshRenderer, adam_step_n, mesh_regularizers  # noqa: E402
from mvedit_amd.recon_loss import mesh_optim_loss  # noqa: E402
from scene import blob_sdf, icosphere, tet_grid  # noqa: E402

N_GRID, S, NV, LR = 128, 512, 6, 1e-3


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = 'cuda'
    pos_np, tets_np = tet_grid(N_GRID)
    pos, tets = torch.from_numpy(pos_np).to(dev), torch.from_numpy(tets_np).to(dev)
    sdf0 = torch.from_numpy(blob_sdf(pos_np, 0, noise=0.0)).to(dev)
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_py.npz'))
    poses = torch.from_numpy(gold['poses'][:NV, :3].astype(np.float32)).to(dev)
    fl = S / (2 * np.tan(np.deg2rad(15)))
    intr = torch.tensor([[fl, fl, S / 2, S / 2]], dtype=torch.float32).repeat(NV, 1).to(dev)
    mr = MeshRenderer(near=0.01, far=100)
    vc = lambda v: torch.cat([torch.full_like(v, 0.7), torch.ones_like(v[:, :1])], -1)
    # targets: the render of a larger sphere
    v0, f0 = icosphere(5, 0.7)
    v0, f0 = torch.from_numpy(v0).to(dev), torch.from_numpy(f0).to(dev)
    with torch.no_grad():
        m = Mesh(v0, f0, vc=vc(v0))
        m.auto_normal()
        o = mr([m], poses[None], intr[None], S, S)
    tgt_m = o['rgba'][0][..., 3:].contiguous()
    tgt_rgb = (o['rgba'][0][..., :3] / tgt_m.clamp(min=1e-3)).contiguous()
    tgt_n = o['normal'][0].contiguous()
    erode = -torch.nn.functional.max_pool2d(-tgt_m.permute(0, 3, 1, 2), 5, stride=1, padding=2).permute(0, 2, 3, 1).contiguous()
    ys, xs = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing='ij')
    dirs = torch.stack([(xs + 0.5 - S / 2) / fl, (ys + 0.5 - S / 2) / fl, torch.ones_like(xs)], -1)[None].repeat(NV, 1, 1, 1).to(dev).contiguous()
    view_w = torch.ones(NV, device=dev)

    def make(capacity):
        sdf, deform, state, dm = sdf0.clone().requires_grad_(True), torch.zeros_like(pos).requires_grad_(True), {}, DMTet(dev)

        def it():
            sdf.grad = deform.grad = None
            if capacity is None:
                v, f = dm(pos + deform, sdf, tets)
                live, skip = None, None
            else:
                v, f = dm(pos + deform, sdf, tets, capacity=capacity)
                live, skip = dm.live, dm.overflow
            m = Mesh(v, f, vc=vc(v), live=live)
            m.auto_normal()
            out = mr([m], poses[None], intr[None], S, S)
            res = mesh_optim_loss(out['rgba'][0], out['normal'][0], out['depth'][0].detach(), tgt_rgb, erode, tgt_m, dirs, view_w, target_n=tgt_n,
                                  normal_reg_weight=1.0)
            lap, nc = mesh_regularizers(v, f, m.face_normals, live=live)
            (res['loss'] + 5.0 * (lap + nc)).backward()
            adam_step_n([sdf, deform], [sdf.grad, deform.grad], state, lr=LR, skip_if=skip)
            return res['loss'].detach()
        return it, dm, state

    probe = DMTet(dev)
    v, f = probe(pos, sdf0, tets)
    nv, nf = v.shape[0], f.shape[0]
    variants = [('exact (one host read per iteration)', None), ('capacity 1.25x', (int(nv * 1.25), int(nf * 1.25))), ('capacity 2x', (2 * nv, 2 * nf)),
                ('exact, a second time', None)]
    lines = [f'mesh_optim iteration with its DMTet call, exact against capacity form: {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'{N_GRID}^3 tet grid ({pos.shape[0]} vertices, {tets.shape[0]} tets), mesh at the start {nv} vertices / {nf} faces, {NV} views at {S}^2, '
             f'vertex colours, no LPIPS term, native Adam with device state on tet_sdf and deform in both forms',
             f'{iters} iterations in ONE window per variant after 3 warm-up iterations, device events around the window, variants one after the other '
             f'in one process; measured once, untuned; launches = device activities of one iteration seen by torch.profiler', '']
    for name, cap in variants:
        it, dm, state = make(cap)
        for _ in range(3):
            it()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            loss = it()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            it()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        tail = '' if cap is None else f'   counts {dm.counts.tolist()} live {dm.live.tolist()} overflow {dm.overflow.tolist()}'
        lines.append(f'  {name:38s} {ms:8.3f} ms per iteration   launches {launches:4d}   loss after the last step {float(loss):.6f}   steps {state["step"].tolist()[0]}{tail}')
        print(lines[-1], flush=True)
    lines += ['', 'the loss and the counts after the last step show how far the runs drift apart from one start: the gradients pass through float atomics in',
              'both forms and Adam turns their rounding into steps of size lr wherever a gradient nearly cancels (the two exact runs differ from each',
              'other as well); the first iteration is compared bit for bit in tests/test_mesh_capacity_gpu.py']
    lines += ['', 'graph replay: not measured (the capture of the iteration is out of scope; the NeRF replay fault of DESIGN.md section 7d item 5 is open)']
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'mesh_optim_capacity.txt')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    text = '\n'.join(lines) + '\n'
    with open(path, 'w') as fh:
        fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
