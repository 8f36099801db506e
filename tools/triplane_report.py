"""Times the tri-plane decoders' dir-net kernels on the GPU (recorded, not asserted; no target exists) -> profiles/triplane_dirnet.txt

2^18 points at the SSDNeRF code size (3 x 6 x 128^2, no hash grid) and at the StableSSDNeRF size (3 x 16 x 80^2, 12-level hash grid):
forward and forward + backward of the dir-net kernels; next to them the default-topology kernels at C = 32 in the same process, and the
dir-net rule evaluated by torch in fp32 on the same GPU (F.grid_sample + Linears; the SH / hash encodings handed in precomputed, so it does
less).  Event timing after warm-up, REPS repetitions of ITERS back-to-back calls each; median and min..max of the per-call time.

    python tools/triplane_report.py [--out profiles/triplane_dirnet.txt]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvedit_amd.shencoder import SHEncoder  # noqa: E402
from mvedit_amd.triplane import TriPlaneDecoder, TriPlaneiNGPDecoder  # noqa: E402

N, WARM, REPS, ITERS = 1 << 18, 3, 7, 5


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / ITERS)
    return f'{statistics.median(ms):8.3f} ms  ({min(ms):.3f} .. {max(ms):.3f})'


def make(topology, C, H, ingp, g):
    r = lambda *s: torch.randn(*s, generator=g)
    xav = lambda o, i: (torch.rand(o, i, generator=g) * 2 - 1) * (6.0 / (i + o)) ** 0.5
    sd = {'base_net.0.weight': xav(H, 3 * C), 'base_net.0.bias': r(H) * 0.1, 'density_net.0.weight': xav(1, H), 'density_net.0.bias': r(1) * 0.1}
    if topology == 'dirnet':
        sd.update({'dir_net.0.weight': xav(H, 16), 'dir_net.0.bias': r(H) * 0.1, 'color_net.0.weight': xav(3, H), 'color_net.0.bias': r(3) * 0.1})
    else:
        sd.update({'color_net.0.weight': xav(H, H + 16), 'color_net.0.bias': r(H) * 0.1, 'color_net.2.weight': xav(3, H), 'color_net.2.bias': r(3) * 0.1})
    if ingp:
        dec = TriPlaneiNGPDecoder(n_levels=12)
        sd.update({'ingp_base_net.0.weight': xav(H, 24), 'ingp_base_net.0.bias': r(H) * 0.1,
                   'encoder.params': (torch.rand(dec.hash['rows'] * 2, generator=g) * 2 - 1) * 1e-2})
    else:
        dec = TriPlaneDecoder()
    return dec.load_state_dict(sd)


def torch_rule(dec, xyz, sh, code):
    """the dir-net rule in torch fp32 on the device (no hash branch: tiny-cuda-nn's encoding has no torch statement here)"""
    P = {k: v for k, v in dec.parameters().items()}
    grids = torch.stack([xyz[:, [0, 1]], xyz[:, [0, 2]], xyz[:, [1, 2]]], 0)[:, None]
    pc = F.grid_sample(code[0], grids, mode='bilinear', padding_mode='border', align_corners=False)
    feat = pc[:, :, 0].permute(2, 1, 0).reshape(xyz.shape[0], -1)
    base = F.linear(feat, P['base_net.0.weight'], P['base_net.0.bias'])
    sigma = torch.exp(F.linear(F.silu(base), P['density_net.0.weight'], P['density_net.0.bias']))[:, 0]
    z = base + F.linear(sh, P['dir_net.0.weight'], P['dir_net.0.bias'])
    return sigma, torch.sigmoid(F.linear(F.silu(z), P['color_net.0.weight'], P['color_net.0.bias']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'triplane_dirnet.txt'))
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    xyz = (torch.rand(N, 3, generator=g) * 2.2 - 1.1).cuda()
    dirs = F.normalize(torch.randn(N, 3, generator=g), dim=-1).cuda()
    g_sig, g_rgb = torch.randn(N, generator=g).cuda() * 0.1, torch.randn(N, 3, generator=g).cuda()
    lines = [f'tri-plane decoders, {N} points, {torch.cuda.get_device_name(0)}; median (min .. max) per call over {REPS} x {ITERS} calls after {WARM} warm-up calls',
             'measured once, untuned', '']
    rows = [('dir-net  SSDNeRF        C  6 128^2 H 64 no hash', 'dirnet', 6, 64, 128, False),
            ('dir-net  StableSSDNeRF  C 16  80^2 H 64 12-level hash', 'dirnet', 16, 64, 80, True),
            ('default  C 32 128^2 H 128 / 128 no hash', 'default', 32, 128, 128, False),
            ('default  C 32  80^2 H 128 / 128 12-level hash', 'default', 32, 128, 80, True)]
    for label, topo, C, H, hw, ingp in rows:
        dec = make(topo, C, H, ingp, g)
        code = torch.randn(1, 3, C, hw, hw, generator=g).cuda()
        lines.append(f'{label}\n    forward             {timed(lambda: dec.point_decode([xyz], [dirs], code))}')
        for p in dec.parameters().values():
            p.requires_grad_(True)

        def fwd_bwd():
            c = code.detach().requires_grad_(True)
            s, r, _ = dec.point_decode_autograd([xyz], [dirs], c)
            ((s * g_sig).sum() + (r * g_rgb).sum()).backward()
            for p in dec.parameters().values():
                p.grad = None
        lines.append(f'    forward + backward  {timed(fwd_bwd)}')
        if topo == 'dirnet' and not ingp:
            sh = SHEncoder(degree=4)(dirs).float()
            with torch.no_grad():
                lines.append(f'    torch fp32 rule, forward             {timed(lambda: torch_rule(dec, xyz, sh, code))}')

            def rule_fwd_bwd():
                c = code.detach().requires_grad_(True)
                s, r = torch_rule(dec, xyz, sh, c)
                ((s * g_sig).sum() + (r * g_rgb).sum()).backward()
                for p in dec.parameters().values():
                    p.grad = None
            lines.append(f'    torch fp32 rule, forward + backward  {timed(rule_fwd_bwd)}')
        for p in dec.parameters().values():
            p.requires_grad_(False)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
