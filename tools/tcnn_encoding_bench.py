"""Times mvedit_amd.tinycudann.Encoding's kernels (csrc/hashgrid_encode.hip) at the reference's default config (12 levels, 320, F = 2,
Smoothstep), with the fused decoder kernels of csrc/nerf.hip beside them as a yardstick:

  * ray-ordered samples of a real march of the test scene (the nerf_optim batch of tools/optim_profile.py: 128 x 128 rays, 512 steps)
  * 2^20 uniform points in the unit cube (no two neighbours in one cell of a fine level)

forward = mve_hashgrid_encode; fwd + bwd(params) adds the zeroing of the table gradient and mve_hashgrid_encode_backward without d/dx;
fused = mve_hashgrid_mlp_decode / mve_hashgrid_mlp_backward (encoding + 24 -> 64 -> 4 MLP + heads, forward recomputed in the backward).
Device-event times, mean of K launches after warm-up.  python tools/tcnn_encoding_bench.py [K]"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from scene import sphere_density_grid  # noqa: E402
from mvedit_amd import nerf, raymarching as rm  # noqa: E402
from mvedit_amd.tinycudann import Encoding  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device('cuda:0')
torch.cuda.set_device(dev)
g = torch.Generator().manual_seed(11)


def ray_ordered_samples():
    bits = rm.packbits(torch.from_numpy(sphere_density_grid(128, radius=0.5)).to(dev), 0.5)
    S, ps = 512, 128
    fl = S / (2 * math.tan(math.radians(15)))
    intr = torch.tensor([[fl, fl, S / 2, S / 2]], device=dev)
    c = torch.tensor([3.7 * math.cos(0.2), 0.0, 3.7 * math.sin(0.2)])
    fwd = -c / c.norm()
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]))
    right = right / right.norm()
    down = torch.linalg.cross(fwd, right)
    pose = torch.zeros(1, 3, 4)
    pose[0, :, 0], pose[0, :, 1], pose[0, :, 2], pose[0, :, 3] = right, down, fwd, c
    ro, rd, _ = nerf.camera_rays(intr * (ps / S), pose.to(dev), ps, ps)
    aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32, device=dev)
    nears, fars = rm.near_far_from_aabb(ro, rd, aabb, 0.2)
    xyzs, _, _, _ = rm.march_rays_train(ro, rd, 1.0, bits, 1, 128, nears, fars, dt_gamma=0.0, max_steps=512)
    return xyzs.contiguous()


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(K):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / K


cfg = {"otype": "HashGrid", "n_levels": 12, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
       "interpolation": "Smoothstep", "per_level_scale": float(2 ** (math.log2(320 / 16) / 11))}
enc = Encoding(3, cfg, dtype=torch.float32).to(dev)
with torch.no_grad():
    enc.params.copy_(((torch.rand(enc.params.numel(), generator=g) * 2 - 1) * 0.1).to(dev))
table = enc.params.detach().reshape(-1, 2)
w1 = (torch.rand(64, 24, generator=g) * 2 - 1) * math.sqrt(6 / (64 + 24))
w2 = (torch.rand(4, 64, generator=g) * 2 - 1) * math.sqrt(6 / (4 + 64))
dec = nerf.INGPDecoderParams(table, w1, torch.zeros(64), w2, torch.tensor([2.0, 0.0, 0.0, 0.0]), 12, 320, device=dev)
print(f'table {enc.n_rows} rows x 2 = {enc.n_rows * 8 / 1e6:.1f} MB; K = {K}', flush=True)

for name, xyz in (('ray-ordered march', ray_ordered_samples()), ('uniform 2^20', (torch.rand(1 << 20, 3, generator=g) * 2 - 1).to(dev))):
    M = xyz.shape[0]
    x01 = ((xyz + 1) / 2).contiguous()
    out = torch.empty(M, 24, device=dev)
    genc = torch.randn(M, 24, generator=g).to(dev)
    gtab = torch.zeros_like(enc.params)
    gs, gr = torch.randn(M, generator=g).to(dev), torch.randn(M, 3, generator=g).to(dev)
    grads = {k: torch.zeros_like(v) for k, v in dec.parameters().items()}
    p = enc.params.detach()

    def fwd_only():
        out.copy_(enc._launch_forward(x01, p))

    def fwd_bwd():
        enc._launch_forward(x01, p)
        gtab.zero_()
        enc._launch_backward(x01, p, genc, gtab, None)

    def bwd_x():
        enc._launch_backward(x01, p, genc, gtab, torch.empty_like(x01))

    def autograd_step():
        enc.params.grad = None
        enc(x01).backward(genc)

    t_f = timed(lambda: enc._launch_forward(x01, p))
    t_fb = timed(fwd_bwd)
    t_bx = timed(bwd_x)
    t_ag = timed(autograd_step)
    t_df = timed(lambda: dec.point_decode(xyz))
    t_db = timed(lambda: dec.point_decode_backward(xyz, gs, gr, grads))
    print(f'{name}: {M} samples', flush=True)
    print(f'  encode forward                          {t_f:.3f} ms', flush=True)
    print(f'  encode forward + zero grad + backward   {t_fb:.3f} ms   (target <= 0.6 ms at the ray-ordered batch)', flush=True)
    print(f'  encode backward with d/dx               {t_bx:.3f} ms', flush=True)
    print(f'  Encoding autograd fwd + .backward()     {t_ag:.3f} ms', flush=True)
    print(f'  fused decode forward (yardstick)        {t_df:.3f} ms', flush=True)
    print(f'  fused decode backward (yardstick)       {t_db:.3f} ms', flush=True)
