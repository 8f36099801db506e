"""The CPU statement of rendering a tri-plane scene, for tests/test_triplane_render.py: the eval loop and the training forward of
oracle/nerf_oracle.py (render_rays_eval :125-150, train_forward :265-277) with a decode that also receives the DIRECTIONS `ORM.march_rays` /
`ORM.march_rays_train` return -- the oracle's own `decode=` hook drops them, and a tri-plane decoder's colour depends on them.  Marching
and compositing are the pinned C restatement (oracle/raymarching.py); the decode is the pinned rule (tests/triplane_dirnet_rule.py for the
dir-net topology, oracle/triplane_oracle.py for the default one): nothing new is stated about the decoders.  For gradients:
`composite_rays_train_torch`, kernel_composite_rays_train_forward in differentiable torch (float64 capable)."""
import numpy as np
import torch

from oracle import nerf_oracle as NO
from oracle import raymarching as ORM


def render_rays_eval(rays_o, rays_d, bitfield, grid_size, decode, bound=1.0, min_near=0.2, dt_gamma=0.0, max_steps=1024, T_thresh=1e-2,
                     trace=False):
    """NO.render_rays_eval with decode(xyzs, dirs) -> (sigmas, rgbs).  -> weights_sum, depth, image, n_samples[, trace].
    trace (per ray, restated in float32 numpy next to ORM.composite_rays, which stays the source of the outputs): `counts`, the samples the
    ray composited; `stopped`, whether it ended by T < T_thresh; `margin`, min over its samples of |T - T_thresh| / T_thresh for the
    transmittance T the stop rule tests (1 - weights_sum before the sample is added)."""
    rays_o = np.ascontiguousarray(rays_o, np.float32).reshape(-1, 3)
    rays_d = np.ascontiguousarray(rays_d, np.float32).reshape(-1, 3)
    N = rays_o.shape[0]
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    nears, fars = ORM.near_far_from_aabb(rays_o, rays_d, aabb, min_near)
    weights_sum, depth, image = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, 3), np.float32)
    rays_alive = np.arange(N, dtype=np.int32)
    rays_t = nears.copy()
    counts, stopped, margin = np.zeros(N, np.int64), np.zeros(N, bool), np.full(N, np.inf)
    step = 0
    n_samples = 0
    while step < max_steps:
        n_alive = rays_alive.shape[0]
        if n_alive == 0:
            break
        n_step = min(max(N // n_alive, 1), 8)
        xyzs, dirs, ts = ORM.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, bitfield, 1, grid_size,
                                        nears, fars, np.zeros(n_alive, np.float32), dt_gamma, max_steps)
        n_samples += int((ts[:, 0] != 0).sum())
        sigmas, rgbs = decode(xyzs, dirs)
        sigmas, rgbs = np.ascontiguousarray(sigmas, np.float32), np.ascontiguousarray(rgbs, np.float32)
        if trace:
            sg, dt = sigmas.reshape(n_alive, n_step), ts[:, 1].reshape(n_alive, n_step)
            ws = weights_sum[rays_alive].copy()
            active = np.ones(n_alive, bool)
            for s in range(n_step):
                active = active & (dt[:, s] != 0)
                alpha = np.float32(1) - np.exp(-sg[:, s] * dt[:, s]).astype(np.float32)
                T = np.float32(1) - ws
                ids = rays_alive[active]
                margin[ids] = np.minimum(margin[ids], np.abs(T[active].astype(np.float64) - T_thresh) / T_thresh)
                counts[ids] += 1
                ws = np.where(active, ws + alpha * T, ws).astype(np.float32)
                stop = active & (T < np.float32(T_thresh))
                stopped[rays_alive[stop]] = True
                active = active & ~stop
        ORM.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image, T_thresh)
        rays_alive = np.ascontiguousarray(rays_alive[rays_alive >= 0])
        step += n_step
    if trace:
        return weights_sum, depth, image, n_samples, dict(counts=counts, stopped=stopped, margin=margin)
    return weights_sum, depth, image, n_samples


def train_forward(rays_o, rays_d, bitfield, grid_size, decode, noises, dt_gamma=0.0, bound=1.0, min_near=0.2, max_steps=1024,
                  weight_culling_th=1e-3):
    """NO.train_forward with decode(xyzs, dirs) -> (sigmas, rgbs) (the culling pass uses its sigmas only)."""
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    nears, fars = ORM.near_far_from_aabb(rays_o, rays_d, aabb, min_near)
    xyzs, dirs, ts, rays = ORM.march_rays_train(rays_o, rays_d, bound, bitfield, 1, grid_size, nears, fars, noises, dt_gamma, max_steps)
    if weight_culling_th > 0:
        sig, _ = decode(xyzs, dirs)
        w, _, _, _ = ORM.composite_rays_train(sig, np.zeros((sig.shape[0], 3), np.float32), ts, rays)
        xyzs, dirs, ts, rays, _ = NO.cull_samples(w, weight_culling_th, xyzs, dirs, ts, rays)
    sig, rgb = decode(xyzs, dirs)
    weights, ws, depth, image = ORM.composite_rays_train(sig, rgb, ts, rays)
    return dict(weights=weights, weights_sum=ws, depth=depth, image=image, rays=rays, ts=ts, xyzs=xyzs, dirs=dirs)


def composite_rays_train_torch(sigmas, rgbs, ts, rays, T_thresh=1e-4):
    """kernel_composite_rays_train_forward (oracle/raymarching_oracle.c:238-268) in differentiable torch: per ray, alpha_k = 1 - exp(-sigma_k
    dt_k), T_k = prod_{i<k} (1 - alpha_i) (cumulative transmittance), w_k = alpha_k T_k for the samples up to and including the first whose
    T_{k+1} < T_thresh (that cut is a constant of the differentiation, as in the kernel's backward).  sigmas [M], rgbs [M,3] torch (any float
    dtype); ts [M,2], rays [N,2] numpy -> weights [M], weights_sum [N], depth [N], image [N,3]."""
    dt_, M = sigmas.dtype, sigmas.shape[0]
    ray_of = np.full(M, -1, np.int64)
    first = np.zeros(M, bool)
    for n, (off, cnt) in enumerate(np.asarray(rays, np.int64)):
        ray_of[off:off + cnt] = n
        if cnt:
            first[off] = True
    assert (ray_of >= 0).all(), 'every sample belongs to a ray'
    t_mid, dts = torch.from_numpy(np.asarray(ts[:, 0], np.float64)).to(dt_), torch.from_numpy(np.asarray(ts[:, 1], np.float64)).to(dt_)
    alpha = 1 - torch.exp(-sigmas * dts)
    # exclusive cumulative product inside each ray, by cumulative sums of log(1 - alpha) restarted at each ray's first sample
    la = torch.log1p(-alpha.clamp(max=1 - 1e-300 if dt_ == torch.float64 else 1 - 1e-7))
    cs = torch.cumsum(la, 0) - la
    start = cs[torch.from_numpy(np.maximum.accumulate(np.where(first, np.arange(M), 0)))]
    T = torch.exp(cs - start)
    keep = (T.detach() >= T_thresh)                  # sample k is reached iff the transmittance after sample k - 1 is not below the threshold
    w = alpha * T * keep
    idx = torch.from_numpy(ray_of)
    N = len(rays)
    ws = torch.zeros(N, dtype=dt_).index_add(0, idx, w)
    depth = torch.zeros(N, dtype=dt_).index_add(0, idx, w / t_mid)
    image = torch.zeros(N, 3, dtype=dt_).index_add(0, idx, w[:, None] * rgbs)
    return w, ws, depth, image
