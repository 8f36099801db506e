"""The arithmetic of the tri-plane decoders' dir-net topology (the one every reference config asks for: `dir_layers=[16, H]`,
`color_layers=[H, 3]`), stated in differentiable torch, float64 capable -- the rule csrc/triplane.hip's dir-net kernels and
mvedit_amd.triplane are held to (tests/test_triplane_dirnet.py), itself held against the reference's own `point_decode` EXECUTED
(tests/golden/triplane_dirnet_ref.npz, tests/golden/make_triplane_dirnet_golden.py).

    feat[n, c * 3 + p] = bilinear grid_sample(border padding, align_corners=False) of channel c of plane p at the point's two plane coordinates
    base_x = feat @ base_w^T + base_b  [+ enc @ ingp_w^T + ingp_b,  enc = HashGrid((xyz + bound) / (2 bound))]
    sigma  = exp(act(base_x) @ dens_w^T + dens_b)                            (trunc_exp; its backward clamps exp to [1e-6, 1e6])
    rgb    = sigmoid(act(base_x + SH_4(dir) @ dir_w^T + dir_b) @ col_w^T + col_b) * (1 + 2 s) - s

The SH direction encoding and the hash-grid encoding are the pinned oracles' (constants here: no gradient w.r.t. dirs, xyz or the table;
the table gradient is tested through a finite difference of this rule)."""
import torch
import torch.nn.functional as F

from oracle import nerf_oracle as NO
from oracle import sh_oracle as SH

ACT = dict(relu=torch.relu, silu=F.silu, softplus=F.softplus)
AXIS = dict(x=0, y=1, z=2)


class _TruncExp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        e = torch.exp(x)
        ctx.save_for_backward(e)
        return e

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0].clamp(min=1e-6, max=1e6)


def plane_features(xyz, code, plane_cfg, flip_z):
    """xyz [N,3], code [3,C,h,w] -> [N, 3C], feature k = c * 3 + p"""
    p = xyz.clone()
    if flip_z:
        p[:, 2] = -p[:, 2]
    grids = torch.stack([torch.stack([p[:, AXIS[pl[0]]], p[:, AXIS[pl[1]]]], -1) for pl in plane_cfg], 0)[:, None]        # [3,1,N,2]
    pc = F.grid_sample(code, grids.to(code.dtype), mode='bilinear', padding_mode='border', align_corners=False)            # [3,C,1,N]
    return pc[:, :, 0].permute(2, 1, 0).reshape(xyz.shape[0], -1)


def point_decode(xyz, dirs, code, w, plane_cfg=('xy', 'xz', 'yz'), flip_z=False, activation='silu', sigmoid_saturation=0.001, hash=None):
    """xyz [N,3], dirs [N,3] or None (density only), code [3,C,h,w]; w: the reference module's state-dict names -> tensors
    (base_net.0.*, density_net.0.*, dir_net.0.*, color_net.0.*, optionally ingp_base_net.0.*);
    hash = dict(table [rows,2] numpy, n_levels, max_resolution, log2_hashmap_size, bound) for TriPlaneiNGPDecoder  -> (sigma [N], rgb [N,3] | None)"""
    dt = code.dtype
    act = ACT[activation]
    base = plane_features(xyz, code, plane_cfg, flip_z) @ w['base_net.0.weight'].T + w['base_net.0.bias']
    if hash is not None:
        enc = NO.hashgrid_encode(((xyz + hash['bound']) / (2 * hash['bound'])).float().numpy(), hash['table'], hash['n_levels'],
                                 hash['max_resolution'], hash['bound'], hash['log2_hashmap_size'])
        base = base + (torch.from_numpy(enc).to(dt) @ w['ingp_base_net.0.weight'].T + w['ingp_base_net.0.bias'])
    sigma = _TruncExp.apply(act(base) @ w['density_net.0.weight'].T + w['density_net.0.bias'])[:, 0]
    if dirs is None:
        return sigma, None
    sh = torch.from_numpy(SH.sh_encode(dirs.numpy(), 4)).to(dt)
    z = base + (sh @ w['dir_net.0.weight'].T + w['dir_net.0.bias'])
    rgb = torch.sigmoid(act(z) @ w['color_net.0.weight'].T + w['color_net.0.bias'])
    return sigma, rgb * (1 + 2 * sigmoid_saturation) - sigmoid_saturation
