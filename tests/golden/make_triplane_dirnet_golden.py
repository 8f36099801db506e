"""Writes tests/golden/triplane_dirnet_ref.npz (+ triplane_dirnet_ref_grads.npz) and tests/golden/triplane_decoder_cfgs.json for the topology every reference config asks
for (`dir_layers=[16, H]`, `color_layers=[H, 3]`): the reference's own `TriPlaneDecoder.point_decode` / `xyz_transform`
(lib/models/decoders/triplane_decoder.py:106-199) and `TriPlaneiNGPDecoder.point_decode` (lib/models/decoders/triplane_ingp_decoder.py:
142-212) are cut out of the files with `ast` (make_triplane_golden.py's `_methods`) and EXECUTED over a stand-in `self` whose sub-modules are
built the way the constructors build them for these settings (:59-92 / :62-95): base_net = Sequential(Linear(3C, H)), density_net =
Sequential(Linear(H, 1), TruncExp()), dir_net = Sequential(Linear(16, H)), color_net = Sequential(Linear(H, 3), Sigmoid()).
dir_net is seeded NONZERO: the reference zero-initialises it (constant_init(self.dir_net[-1], 0)), which would make every output independent
of the view direction and hide the dir_net product of the kernel.  SH encoder and hash grid: the pinned oracles, a 2^12-row hash map.
Outputs in float32; in float64 the outputs again and, through autograd, the gradients of a recorded random linear functional
sum(g_sigma * sigma) + sum(g_rgb * rgb) w.r.t. the code planes and every Linear.
The JSON holds the `decoder` dict of every reference config file that has one (values only; the runner's override type='TriPlaneiNGPDecoder'
applied to configs/sd/stablessdnerf_cars_lpips.py as lib/apis/adapter3d.py:244 does) and the stand-in modules' state_dict keys with shapes.
Run from the repo root (needs /root/reference):  python tests/golden/make_triplane_dirnet_golden.py"""
import ast
import glob
import importlib.util
import json
import os
import sys
sys.dont_write_bytecode = True
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
from make_triplane_golden import LOG2_HASHMAP, REF, _methods  # noqa: E402
from oracle import nerf_oracle as NO  # noqa: E402
from oracle import sh_oracle as SH  # noqa: E402

OUT = os.path.join(HERE, 'triplane_dirnet_ref.npz')
OUT_GRADS = os.path.join(HERE, 'triplane_dirnet_ref_grads.npz')      # the float64 gradients: a file of their own keeps both under 1 MiB
OUT_CFG = os.path.join(HERE, 'triplane_decoder_cfgs.json')
CASES = [('ssd', dict(C=6, hidden=64, ingp=False, flip_z=False, plane_cfg=['xy', 'xz', 'yz'], act='silu', seed=21)),
         ('stable', dict(C=16, hidden=64, ingp=True, flip_z=True, plane_cfg=['yx', 'yz', 'xz'], act='silu', seed=22)),
         ('wide', dict(C=8, hidden=128, ingp=False, flip_z=False, plane_cfg=['xy', 'xz', 'yz'], act='relu', seed=23))]
N_LEVELS, MAX_RES = 12, 320


class _KeepPrecision(torch.Tensor):
    def float(self):
        return self


def build_self(C, hidden, ingp, flip_z, plane_cfg, act, seed):
    spec = importlib.util.spec_from_file_location('ref_activation', os.path.join(REF, 'lib/ops/activation.py'))
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    torch.manual_seed(seed)
    s = nn.Module()                     # a Module, so that state_dict() names the parameters as the reference's does
    s.plane_cfg, s.interp_mode, s.flip_z, s.use_dir_enc, s.sigmoid_saturation = plane_cfg, 'bilinear', flip_z, True, 0.001
    s.code_dropout, s.scene_base, s.bound = None, None, 1.0
    actl = dict(relu=nn.ReLU, silu=nn.SiLU, softplus=nn.Softplus)[act]
    s.base_net = nn.Sequential(nn.Linear(3 * C, hidden))
    s.base_activation = actl()
    s.density_net = nn.Sequential(nn.Linear(hidden, 1), A.TruncExp())
    s.dir_net = nn.Sequential(nn.Linear(16, hidden))
    s.color_net = nn.Sequential(nn.Linear(hidden, 3), nn.Sigmoid())
    nets = [s.base_net, s.density_net, s.dir_net, s.color_net]
    if ingp:
        s.ingp_base_net = nn.Sequential(nn.Linear(2 * N_LEVELS, hidden))
        nets.append(s.ingp_base_net)
    for m in nets:
        for lin in m:
            if isinstance(lin, nn.Linear):
                nn.init.xavier_uniform_(lin.weight)
                nn.init.uniform_(lin.bias, -0.2, 0.2)
    object.__setattr__(s, 'dir_encoder', lambda d: torch.from_numpy(SH.sh_encode(d.detach().numpy(), 4)).to(d.dtype))
    table = None
    if ingp:
        meta, rows = NO.grid_meta(N_LEVELS, 16, MAX_RES, 1.0, LOG2_HASHMAP)
        table = (torch.rand(rows, 2) * 2 - 1) * 0.5
        # point_decode calls `.float()` on the encoding (tiny-cuda-nn may hand out halves); the stand-in's `.float()` keeps the working
        # precision, so that the float64 run stays float64 (the encoding itself is the oracle's float32 arithmetic either way)
        object.__setattr__(s, 'encoder', lambda x01: types.SimpleNamespace(float=lambda: torch.from_numpy(
            NO.hashgrid_encode(x01.detach().float().numpy(), table.numpy(), N_LEVELS, MAX_RES, 1.0, LOG2_HASHMAP)).to(x01.dtype)))
    return s, table


def decoder_cfgs():
    """{config path relative to configs/: the model's decoder dict}, values only, evaluated from the file's own expressions"""
    out = {}
    for path in sorted(glob.glob(os.path.join(REF, 'configs', '**', '*.py'), recursive=True)):
        tree = ast.parse(open(path).read())
        for node in tree.body:
            if not (isinstance(node, ast.Assign) and getattr(node.targets[0], 'id', None) == 'model' and isinstance(node.value, ast.Call)):
                continue
            for kw in node.value.keywords:
                if kw.arg == 'decoder':
                    d = eval(compile(ast.Expression(kw.value), path, 'eval'), {'dict': dict, '__builtins__': {}})
                    rel = os.path.relpath(path, os.path.join(REF, 'configs'))
                    if rel == os.path.join('sd', 'stablessdnerf_cars_lpips.py'):
                        d['type'] = 'TriPlaneiNGPDecoder'
                    out[rel] = json.loads(json.dumps(d))          # tuples -> lists: values only
    return out


def main():
    out, grads, keys = {}, {}, {}
    for tag, kw in CASES:
        ns = dict(torch=torch, nn=nn, F=F)
        m = _methods(os.path.join(REF, 'lib/models/decoders/triplane_decoder.py'), 'TriPlaneDecoder', ('xyz_transform', 'point_decode'), ns)
        if kw['ingp']:
            m.update(_methods(os.path.join(REF, 'lib/models/decoders/triplane_ingp_decoder.py'), 'TriPlaneiNGPDecoder', ('point_decode',), ns))
        s, table = build_self(**kw)
        object.__setattr__(s, 'xyz_transform', types.MethodType(m['xyz_transform'], s))
        keys[tag] = {k: list(v.shape) for k, v in s.state_dict().items()}
        if kw['ingp']:
            keys[tag]['encoder.params'] = [table.numel()]
        g = torch.Generator().manual_seed(31)
        N, h, w = 600, 24, 32
        code = torch.randn(1, 3, kw['C'], h, w, generator=g)
        xyz = torch.rand(N, 3, generator=g) * 2.3 - 1.15                     # some points beyond the planes: border padding
        dirs = F.normalize(torch.randn(N, 3, generator=g), dim=-1)
        g_sig = torch.randn(N, generator=g) * 0.1
        g_rgb = torch.randn(N, 3, generator=g)
        with torch.no_grad():
            sig, rgb, npts = m['point_decode'](s, [xyz], [dirs], code)
            sig_d, none_rgb, _ = m['point_decode'](s, [xyz], None, code, density_only=True)
            # the reference with its own initialisation of dir_net (zeros): rgb no longer depends on the direction
            saved = [p.clone() for p in s.dir_net.parameters()]
            for p in s.dir_net.parameters():
                p.zero_()
            _, rgb_z, _ = m['point_decode'](s, [xyz], [dirs], code)
            _, rgb_z2, _ = m['point_decode'](s, [xyz], [dirs.flip(0)], code)
            for p, q in zip(s.dir_net.parameters(), saved):
                p.copy_(q)
            _, rgb_f, _ = m['point_decode'](s, [xyz], [dirs.flip(0)], code)
        assert none_rgb is None and torch.equal(sig, sig_d) and npts == [N] and torch.equal(rgb_z, rgb_z2)
        pre = f'{tag}_'
        out.update({pre + 'code': code.numpy(), pre + 'xyz': xyz.numpy(), pre + 'dirs': dirs.numpy(), pre + 'sigmas': sig.numpy(), pre + 'rgbs': rgb.numpy(),
                    pre + 'rgbs_zero_dirnet': rgb_z.numpy(), pre + 'rgbs_flipped_dirs': rgb_f.numpy(), pre + 'g_sig': g_sig.numpy(), pre + 'g_rgb': g_rgb.numpy()})
        for k, v in s.state_dict().items():
            out[pre + 'w:' + k] = v.numpy()
        if kw['ingp']:
            out[pre + 'table'] = table.numpy()
        # float64: outputs and autograd gradients.  point_decode samples `code.float()`, which would round the planes' GRADIENT to float32 on
        # its way back; the planes go in as a tensor whose `.float()` keeps the working precision (as the stand-in encoder's does)
        s.double()
        c64 = code.double().as_subclass(_KeepPrecision).requires_grad_(True)
        sig64, rgb64, _ = m['point_decode'](s, [xyz.double()], [dirs.double()], c64)
        out[pre + 'sigmas64'], out[pre + 'rgbs64'] = sig64.detach().as_subclass(torch.Tensor).numpy(), rgb64.detach().as_subclass(torch.Tensor).numpy()
        leaves = [c64] + list(s.parameters())
        names = ['code'] + [k for k, _ in s.named_parameters()]
        loss = (sig64 * g_sig.double()).sum() + (rgb64 * g_rgb.double()).sum()
        for n, gr in zip(names, torch.autograd.grad(loss, leaves)):
            grads[f'{pre}grad:{n}'] = gr.as_subclass(torch.Tensor).numpy()
    np.savez_compressed(OUT, **out)
    np.savez_compressed(OUT_GRADS, **grads)
    cfgs = decoder_cfgs()
    with open(OUT_CFG, 'w') as fh:
        json.dump({'configs': cfgs, 'state_dict_keys': keys}, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', OUT, os.path.getsize(OUT), OUT_GRADS, os.path.getsize(OUT_GRADS), OUT_CFG, len(cfgs), 'configs')


if __name__ == '__main__':
    main()
