"""The tri-plane decoders' dir-net topology (`dir_layers=[16, H]`, `color_layers=[H, 3]`: what every config file of the reference asks for):
csrc/triplane.hip's k_triplane_dirnet_* behind mvedit_amd.triplane, against the reference's own `point_decode` EXECUTED
(tests/golden/triplane_dirnet_ref.npz + _grads.npz, tests/golden/make_triplane_dirnet_golden.py) and the float64 rule tests/triplane_dirnet_rule.py.
Bars are test_triplane.py's: sigma 2e-5 relative (an exponential), rgb 2e-5 absolute on the GPU (2e-6 for the fp32 restatement), gradients
2e-4 of the tensor's magnitude + 1e-6; the float64 rule against the float64 reference run: 1e-10."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import triplane_dirnet_rule as R  # noqa: E402

G = np.load(os.path.join(HERE, 'golden', 'triplane_dirnet_ref.npz'))
GG = np.load(os.path.join(HERE, 'golden', 'triplane_dirnet_ref_grads.npz'))
with open(os.path.join(HERE, 'golden', 'triplane_decoder_cfgs.json')) as fh:
    CFGS = json.load(fh)
CASES = {'ssd': dict(plane_cfg=('xy', 'xz', 'yz'), flip_z=False, activation='silu', ingp=False),
         'stable': dict(plane_cfg=('yx', 'yz', 'xz'), flip_z=True, activation='silu', ingp=True),
         'wide': dict(plane_cfg=('xy', 'xz', 'yz'), flip_z=False, activation='relu', ingp=False)}
HASH = dict(n_levels=12, max_resolution=320, log2_hashmap_size=12, bound=1.0)


def weights(tag, dtype=torch.float32):
    pre = f'{tag}_w:'
    return {k[len(pre):]: torch.from_numpy(G[k]).to(dtype) for k in G.files if k.startswith(pre)}


def rule(tag, xyz, dirs, code, w, table=None):
    c = CASES[tag]
    hash_ = dict(HASH, table=G[f'{tag}_table'] if table is None else table) if c['ingp'] else None
    return R.point_decode(xyz, dirs, code, w, c['plane_cfg'], c['flip_z'], c['activation'], hash=hash_)


def state_dict(tag):
    sd = {k: v.clone() for k, v in weights(tag).items()}
    if CASES[tag]['ingp']:
        sd['encoder.params'] = torch.from_numpy(G[f'{tag}_table'].reshape(-1).copy())
    return sd


def engine(tag, device='cuda'):
    from mvedit_amd.triplane import TriPlaneDecoder, TriPlaneiNGPDecoder
    c = CASES[tag]
    kw = dict(plane_cfg=c['plane_cfg'], activation=c['activation'], flip_z=c['flip_z'], device=device)
    eng = TriPlaneiNGPDecoder(n_levels=12, max_resolution=320, log2_hashmap_size=12, **kw) if c['ingp'] else TriPlaneDecoder(**kw)
    return eng.load_state_dict(state_dict(tag))


# ---- CPU: the goldens and the rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', list(CASES))
def test_rule_equals_reference_output_and_gradients(tag):
    t = lambda k: torch.from_numpy(G[f'{tag}_{k}'])
    sig, rgb = rule(tag, t('xyz'), t('dirs'), t('code')[0], weights(tag))
    np.testing.assert_allclose(sig.numpy(), G[f'{tag}_sigmas'], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(rgb.numpy(), G[f'{tag}_rgbs'], rtol=0, atol=2e-6)
    assert G[f'{tag}_sigmas'].std() > 0.05 and G[f'{tag}_rgbs'].std() > 0.02
    assert (np.abs(G[f'{tag}_xyz']) > 1).any(), 'border padding must be exercised'
    # float64: values and the gradients of the recorded functional
    w64 = {k: v.clone().requires_grad_(True) for k, v in weights(tag, torch.float64).items()}
    code64 = t('code')[0].double().requires_grad_(True)
    sig, rgb = rule(tag, t('xyz').double(), t('dirs').double(), code64, w64)
    np.testing.assert_allclose(sig.detach().numpy(), G[f'{tag}_sigmas64'], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(rgb.detach().numpy(), G[f'{tag}_rgbs64'], rtol=0, atol=1e-10)
    ((sig * t('g_sig').double()).sum() + (rgb * t('g_rgb').double()).sum()).backward()
    pre = f'{tag}_grad:'
    names = [k[len(pre):] for k in GG.files if k.startswith(pre)]
    assert sorted(names) == sorted(['code'] + list(w64))
    for n in names:
        got = code64.grad if n == 'code' else w64[n].grad
        want = GG[pre + n].reshape(got.shape)
        scale = max(1.0, np.abs(want).max())
        assert np.abs(got.numpy() - want).max() <= 1e-10 * scale, n


@pytest.mark.parametrize('tag', list(CASES))
def test_golden_rgb_depends_on_the_direction_only_through_dir_net(tag):
    """The reference initialises dir_net to zero; the golden's is seeded nonzero so that the kernel's dir_net product is visible."""
    t = lambda k: torch.from_numpy(G[f'{tag}_{k}'])
    w = weights(tag)
    assert float(w['dir_net.0.weight'].abs().max()) > 0.1
    w0 = dict(w, **{'dir_net.0.weight': torch.zeros_like(w['dir_net.0.weight']), 'dir_net.0.bias': torch.zeros_like(w['dir_net.0.bias'])})
    _, a = rule(tag, t('xyz'), t('dirs'), t('code')[0], w0)
    _, b = rule(tag, t('xyz'), t('dirs').flip(0), t('code')[0], w0)
    assert torch.equal(a, b)
    np.testing.assert_allclose(a.numpy(), G[f'{tag}_rgbs_zero_dirnet'], rtol=0, atol=2e-6)
    _, c = rule(tag, t('xyz'), t('dirs').flip(0), t('code')[0], w)
    np.testing.assert_allclose(c.numpy(), G[f'{tag}_rgbs_flipped_dirs'], rtol=0, atol=2e-6)
    moved = float(np.abs(G[f'{tag}_rgbs_flipped_dirs'] - G[f'{tag}_rgbs']).max())
    by_dirnet = float(np.abs(G[f'{tag}_rgbs_zero_dirnet'] - G[f'{tag}_rgbs']).max())
    print(f'{tag}: max |rgb(dirs) - rgb(other dirs)| = {moved:.3f}; max |rgb - rgb(dir_net = 0)| = {by_dirnet:.3f}')
    assert moved > 1e-2 and by_dirnet > 1e-2


# ---- CPU: the Python surface --------------------------------------------------------------------------------------------------------------
def _cls(cfg):
    from mvedit_amd.triplane import TriPlaneDecoder, TriPlaneiNGPDecoder
    return TriPlaneiNGPDecoder if cfg['type'] == 'TriPlaneiNGPDecoder' else TriPlaneDecoder


def test_from_config_accepts_every_reference_config():
    pytest.importorskip('mvedit_amd._lib')
    from mvedit_amd.triplane import TOPOLOGY_DIRNET
    assert len(CFGS['configs']) == 16
    for path, cfg in CFGS['configs'].items():
        dec = _cls(cfg).from_config(cfg, device='cpu')
        assert dec.topology == TOPOLOGY_DIRNET and dec.cfg_layers == (TOPOLOGY_DIRNET, cfg['base_layers'][0], 64, None), path
        assert dec.flip_z == cfg.get('flip_z', False) and (dec.hash is not None) == (cfg['type'] == 'TriPlaneiNGPDecoder')
    sd_cfg = CFGS['configs']['sd/stablessdnerf_cars_lpips.py']
    assert _cls(sd_cfg).from_config(sd_cfg, device='cpu').axes == [1, 0, 1, 2, 0, 2]          # ['yx', 'yz', 'xz']


def test_from_config_accepts_the_default_topology_and_refuses_what_is_not_built():
    pytest.importorskip('mvedit_amd._lib')
    from mvedit_amd.triplane import TOPOLOGY_DEFAULT, TriPlaneDecoder, TriPlaneiNGPDecoder
    assert TriPlaneDecoder.from_config({}, device='cpu').cfg_layers == (TOPOLOGY_DEFAULT, 96, 128, 128)          # the constructor's own defaults
    base = CFGS['configs']['paper_cfgs/ssdnerf_cars_uncond.py']
    for bad in (dict(use_dir_enc=False), dict(interp_mode='nearest'), dict(scene_base_size=[3, 6, 128, 128]), dict(code_dropout=0.1),
                dict(base_layers=[18, 64, 64]), dict(density_layers=[64, 64, 1]), dict(dir_layers=[16, 64, 64]), dict(color_layers=[64, 64, 3]),
                dict(dir_layers=None), dict(base_layers=[18, 32], density_layers=[32, 1], color_layers=[32, 3], dir_layers=[16, 32])):
        with pytest.raises(NotImplementedError):
            TriPlaneDecoder.from_config(dict(base, **bad), device='cpu')
    with pytest.raises(NotImplementedError):
        TriPlaneiNGPDecoder.from_config(dict(base, ingp_base_layers=2), device='cpu', log2_hashmap_size=12)
    # a decoder built from a config holds the state dict to that config
    dec = TriPlaneDecoder.from_config(base, device='cpu').load_state_dict(state_dict('ssd'))
    assert set(dec.parameters()) == set(CFGS['state_dict_keys']['ssd'])
    with pytest.raises(ValueError):
        TriPlaneDecoder.from_config(base, device='cpu').load_state_dict(state_dict('wide'))


def _default_sd(H=64, H2=64, C=4):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    return {'base_net.0.weight': r(H, 3 * C), 'base_net.0.bias': r(H), 'density_net.0.weight': r(1, H), 'density_net.0.bias': r(1),
            'color_net.0.weight': r(H2, H + 16), 'color_net.0.bias': r(H2), 'color_net.2.weight': r(3, H2), 'color_net.2.bias': r(3)}


@pytest.mark.parametrize('tag', list(CASES))
def test_load_state_dict_recognises_the_topology_from_the_keys(tag):
    pytest.importorskip('mvedit_amd._lib')
    from mvedit_amd.triplane import TOPOLOGY_DEFAULT, TOPOLOGY_DIRNET, TriPlaneDecoder
    recorded = CFGS['state_dict_keys'][tag]
    sd = state_dict(tag)
    assert {k: list(v.shape) for k, v in sd.items()} == recorded
    sd['preprocessor.conv_in.weight'] = torch.zeros(4, 4, 3, 3)                       # a full decoder's state dict: ignored
    eng = engine(tag, 'cpu').load_state_dict(sd)
    assert eng.topology == TOPOLOGY_DIRNET and set(eng.parameters()) == set(recorded)
    assert eng.w['dir_wT'].shape == (16, recorded['dir_net.0.bias'][0]) and eng.w['col2_w'].shape == (3, recorded['dir_net.0.bias'][0])
    plain = TriPlaneDecoder(device='cpu')
    assert plain.load_state_dict(_default_sd()).topology == TOPOLOGY_DEFAULT and 'dir_wT' not in plain.w
    H = recorded['base_net.0.bias'][0]
    refused = {'color_net.2.weight': torch.zeros(3, H),                               # a mixture of the two topologies
               'base_net.2.weight': torch.zeros(H, H), 'density_net.2.weight': torch.zeros(1, H), 'dir_net.2.weight': torch.zeros(H, H),
               'color_net.4.weight': torch.zeros(3, H), 'scene_base': torch.zeros(3, 6, 8, 8)}
    for name, t in refused.items():
        with pytest.raises(NotImplementedError, match=name.replace('.', r'\.')):
            engine(tag, 'cpu').load_state_dict(dict(state_dict(tag), **{name: t}))
    with pytest.raises(NotImplementedError, match=r'color_net\.2\.weight'):           # the default topology + a dir_net: the same mixture
        TriPlaneDecoder(device='cpu').load_state_dict(dict(_default_sd(), **{'dir_net.0.weight': torch.zeros(64, 16), 'dir_net.0.bias': torch.zeros(64)}))
    with pytest.raises(NotImplementedError, match=r'base_net\.0\.weight'):
        TriPlaneDecoder(device='cpu').load_state_dict(_default_sd(H=32, H2=64))
    for name in recorded:
        with pytest.raises(KeyError, match=name.replace('.', r'\.')):
            engine(tag, 'cpu').load_state_dict({k: v for k, v in state_dict(tag).items() if k != name})


def test_packed_dir_net_copies_follow_edits():
    """test_triplane.py::test_packed_parameter_copies_follow_edits, for dir_net.*"""
    pytest.importorskip('mvedit_amd._lib')
    eng = engine('ssd', 'cpu')
    p_b, p_w = eng.params['dir_net.0.bias'], eng.params['dir_net.0.weight']
    assert eng.w['dir_b'].data_ptr() != p_b.data_ptr() and torch.equal(eng.w['dir_wT'], p_w.t())
    p_b.add_(1.0)
    eng._pack()
    assert torch.equal(eng.w['dir_b'], p_b)
    p_b.data.mul_(2.0)
    p_w.data.mul_(2.0)
    eng._pack()
    assert not torch.equal(eng.w['dir_b'], p_b) and not torch.equal(eng.w['dir_wT'], p_w.t())
    eng.invalidate()
    eng._pack()
    assert torch.equal(eng.w['dir_b'], p_b) and torch.equal(eng.w['dir_wT'], p_w.t())


@pytest.mark.parametrize('struct', ['MveTriplaneDesc', 'MveTriplaneGrads'])
def test_extended_struct_layouts_match_the_header(tmp_path, struct):
    pytest.importorskip('mvedit_amd._lib')
    from mvedit_amd import triplane as T
    mirror = dict(MveTriplaneDesc=T._Desc, MveTriplaneGrads=T._Grads)[struct]
    fields = [f[0] for f in mirror._fields_]
    assert fields[-2:] == dict(MveTriplaneDesc=['d_dir_wT', 'd_dir_b'], MveTriplaneGrads=['d_dir_w', 'd_dir_b'])[struct]
    src = tmp_path / 'layout.c'
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "mvedit_amd.h"\nint main(void) {{\n  printf("%zu", sizeof({struct}));\n'
                   + ''.join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in fields)
                   + '  printf(" %d %d", MVE_TRIPLANE_DEFAULT, MVE_TRIPLANE_DIRNET);\n  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(os.path.dirname(HERE), 'include'), str(src), '-o', str(exe)], check=True)
    nums = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == ctypes.sizeof(mirror) and nums[1:-2] == [getattr(mirror, f).offset for f in fields]
    assert nums[-2:] == [T.TOPOLOGY_DEFAULT, T.TOPOLOGY_DIRNET]


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('tag', list(CASES))
def test_hip_vs_reference_output(lib, tag):
    eng = engine(tag)
    t = lambda k: torch.from_numpy(G[f'{tag}_{k}']).cuda()
    sig, rgb, n = eng.point_decode([t('xyz')], [t('dirs')], t('code'))
    assert n == [600]
    np.testing.assert_allclose(sig.cpu().numpy(), G[f'{tag}_sigmas'], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(rgb.cpu().numpy(), G[f'{tag}_rgbs'], rtol=0, atol=2e-5)
    sig2, n2 = eng.point_density_decode([t('xyz')], t('code'))
    assert torch.equal(sig2, sig) and n2 == n
    with pytest.raises(NotImplementedError):
        eng.point_decode([t('xyz').requires_grad_(True)], [t('dirs')], t('code'))
    # point independence: a prefix decoded alone gives the same bits (5: one partial wave; 64: exactly one; 65: one and a tail of one)
    for m in (5, 64, 65):
        s_m, r_m, n_m = eng.point_decode([t('xyz')[:m]], [t('dirs')[:m]], t('code'))
        assert n_m == [m] and torch.equal(s_m, sig[:m]) and torch.equal(r_m, rgb[:m]), m


@pytest.mark.gpu
@pytest.mark.parametrize('density_only', [False, True], ids=['sigma+rgb', 'sigma'])
@pytest.mark.parametrize('tag', list(CASES))
def test_hip_backward_vs_rule_autograd(lib, tag, density_only):
    """mve_triplane_backward's dir-net path (behind point_decode_autograd) against torch autograd over the float64 rule, as
    test_triplane.py::test_hip_backward_vs_oracle_autograd holds the default topology; the hash-table gradient through the same directional
    finite difference of the rule."""
    c = CASES[tag]
    eng = engine(tag)
    g = torch.Generator().manual_seed(11)
    N = 3001
    xyz = torch.rand(N, 3, generator=g) * 2.2 - 1.1
    dirs = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    code = torch.from_numpy(G[f'{tag}_code']).clone()
    g_sig = torch.randn(N, generator=g) * 0.1
    g_rgb = torch.randn(N, 3, generator=g)

    def rule_loss(w64, code64, table):
        so, ro = rule(tag, xyz.double(), None if density_only else dirs.double(), code64, w64, table)
        loss = (so * g_sig.double()).sum()
        return loss if density_only else loss + (ro * g_rgb.double()).sum()

    w64 = {k: v.clone().requires_grad_(True) for k, v in weights(tag, torch.float64).items()}
    code64 = code[0].double().clone().requires_grad_(True)
    table = G[f'{tag}_table'] if c['ingp'] else None
    rule_loss(w64, code64, table).backward()

    def run():
        for p in eng.parameters().values():
            p.requires_grad_(True)
            p.grad = None
        code_d = code.cuda().requires_grad_(True)
        sig, rgb, n = eng.point_decode_autograd([xyz.cuda()], [dirs.cuda()], code_d, density_only=density_only)
        assert n == [N] and (rgb is None) == density_only
        loss = (sig * g_sig.cuda()).sum()
        if not density_only:
            loss = loss + (rgb * g_rgb.cuda()).sum()
        loss.backward()
        return sig.detach(), (None if rgb is None else rgb.detach()), code_d.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in eng.parameters().items()}

    sig, rgb, g_code, grads = run()

    def close(got, want, what):
        want = want.float()
        scale = want.abs().max().item()
        err = (got.cpu() - want).abs().max().item()
        assert err <= 2e-4 * scale + 1e-6, f'{tag} {what}: max |d| {err:.3e} against a gradient of magnitude {scale:.3e}'

    close(g_code[0], code64.grad, 'code planes')
    colour = ('dir_net.0.weight', 'dir_net.0.bias', 'color_net.0.weight', 'color_net.0.bias')
    assert set(colour) < set(grads)
    for name, gr in grads.items():
        if name == 'encoder.params':
            continue
        if density_only and name in colour:
            assert gr is None or float(gr.abs().max()) == 0.0, name
            continue
        close(gr.reshape(w64[name].shape), w64[name].grad, name)
    if c['ingp']:
        gt = grads['encoder.params'].cpu().reshape(-1, 2)
        D = np.random.default_rng(3).standard_normal(table.shape).astype(np.float32)
        eps = 1e-2
        w0 = {k: v.detach() for k, v in w64.items()}
        with torch.no_grad():
            fd = (rule_loss(w0, code64.detach(), table + eps * D) - rule_loss(w0, code64.detach(), table - eps * D)).item() / (2 * eps)
        an = float((gt.double() * torch.from_numpy(D).double()).sum())
        assert abs(fd - an) <= 2e-3 * max(abs(fd), abs(an)) + 1e-4, (fd, an)
    # the forward of point_decode_autograd equals point_decode
    with torch.no_grad():
        s2, r2, _ = eng.point_decode([xyz.cuda()], None if density_only else [dirs.cuda()], code.cuda(), density_only=density_only)
    assert torch.equal(s2, sig) and (density_only or torch.equal(r2, rgb))
    # every Linear's gradient is reduced in a fixed order: a second run gives the same bits
    _, _, _, again = run()
    for name, gr in grads.items():
        if name != 'encoder.params' and gr is not None:
            assert torch.equal(gr, again[name]), name
