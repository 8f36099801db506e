"""LoFTREngine without a GPU: the weight table, the host-side preparations, the refusals, the call surface, the plans, the selection rule."""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loftr_rule                                      # noqa: E402

_spec = importlib.util.spec_from_file_location('make_loftr_golden', os.path.join(HERE, 'golden', 'make_loftr_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope='module')
def mt(lib):
    from mvedit_amd import matcher
    return matcher


@pytest.fixture(scope='module')
def weights():
    return {'matcher.' + k: torch.from_numpy(np.asarray(v)) for k, v in G.make_weights('A').items()}


def test_key_table_consumes_the_reference_layout_exactly_once(mt, weights):
    table = mt.key_table()
    assert sorted(table.values()) == sorted(G.weight_shapes()), 'the table is not the reference state dict'
    assert len(set(table.values())) == len(table)
    params = mt.match_state_dict(weights)                                   # the matcher.-prefixed keys the reference's override strips
    assert not [k for k in params if 'num_batches_tracked' in k] and len(params) == len(table) - 17      # 17 BatchNorms
    assert mt.match_state_dict({k[len('matcher.'):]: v for k, v in weights.items()}).keys() == params.keys()
    missing = dict(weights)
    del missing['matcher.loftr_fine.layers.1.norm2.bias']
    with pytest.raises(KeyError, match='loftr_fine.layers.1.norm2.bias'):
        mt.match_state_dict(missing)
    with pytest.raises(KeyError, match='coarse_matching.bin_score'):
        mt.match_state_dict(dict(weights, **{'matcher.coarse_matching.bin_score': torch.zeros(())}))


def test_slots_have_the_engines_sizes_and_zero_padding(mt, weights):
    slots = mt.pack_slots(mt.match_state_dict(weights))
    n = lambda k: slots[k].numel()
    assert n('stem.w') == 128 * 56 and n('l2.b0.c1.w') == 200 * 9 * 128 and n('l2.b1.c2.w') == 200 * 9 * 200 and n('l2.b0.ds.w') == 200 * 128
    assert n('l3.b0.c1.w') == 256 * 9 * 200 and n('l2oc.w') == 256 * 200 and n('l1oc2.3.w') == 128 * 9 * 200 and n('c0.kv.w') == 512 * 256
    assert n('f1.mlp0.w') == 256 * 256 and n('mf.w') == 128 * 256 and n('l1oc2.0.b') == 200
    assert bool((slots['stem.w'][:, 49:] == 0).all())
    w = slots['l2.b1.c2.w']                                                   # [O][3][3][I] (200 is no multiple of 64): output and input channels 196..199 zero
    assert w.shape == (200, 3, 3, 200) and bool((w[196:] == 0).all()) and bool((w[..., 196:] == 0).all()) and bool((slots['l2.b1.c2.b'][196:] == 0).all())
    assert bool((slots['l3.b0.c1.w'].reshape(256, 3, 3, 200)[..., 196:] == 0).all())
    assert torch.equal(slots['c3.kv.w'][:256], weights['matcher.loftr_coarse.layers.3.k_proj.weight'])
    assert torch.equal(slots['c3.kv.w'][256:], weights['matcher.loftr_coarse.layers.3.v_proj.weight'])


def test_batchnorm_fold_is_conv_then_bn_in_float64(mt):
    g = torch.Generator().manual_seed(3)
    conv = torch.nn.Conv2d(6, 10, 3, stride=2, padding=1, bias=False).double()
    bn = torch.nn.BatchNorm2d(10).double().eval()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(10, generator=g))
        bn.bias.copy_(0.2 * torch.randn(10, generator=g))
        bn.running_mean.copy_(0.5 * torch.randn(10, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(10, generator=g))
        x = torch.randn(2, 6, 9, 8, generator=g, dtype=torch.float64)
        want = bn(conv(x))
        w, b = mt.fold_batchnorm(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        got = F.conv2d(x, w, b, stride=2, padding=1)
    assert w.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-13


@pytest.mark.parametrize('fix', [True, False])
def test_position_table_is_the_closed_form(mt, fix):
    h, w, d = 9, 11, 256
    t = mt.position_table(d, h, w, fix)
    assert t.dtype == torch.float64 and t.shape == (h * w, d)
    rate = -math.log(10000.0) / (d // 2) if fix else -1.0                 # the buggy form: (-log(1e4) / d_model) // 2 = floor(-0.018) = -1
    assert (-math.log(10000.0) / d // 2) == -1.0
    for (y, x, k) in ((0, 0, 0), (3, 7, 5), (8, 10, 63), (4, 2, 17)):
        div = math.exp(2 * k * rate)
        want = [math.sin((x + 1) * div), math.cos((x + 1) * div), math.sin((y + 1) * div), math.cos((y + 1) * div)]
        got = t[y * w + x, 4 * k:4 * k + 4].tolist()
        assert max(abs(a - b) for a, b in zip(got, want)) <= 1e-14
    with pytest.raises(ValueError):
        mt.position_table(d, 257, 4, fix)


def test_refusals_come_before_the_library_is_touched(mt, monkeypatch):
    eng = mt.LoFTREngine(None, torch.float16, device='cpu')                  # create and plan are host-side
    touched = []
    real = mt._lib.call
    monkeypatch.setattr(mt._lib, 'call', lambda name, *a: touched.append(name) or real(name, *a))
    im = torch.zeros(1, 1, 96, 96)
    no = NotImplementedError
    for batch in (dict(image0=im, image1=im, mask0=torch.ones(1, 12, 12)), dict(image0=im, image1=im, mask1=torch.ones(1, 12, 12))):
        with pytest.raises(no):
            eng(batch)
    with pytest.raises(no):
        eng.train()
    with pytest.raises(no):
        eng.requires_grad_(True)
    for bad in (dict(match_coarse=dict(match_type='sinkhorn')), dict(coarse=dict(attention='full')), dict(fine=dict(attention='full')), dict(resolution=(16, 4)),
                dict(fine_concat_coarse_feat=False), dict(fine_window_size=7), dict(coarse=dict(nhead=4)), dict(fine=dict(nhead=4)),
                dict(resnetfpn=dict(block_dims=[128, 192, 256]))):
        with pytest.raises(no):
            mt.LoFTREngine(bad, torch.float16, device='cpu')
    for i0, i1 in ((torch.zeros(1, 3, 96, 96), torch.zeros(1, 3, 96, 96)), (torch.zeros(96, 96), torch.zeros(96, 96)), (im, torch.zeros(1, 1, 96, 88)),
                   (torch.zeros(1, 1, 100, 96), torch.zeros(1, 1, 100, 96)), (torch.zeros(1, 1, 96, 92), torch.zeros(1, 1, 96, 92)),
                   (torch.zeros(1, 1, 8, 2056), torch.zeros(1, 1, 8, 2056))):
        with pytest.raises(ValueError):
            eng(dict(image0=i0, image1=i1))
    assert not touched, touched


def test_module_style_calls_and_the_opt_in_swap(mt):
    from mvedit_amd import dropin
    eng = mt.LoFTREngine(dict(coarse=dict(temp_bug_fix=True)), torch.bfloat16, device='cpu')
    assert eng.requires_grad_(False).to('cpu') is eng and eng.eval() is eng and eng.to(torch.device('cpu')) is eng and eng.train(False) is eng
    assert next(eng.parameters()).dtype == torch.bfloat16
    with pytest.raises(NotImplementedError):
        eng.to(torch.float32)
    runner = types.SimpleNamespace(matcher=None)
    assert dropin.swap_matcher(runner) is runner and runner.matcher is None      # before load_matcher / after unload_matcher: nothing to replace
    marked = types.SimpleNamespace(matcher=eng)
    object.__setattr__(eng, '_mve_is_engine', True)
    assert dropin.swap_matcher(marked).matcher is eng                            # idempotent


def test_plans_are_host_side_and_scale_with_the_capacity(mt):
    eng = mt.LoFTREngine(None, torch.float16, device='cpu')
    a = eng.plan(1, 96, 96, 1)
    labels = [lab for _, _, lab in eng.op_table()]
    assert labels.count('linear attention K^T V') == 12 and labels.count('mutual-nearest selection') == 1 and a['flops']['conv'] > 0 and a['flops']['attention'] > 0 and a['flops']['norm'] == 0
    f = eng.plan(1, 96, 96, 2)
    assert [lab for _, _, lab in eng.op_table()].count('linear attention apply') == 3 and f['n_ops'] < a['n_ops']
    assert eng.plan(2, 72, 88, 1)['workspace_bytes'] > 0
    with pytest.raises(mt._lib.MveError):
        eng.plan(1, 100, 96, 1)


def test_selection_rule_reproduces_the_float64_ids():
    z = G.load()
    for case in G.CASES:
        sim = torch.from_numpy(z[f'{case}/sim_matrix'])
        conf = (F.softmax(sim, 1) * F.softmax(sim, 2)).numpy()               # the reference's conf_matrix (the generator asserts equality)
        hw = (G.CASES[case]['H'] // 8, G.CASES[case]['W'] // 8)
        b, i, j, m = loftr_rule.coarse_matches(conf, hw, hw, 0.2, 2)
        assert np.array_equal(b, z[f'{case}/b_ids']) and np.array_equal(i, z[f'{case}/i_ids']) and np.array_equal(j, z[f'{case}/j_ids'])
        assert np.allclose(m, z[f'{case}/mconf'], rtol=1e-12, atol=0) and len(b) >= G.MIN_MATCHES
        assert np.array_equal(loftr_rule.coarse_keypoints(j, hw[1]).astype(np.float64), z[f'{case}/mkpts1_c'])
