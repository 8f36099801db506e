"""LoFTREngine on an MI355X against the float64 golden (tests/golden/make_loftr_golden.py: the reference's own `loftr` package on the CPU).

Cases A (N = 1, 96 x 96, temp_bug_fix=True) and B (N = 2, 72 x 88, temp_bug_fix=False), fp16 and bf16; weights and pixels are regenerated from the
golden's seeds and checked by sha256.

  continuous taps   every tap from the stem through sim_matrix: rel-L2 against float64 on the golden's stored positions <= 1.5 x the error of torch's
                    own CPU 16-bit module on that tap (the project's bar for pinned networks).  conf_matrix is printed, not held: it is
                    exponentially sensitive (the CPU 16-bit modules sit at 0.1 - 0.9 rel-L2).
  selection         b_ids / i_ids / j_ids / mconf equal, exactly and in order, what tests/loftr_rule.py derives from the engine's own downloaded
                    conf_matrix; mkpts*_c are the ids times 8
  fine stage        run on the golden's float64 ids (`coarse_matches=`): unfold, merged and fine windows, expec_f and mkpts1_f <= 1.5 x the CPU
                    16-bit module's error (which ran its fine stage on the same ids); |mkpts1_f - mkpts1_c| <= 4 px
  the call          engine(batch) fills every key the reference fills; M = 0 (thr raised to 2) runs no fine op; an all-zero pair runs without
                    error (the position encoding alone separates the cells, so it may well match)
  recorded          common / only-float64 / only-engine match counts beside the CPU 16-bit module's (chaos on seeded weights: not asserted)

Measured on an MI355X: rel-L2 against float64, engine | CPU 16-bit module (the ratio is what the 1.5 bar holds).  The fp16 CPU module loses two
digits from coarse layer 3 (case A) / 5 (case B) on -- LinearAttention in fp16 -- which the engine's fp32 accumulators do not.
                      case A fp16          case A bf16          case B fp16          case B bf16
  stem             2.35e-4 | 2.34e-4    2.15e-3 | 3.32e-3    2.32e-4 | 2.38e-4    2.22e-3 | 3.70e-3
  layer1           3.99e-4 | 4.46e-4    3.51e-3 | 5.17e-3    4.68e-4 | 4.85e-4    3.44e-3 | 5.36e-3
  layer2           5.95e-4 | 6.28e-4    4.66e-3 | 7.38e-3    5.79e-4 | 5.67e-4    4.27e-3 | 7.06e-3
  layer3           7.79e-4 | 7.32e-4    5.25e-3 | 9.56e-3    7.39e-4 | 8.31e-4    5.98e-3 | 9.01e-3
  fpn_c            8.33e-4 | 8.27e-4    6.19e-3 | 9.78e-3    8.04e-4 | 8.67e-4    6.55e-3 | 9.87e-3
  fpn_f            6.64e-4 | 6.34e-4    6.37e-3 | 8.84e-3    9.17e-4 | 8.43e-4    7.14e-3 | 1.02e-2
  pos0 / pos1      7.80e-4 | 8.33e-4    5.77e-3 | 9.09e-3    8.00e-4 | 8.68e-4    6.55e-3 | 9.06e-3
  c0_0             8.00e-4 | 8.68e-4    6.66e-3 | 9.41e-3    8.13e-4 | 9.11e-4    7.32e-3 | 9.80e-3
  c3_0             9.63e-4 | 3.33e-2    8.31e-3 | 1.09e-2    9.61e-4 | 1.05e-3    8.27e-3 | 1.12e-2
  c7_0             1.05e-3 | 6.27e-2    9.02e-3 | 1.18e-2    1.09e-3 | 1.94e-2    9.46e-3 | 1.24e-2
  c7_1             1.02e-3 | 7.27e-2    9.26e-3 | 1.23e-2    1.16e-3 | 2.60e-2    9.67e-3 | 1.25e-2
  sim_matrix       1.26e-4 | 7.24e-3    1.01e-3 | 3.09e-3    1.39e-4 | 2.44e-3    1.12e-3 | 3.24e-3
  worst ratio      1.06 (layer3)        0.82 (c4_0)          1.09 (fpn_f)         0.83 (c6_0)
  conf_matrix      1.06e-3 | 9.28e-2    2.13e-2 | 7.69e-2    1.24e-2 | 1.73e-1    8.86e-2 | 8.74e-1      (printed, not held)
 fine stage on the float64 ids:
  unfold0          6.51e-4 | 6.37e-4    6.15e-3 | 8.47e-3    9.52e-4 | 8.52e-4    7.01e-3 | 9.95e-3
  merged0          7.81e-4 | 1.46e-2    7.33e-3 | 1.01e-2    9.07e-4 | 3.83e-3    7.12e-3 | 1.02e-2
  fine1            7.71e-4 | 1.77e-2    7.69e-3 | 1.02e-2    1.02e-3 | 7.01e-3    8.52e-3 | 1.18e-2
  expec_f          1.36e-3 | 7.13e-3    1.64e-2 | 6.01e-2    1.78e-3 | 5.22e-3    1.41e-2 | 2.70e-2
  mkpts1_f         1.02e-4 | 5.19e-4    1.27e-3 | 4.55e-3    1.89e-4 | 5.47e-4    1.44e-3 | 2.69e-3
  worst ratio      1.02 (unfold0)       0.75 (fine0)         1.14 (unfold1)       0.73 (merged1)
 match sets against the 8 float64 matches (common / only float64 / only 16-bit) -- recorded, not asserted:
  engine           8 / 0 / 0            7 / 1 / 3            8 / 0 / 0            6 / 2 / 0
  CPU module       7 / 1 / 3            3 / 5 / 5            6 / 2 / 3            2 / 6 / 5
"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loftr_rule                                      # noqa: E402

_spec = importlib.util.spec_from_file_location('make_loftr_golden', os.path.join(HERE, 'golden', 'make_loftr_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

pytestmark = pytest.mark.gpu

DTYPES = {'fp16': torch.float16, 'bf16': torch.bfloat16}
ERR_KEY = {'fp16': 'err16', 'bf16': 'errbf'}
COARSE = ('stem', 'layer1', 'layer2', 'layer3', 'fpn_c', 'fpn_f', 'pos0', 'pos1') + tuple(f'c{k}_{s}' for k in range(8) for s in (0, 1)) + ('sim_matrix',)
FINE = ('unfold0', 'unfold1', 'merged0', 'merged1', 'fine0', 'fine1', 'expec_f', 'mkpts1_f')
_cache = {}


def golden():
    if 'golden' not in _cache:
        _cache['golden'] = G.load()
    return _cache['golden']


def inputs(case):
    if ('in', case) not in _cache:
        seed = int(golden()[f'{case}/seed'])
        sd = {'matcher.' + k: torch.from_numpy(np.asarray(v)) for k, v in G.make_weights(case, seed).items()}
        px = tuple(torch.from_numpy(p) for p in G.make_pixels(case, seed))
        _cache[('in', case)] = (sd, px)
    return _cache[('in', case)]


def engine(lib, case, dt):
    if ('eng', case, dt) not in _cache:
        from mvedit_amd.matcher import LoFTREngine
        eng = LoFTREngine(dict(coarse=dict(temp_bug_fix=G.CASES[case]['temp_bug_fix'])), dtype=DTYPES[dt], device='cuda')
        eng.load_state_dict(inputs(case)[0])
        _cache[('eng', case, dt)] = eng
    return _cache[('eng', case, dt)]


def free_run(lib, case, dt):
    if ('free', case, dt) not in _cache:
        px = inputs(case)[1]
        _cache[('free', case, dt)] = engine(lib, case, dt).run(px[0], px[1], output_features=True)
    return _cache[('free', case, dt)]


def engine_tap(case, name, feats, out):
    N = G.CASES[case]['N']
    if name == 'layer2':
        assert bool((feats['layer2'][:, 196:] == 0).all()), 'the 4 padding channels of the 196-wide stage are not zero'
        return feats['layer2'][:, :196]
    if name[:3] == 'pos' or (name[0] == 'c' and name[1].isdigit()):
        key, side = name[:-1].rstrip('_'), int(name[-1])
        return feats[key][side * N:(side + 1) * N]
    if name[:-1] in ('unfold', 'merged', 'fine'):
        M = feats[name[:-1]].shape[0] // 2
        return feats[name[:-1]][int(name[-1]) * M:(int(name[-1]) + 1) * M]
    if name in ('expec_f', 'mkpts1_f', 'conf_matrix'):
        return out[name]
    return feats[name]


def tap_errors(case, dt, names, feats, out):
    g, rows = golden(), []
    for name in names:
        got = engine_tap(case, name, feats, out)
        assert tuple(got.shape) == tuple(g[f'{case}/shape/{name}']), (name, tuple(got.shape))
        got = got.double().cpu().reshape(-1)
        if name == 'sim_matrix':
            idx, ref = G.sample_index(case, name, got.numel()), torch.from_numpy(g[f'{case}/sim_matrix']).reshape(-1)
            ref = ref[idx]
        else:
            idx, ref = G.sample_index(case, name, got.numel()), torch.from_numpy(g[f'{case}/{name}']).double()
        err = float((got[idx] - ref).norm() / ref.norm())
        rows.append((name, err, float(g[f'{case}/{ERR_KEY[dt]}/{name}'])))
    return rows


def show(title, rows):
    print(f'\n{title}\n  {"tap":<12} {"engine":>10} {"module":>10} {"ratio":>6}')
    for name, err, mod in rows:
        print(f'  {name:<12} {err:>10.3e} {mod:>10.3e} {err / mod:>6.2f}')


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('case', ['A', 'B'])
def test_continuous_taps_within_one_and_a_half_module_errors(lib, case, dt):
    out, feats = free_run(lib, case, dt)
    rows = tap_errors(case, dt, COARSE, feats, out)
    show(f'case {case} {dt}: rel-L2 against float64, engine / CPU {dt} module', rows)
    show('  (printed, not held)', tap_errors(case, dt, ('conf_matrix',), feats, out))
    bad = [(n, e, m) for n, e, m in rows if not e <= 1.5 * m]
    assert not bad, bad


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('case', ['A', 'B'])
def test_selection_is_the_rule_on_the_engines_own_conf_matrix(lib, case, dt):
    out, _ = free_run(lib, case, dt)
    c = G.CASES[case]
    hw = (c['H'] // 8, c['W'] // 8)
    b, i, j, m = loftr_rule.coarse_matches(out['conf_matrix'].cpu().numpy(), hw, hw, 0.2, 2)
    assert np.array_equal(out['b_ids'].cpu().numpy(), b) and np.array_equal(out['i_ids'].cpu().numpy(), i) and np.array_equal(out['j_ids'].cpu().numpy(), j)
    assert np.array_equal(out['mconf'].cpu().numpy().view(np.int32), m.view(np.int32))
    assert np.array_equal(out['mkpts0_c'].cpu().numpy(), loftr_rule.coarse_keypoints(i, hw[1]).reshape(-1, 2))
    assert np.array_equal(out['mkpts1_c'].cpu().numpy(), loftr_rule.coarse_keypoints(j, hw[1]).reshape(-1, 2))
    # recorded, not asserted: the match set against float64, beside the CPU 16-bit module's
    g = golden()
    want = set(zip(g[f'{case}/b_ids'].tolist(), g[f'{case}/i_ids'].tolist(), g[f'{case}/j_ids'].tolist()))
    got = set(zip(b.tolist(), i.tolist(), j.tolist()))
    mod = g[f'{case}/matches16'][list(DTYPES).index(dt)].tolist()
    print(f'\ncase {case} {dt} match sets (common / only float64 / only 16-bit): engine {[len(want & got), len(want - got), len(got - want)]}, CPU {dt} module {mod}')


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('case', ['A', 'B'])
def test_fine_stage_on_the_float64_matches(lib, case, dt):
    g, px = golden(), inputs(case)[1]
    ids = tuple(torch.from_numpy(g[f'{case}/{k}']) for k in ('b_ids', 'i_ids', 'j_ids'))
    out, feats = engine(lib, case, dt).run(px[0], px[1], coarse_matches=ids, output_features=True)
    assert out['mkpts1_f'].dtype == torch.float32 and out['expec_f'].dtype == torch.float32
    assert np.array_equal(out['mkpts1_c'].cpu().numpy().astype(np.float64), g[f'{case}/mkpts1_c'])
    rows = tap_errors(case, dt, FINE, feats, out)
    show(f'case {case} {dt}, fine stage on the float64 ids: rel-L2 against float64, engine / CPU {dt} module', rows)
    bad = [(n, e, m) for n, e, m in rows if not e <= 1.5 * m]
    assert not bad, bad
    assert float((out['mkpts1_f'] - out['mkpts1_c']).abs().max()) <= 4.0


@pytest.mark.parametrize('dt', list(DTYPES))
def test_the_call_fills_the_batch_and_survives_an_empty_match_set(lib, dt):
    case = 'A'
    eng, px = engine(lib, case, dt), inputs(case)[1]
    batch = dict(image0=px[0].float().cuda(), image1=px[1].float().cuda())
    assert eng.requires_grad_(False).to('cuda').eval() is eng
    assert eng(batch) is None
    keys = ('mkpts0_f', 'mkpts1_f', 'mconf', 'mkpts0_c', 'mkpts1_c', 'b_ids', 'i_ids', 'j_ids', 'm_bids', 'conf_matrix', 'expec_f', 'hw0_i', 'hw1_i', 'hw0_c',
            'hw1_c', 'hw0_f', 'hw1_f', 'W', 'bs')
    assert not [k for k in keys if k not in batch]
    M = batch['b_ids'].shape[0]
    assert M > 0 and batch['mkpts0_f'] is batch['mkpts0_c']
    for k in ('mkpts0_f', 'mkpts1_f', 'mconf', 'expec_f', 'conf_matrix'):
        assert batch[k].dtype == torch.float32 and batch[k].is_cuda, k
    assert batch['mkpts1_f'].shape == (M, 2) and batch['expec_f'].shape == (M, 3) and batch['b_ids'].dtype == torch.int64
    assert tuple(batch['hw0_c']) == (12, 12) and tuple(batch['hw0_f']) == (48, 48) and tuple(batch['hw0_i']) == (96, 96) and batch['W'] == 5 and batch['bs'] == 1
    free = free_run(lib, case, dt)[0]
    assert torch.equal(batch['mkpts1_f'], free['mkpts1_f']) and torch.equal(batch['conf_matrix'], free['conf_matrix'])      # two runs: the same bits
    # M = 0: the threshold raised to 2 (a confidence is at most 1) -- no fine op runs, the fine key points ARE the empty coarse ones
    out = eng.run(px[0], px[1], thr=2.0)
    assert out['b_ids'].shape == (0,) and out['mkpts1_f'].shape == (0, 2) and out['expec_f'].shape == (0, 3) and out['mkpts0_f'] is out['mkpts0_c']
    assert out['mkpts1_f'] is out['mkpts1_c'] and torch.equal(out['conf_matrix'], free['conf_matrix'])
    # an all-zero pair (whatever it matches -- the position encoding alone separates the cells) runs without error
    out = eng.run(torch.zeros_like(px[0]), torch.zeros_like(px[1]))
    assert bool(torch.isfinite(out['conf_matrix']).all()) and out['mkpts1_f'].shape == (out['b_ids'].shape[0], 2) and bool(torch.isfinite(out['mkpts1_f']).all())
