"""DPTNormalEngine on an MI355X against the float64 golden (tests/golden/make_dpt_normal_golden.py: transformers' DPTModel + neck, the reference's
own decoder and head on the same weights).

The bar, for every tap and the output, in fp16 and bf16: rel-L2 against float64 <= 1.5 x the stored error of the 16-bit CPU module on that tap
(the project's standing bar for pinned third-party networks).  A tap of more than 8192 values is compared on the positions the golden stores
(`G.sample_index`); the module's error was measured on the same positions.  The engine rounds at other points than the module (fused epilogues,
weights standardised in float64 and rounded once, fp32 softmax), so equality is not expected; a structural error (padding on the wrong side, the
shortcut's norm activated, a misplaced class row) shows at 1e-1 or more.

Measured on an MI355X (engine rel-L2 / 16-bit module rel-L2 = ratio; the table is filled by `test_every_tap_is_within_the_module_bar`, which
prints it):

    A fp16 stem     engine 3.683e-04  module 7.387e-04  ratio 0.50
    A fp16 stage1   engine 1.880e-03  module 3.368e-03  ratio 0.56
    A fp16 stage2   engine 3.117e-03  module 5.567e-03  ratio 0.56
    A fp16 stage3   engine 6.023e-03  module 1.061e-02  ratio 0.57
    A fp16 tokens3  engine 4.588e-03  module 7.790e-03  ratio 0.59
    A fp16 tokens4  engine 4.616e-03  module 7.736e-03  ratio 0.60
    A fp16 fusion4  engine 3.833e-03  module 6.724e-03  ratio 0.57
    A fp16 fusion3  engine 4.097e-03  module 7.766e-03  ratio 0.53
    A fp16 fusion2  engine 3.137e-03  module 6.609e-03  ratio 0.47
    A fp16 fusion1  engine 3.601e-03  module 7.803e-03  ratio 0.46
    A fp16 output   engine 4.974e-03  module 1.127e-02  ratio 0.44
    A bf16 stem     engine 3.344e-03  module 5.731e-03  ratio 0.58
    A bf16 stage1   engine 1.662e-02  module 2.741e-02  ratio 0.61
    A bf16 stage2   engine 2.684e-02  module 4.378e-02  ratio 0.61
    A bf16 stage3   engine 5.133e-02  module 8.664e-02  ratio 0.59
    A bf16 tokens3  engine 3.827e-02  module 6.009e-02  ratio 0.64
    A bf16 tokens4  engine 3.775e-02  module 6.008e-02  ratio 0.63
    A bf16 fusion4  engine 3.670e-02  module 5.135e-02  ratio 0.71
    A bf16 fusion3  engine 3.993e-02  module 6.020e-02  ratio 0.66
    A bf16 fusion2  engine 3.242e-02  module 5.257e-02  ratio 0.62
    A bf16 fusion1  engine 3.573e-02  module 6.006e-02  ratio 0.60
    A bf16 output   engine 3.732e-02  module 6.623e-02  ratio 0.56
    B fp16 stem     engine 3.346e-04  module 7.289e-04  ratio 0.46
    B fp16 stage1   engine 1.320e-03  module 2.925e-03  ratio 0.45
    B fp16 stage2   engine 2.849e-03  module 6.158e-03  ratio 0.46
    B fp16 stage3   engine 4.611e-03  module 9.813e-03  ratio 0.47
    B fp16 tokens3  engine 6.439e-03  module 1.340e-02  ratio 0.48
    B fp16 tokens4  engine 6.164e-03  module 1.285e-02  ratio 0.48
    B fp16 fusion4  engine 5.823e-03  module 1.264e-02  ratio 0.46
    B fp16 fusion3  engine 4.413e-03  module 8.350e-03  ratio 0.53
    B fp16 fusion2  engine 4.677e-03  module 8.054e-03  ratio 0.58
    B fp16 fusion1  engine 4.906e-03  module 7.228e-03  ratio 0.68
    B fp16 output   engine 1.205e-02  module 1.505e-02  ratio 0.80
    B bf16 stem     engine 3.080e-03  module 5.443e-03  ratio 0.57
    B bf16 stage1   engine 1.172e-02  module 2.277e-02  ratio 0.51
    B bf16 stage2   engine 2.408e-02  module 4.638e-02  ratio 0.52
    B bf16 stage3   engine 3.605e-02  module 7.286e-02  ratio 0.49
    B bf16 tokens3  engine 4.855e-02  module 9.619e-02  ratio 0.50
    B bf16 tokens4  engine 4.653e-02  module 9.155e-02  ratio 0.51
    B bf16 fusion4  engine 3.398e-02  module 6.599e-02  ratio 0.51
    B bf16 fusion3  engine 2.913e-02  module 5.388e-02  ratio 0.54
    B bf16 fusion2  engine 2.832e-02  module 5.462e-02  ratio 0.52
    B bf16 fusion1  engine 2.653e-02  module 5.363e-02  ratio 0.49
    B bf16 output   engine 7.341e-02  module 1.412e-01  ratio 0.52

No tap needs more than 0.80 x the module's error.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_dpt_normal_golden', os.path.join(HERE, 'golden', 'make_dpt_normal_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

FACTOR = 1.5
DTYPES = {'fp16': torch.float16, 'bf16': torch.bfloat16}
_cache = {}


def golden():
    if 'golden' not in _cache:
        _cache['golden'] = dict(np.load(G.REF))
    return _cache['golden']


def weights(case):
    if ('w', case) not in _cache:
        sd = G.make_weights(case)
        assert G.digest(sd) == str(golden()[f'{case}.weights_sha256']), 'the regenerated weights are not the ones the golden was made with'
        _cache[('w', case)] = {k: torch.from_numpy(v).float() for k, v in sd.items()}
    return _cache[('w', case)]


def pixels(case):
    if ('px', case) not in _cache:
        px = G.make_pixels(case)
        assert G.digest({'pixels': px}) == str(golden()[f'{case}.pixels_sha256']), 'the regenerated pixels are not the ones the golden was made with'
        _cache[('px', case)] = torch.from_numpy(px).float()
    return _cache[('px', case)]


def engine(case, tag):
    if ('eng', case, tag) not in _cache:
        from mvedit_amd.normal_model import DPTNormalEngine
        _cache[('eng', case, tag)] = DPTNormalEngine(G.engine_config(case), dtype=DTYPES[tag], device='cuda').load_state_dict(weights(case))
    return _cache[('eng', case, tag)]


def forward(case, tag):
    if ('out', case, tag) not in _cache:
        _cache[('out', case, tag)] = engine(case, tag).run(pixels(case), output_features=True)
    return _cache[('out', case, tag)]


def reference_layout(case):
    """The case's weights under the reference checkpoint's key names (plus the keys that checkpoint carries and the engine drops)."""
    from mvedit_amd.normal_model import key_table
    cfg = G.engine_config(case)
    tr, ref = key_table(cfg, 'transformers'), key_table(cfg, 'reference')
    w = weights(case)
    sd = {}
    for logical, key in ref.items():
        if logical.endswith(('.q.weight', '.q.bias', '.k.weight', '.k.bias', '.v.weight', '.v.bias')) or '?' in logical:
            continue
        if '.qkv.' in logical:          # timm fuses q | k | v into one Linear(C, 3C)
            sd[key] = torch.cat([w[tr[logical.replace('.qkv.', f'.{n}.')]] for n in 'qkv'], 0)
        else:
            sd[key] = w[tr[logical]]
    return sd


@pytest.mark.parametrize('tag', ['fp16', 'bf16'])
@pytest.mark.parametrize('case', ['A', 'B'])
def test_every_tap_is_within_the_module_bar(case, tag):
    g = golden()
    out, feats = forward(case, tag)
    lines, worst = [], []
    for t in G.TAPS:
        got = feats[t].double().cpu().numpy()
        assert tuple(got.shape) == tuple(g[f'{case}.{t}.shape']), (t, got.shape)
        ref = g[f'{case}.{t}'].astype(np.float64)
        idx = G.sample_index(case, t, got.size)
        err = G.rel_l2(np.ascontiguousarray(got).reshape(-1)[idx], ref)
        bar = float(g[f'{case}.err_{tag}.{t}'])
        lines.append(f'    {case} {tag} {t:8s} engine {err:.3e}  module {bar:.3e}  ratio {err / bar:.2f}')
        if not err <= FACTOR * bar:
            worst.append(lines[-1])
    print('\n' + '\n'.join(lines))
    assert not worst, 'taps over 1.5 x the 16-bit module error:\n' + '\n'.join(worst)


@pytest.mark.parametrize('tag', ['fp16', 'bf16'])
@pytest.mark.parametrize('case', ['A', 'B'])
def test_output_shape_dtype_sign_and_call(case, tag):
    c = G.CASES[case]
    out, feats = forward(case, tag)
    S = c['image_size']
    assert tuple(out.shape) == ((c['B'], S, S) if c['num_channels'] == 1 else (c['B'], c['num_channels'], S, S))      # num_channels 1: dimension 1 squeezed
    assert out.dtype == DTYPES[tag] and out.device.type == 'cuda' and feats['output'] is out
    assert bool((out >= 0).all()) and bool(torch.isfinite(out).all()) and float((out > 0).float().mean()) > 0.2      # the trailing ReLU
    again = engine(case, tag)(pixels(case))
    assert torch.equal(again, out), '__call__ and run differ'
    assert torch.equal(engine(case, tag).run(pixels(case)), out)


@pytest.mark.parametrize('case', ['A', 'B'])
def test_reference_and_transformers_layouts_load_to_the_same_bits(case):
    from mvedit_amd.normal_model import DPTNormalEngine, detect_layout
    sd = reference_layout(case)
    assert detect_layout(sd) == 'reference' and detect_layout(weights(case)) == 'transformers'
    eng = DPTNormalEngine(G.engine_config(case), dtype=torch.float16, device='cuda').load_state_dict(sd)
    out, _ = forward(case, 'fp16')
    assert torch.equal(eng(pixels(case)), out)
