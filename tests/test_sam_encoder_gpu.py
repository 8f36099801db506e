"""SamImageEncoderEngine against the pinned reference: transformers' own SamVisionEncoder in float64 (tests/golden/make_sam_encoder_golden.py ->
sam_encoder_ref.npz; nothing here imports transformers).

Bar: the engine's rel-L2 against float64 is at most 1.5 x the error the golden records for the 16-bit CPU module (.half() / .bfloat16()) on the same
tensor -- the project's bar for pinned third-party networks: the engine rounds at other points (fused bias and residual, fp32 softmax and bias,
an unrounded q scale), so equality is not expected and the factor absorbs summation order; a structural error (a wrong window order, pad tokens
left out of the keys, a swapped or dropped bias term, a wrong table row) shows at 1e-1 or more.  Tensors of more than 8192 values are compared on
the positions the golden stores.

Measured on an MI355X (engine / the 16-bit CPU module, rel-L2 against float64):

    case  tensor              fp16 engine / module           bf16 engine / module
    A     hidden_states[0]    2.773e-04 / 2.773e-04          3.044e-03 / 3.081e-03
    A     hidden_states[1]    9.453e-04 / 1.358e-03          9.682e-03 / 1.323e-02
    A     hidden_states[2]    1.030e-03 / 1.423e-03          1.033e-02 / 1.386e-02
    A     hidden_states[3]    1.093e-03 / 1.504e-03          1.100e-02 / 1.456e-02
    A     neck                1.152e-03 / 1.544e-03          1.151e-02 / 1.506e-02
    B     hidden_states[0]    2.690e-04 / 2.690e-04          2.954e-03 / 2.984e-03
    B     hidden_states[1]    7.113e-04 / 9.569e-04          7.424e-03 / 9.630e-03
    B     hidden_states[2]    7.769e-04 / 1.021e-03          8.003e-03 / 1.022e-02
    B     hidden_states[3]    7.618e-04 / 9.795e-04          7.722e-03 / 9.687e-03
    B     hidden_states[4]    8.566e-04 / 1.059e-03          8.235e-03 / 1.019e-02
    B     neck                8.973e-04 / 1.066e-03          8.904e-03 / 1.092e-02

The worst ratio is 1.00 (hidden_states[0]: patch GEMM and the position add round where transformers rounds), every other tensor sits at 0.70 .. 0.84
(the module rounds q * scale, the bias and the softmax to 16 bit; the engine keeps them in fp32).  Block 1 (A) / 3 (B) is the global one.  With the
two tables zeroed the neck output moves by 2.98e-1 (A) / 1.79e-1 (B), in the engine as in transformers' float64 module.
mve_attention_relpos alone (tests/test_sam_kernels_gpu.py): fp16 2.23e-4 .. 2.25e-4 (bar 1e-3), bf16 1.77e-3 .. 1.78e-3 (bar 8e-3, on max|err| / max|ref| too).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_sam_encoder_golden', os.path.join(HERE, 'golden', 'make_sam_encoder_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

_cache = {}


def golden():
    if 'npz' not in _cache:
        _cache['npz'] = dict(np.load(G.REF))
    return _cache['npz']


def weights(case):
    if ('sd', case) not in _cache:
        sd = G.make_weights(case)
        assert G.digest(sd) == str(golden()[f'{case}.weights_sha256']), 'the regenerated weights are not the ones the golden was made with'
        _cache[('sd', case)] = {k: torch.from_numpy(v).float() for k, v in sd.items()}
    return _cache[('sd', case)]


def engine(case, dtype, layout='transformers'):
    """one engine per (case, dtype, key layout), shared by the tests"""
    from mvedit_amd.sam import SamImageEncoderEngine
    key = (case, dtype, layout)
    if key not in _cache:
        sd = weights(case)
        if layout == 'segment_anything':
            sd = {'image_encoder.' + k: v for k, v in G.segment_anything_keys(sd).items()}
        elif layout == 'zero tables':
            sd = {k: (torch.zeros_like(v) if 'rel_pos' in k else v) for k, v in sd.items()}
        _cache[key] = SamImageEncoderEngine(G.config_dict(case), dtype=dtype, device='cuda').load_state_dict(sd)
    return _cache[key]


def pixels(case):
    if ('px', case) not in _cache:
        px = G.make_pixels(case)
        assert G.digest({'pixel_values': px}) == str(golden()[f'{case}.pixels_sha256']), 'the regenerated pixels are not the ones the golden was made with'
        _cache[('px', case)] = torch.from_numpy(px).float()
    return _cache[('px', case)]


def outputs(case, dtype):
    """(neck, hidden states) of the case's batch, computed once per (case, dtype)"""
    key = ('out', case, dtype)
    if key not in _cache:
        _cache[key] = engine(case, dtype).run(pixels(case), output_hidden_states=True)
    return _cache[key]


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize('dtype,tag', [(torch.float16, 'fp16'), (torch.bfloat16, 'bf16')])
@pytest.mark.parametrize('case', ['A', 'B'])
def test_engine_against_transformers_float64(case, dtype, tag):
    ref, c = golden(), G.config_dict(case)
    B, Gd = G.CASES[case]['B'], G.grid(case)
    neck, hs = outputs(case, dtype)
    assert neck.shape == (B, 256, Gd, Gd) and neck.dtype == dtype and len(hs) == c['num_hidden_layers'] + 1
    assert all(h.shape == (B, Gd, Gd, c['hidden_size']) and h.dtype == dtype for h in hs)
    assert torch.equal(engine(case, dtype)(pixels(case).cuda()), neck)                   # ImageEncoderViT.forward: the embedding alone
    theirs = list(ref[f'{case}.err_{tag}.hidden_states']) + [float(ref[f'{case}.err_{tag}.neck'])]
    failures = []
    for name, t, their in zip(G.tensor_names(case), list(hs) + [neck], theirs):
        assert tuple(ref[f'{case}.{name}.shape']) == tuple(t.shape), name
        got = t.double().cpu().numpy().reshape(-1)[G.sample_index(case, name, t.numel())]
        err = rel_l2(got, ref[f'{case}.{name}'])
        print(f'{case} {tag} {name}: engine {err:.3e}  transformers {float(their):.3e}  ratio {err / float(their):.2f}')
        if not err <= 1.5 * float(their):
            failures.append((name, err, float(their)))
    assert not failures, failures


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('case', ['A', 'B'])
def test_both_key_layouts_load_to_the_same_bits(case, dtype):
    neck, hs = outputs(case, dtype)
    other, ohs = engine(case, dtype, 'segment_anything').run(pixels(case), output_hidden_states=True)
    assert torch.equal(other, neck) and all(torch.equal(a, b) for a, b in zip(ohs, hs))


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_determinism_and_batch_independence(dtype):
    eng, px = engine('A', dtype), pixels('A').cuda()
    neck, hs = outputs('A', dtype)
    again, ahs = eng.run(px, output_hidden_states=True)
    assert torch.equal(again, neck) and all(torch.equal(a, b) for a, b in zip(ahs, hs))      # two runs agree bit for bit
    for b in range(px.shape[0]):                                                             # an item alone, and the batch reversed
        alone, lhs = eng.run(px[b:b + 1], output_hidden_states=True)
        assert torch.equal(alone[0], neck[b]) and all(torch.equal(x[0], y[b]) for x, y in zip(lhs, hs)), b
    assert torch.equal(eng(px.flip(0)), neck.flip(0))
    assert torch.equal(eng(px.double()), neck) and torch.equal(eng(px.to(dtype)), neck)      # pixels of any float dtype are cast to the engine's


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('case', ['A', 'B'])
def test_the_relative_position_bias_is_live(case, dtype):
    """With rel_pos_h / rel_pos_w zeroed the engine's output moves as far as transformers' own does (the golden records that change in float64):
    the tables reach the kernel, in windowed and global blocks alike.  The band: both differences are taken between outputs that carry a 16-bit
    error of at most 1.5e-2 of the output's norm, against a change of 1.8e-1 .. 3.0e-1 -- under a fifth of it; a kernel that used one table of the
    two, or the tables of the wrong block, would land far outside."""
    neck, hs = outputs(case, dtype)
    flat, fhs = engine(case, dtype, 'zero tables').run(pixels(case), output_hidden_states=True)
    assert torch.equal(fhs[0], hs[0])                                                        # nothing in front of block 0 reads a table
    assert all(not torch.equal(a, b) for a, b in zip(fhs[1:], hs[1:])) and not torch.equal(flat, neck)
    change, want = rel_l2(flat.double().cpu().numpy(), neck.double().cpu().numpy()), float(golden()[f'{case}.neck_change_without_tables'])
    print(f'{case} {dtype}: neck changes by {change:.3e} without the tables (transformers float64: {want:.3e})')
    assert 0.8 * want <= change <= 1.25 * want


def test_engine_refuses_on_the_gpu_too():
    eng = engine('A', torch.float16)
    with pytest.raises(NotImplementedError, match='output_attentions'):
        eng(pixels('A').cuda(), output_attentions=True)
    with pytest.raises(ValueError, match=r'\[B, 3, 256, 256\]'):
        eng(torch.zeros(1, 3, 320, 320, device='cuda'))
    assert eng.to('cuda') is eng and eng.to(torch.float16) is eng and eng.eval() is eng and eng.img_size == 256
    assert next(eng.parameters()).dtype == torch.float16 and next(eng.parameters()).is_cuda
    with pytest.raises(NotImplementedError):
        eng.to('cpu')
