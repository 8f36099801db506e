"""CLIPTextEngine against the pinned reference: transformers' own CLIPTextModel / CLIPTextModelWithProjection in float64
(tests/golden/make_clip_text_golden.py -> clip_text_ref.npz, clip_text_hidden_ref.npz; nothing here imports transformers).

Bar: the engine's rel-L2 against float64 is at most 1.5 x the error the golden records for transformers' own .half() / .bfloat16() module on
the same output.  The engine rounds at other points (fused bias and residual, fp32 softmax), so equality is not expected and the factor
absorbs summation order; a structural error (wrong mask, the wrong GELU, pooling off by one) shows at 1e-1 or more.

Measured on an MI355X (engine / transformers' 16-bit module, rel-L2 against float64):

    case.input  output              fp16 engine / transformers     bf16 engine / transformers
    A.0         last_hidden_state   1.311e-3 / 1.386e-3            1.342e-2 / 1.516e-2
    A.0         hidden_states[-2]   1.058e-3 / 1.110e-3            1.096e-2 / 1.250e-2
    A.0         pooler_output       9.577e-4 / 9.492e-4            8.963e-3 / 1.136e-2
    B.0         last_hidden_state   1.037e-3 / 1.099e-3            9.840e-3 / 1.088e-2
    B.0         hidden_states[-2]   9.304e-4 / 9.924e-4            8.955e-3 / 9.920e-3
    B.0         pooler_output       9.697e-4 / 1.022e-3            1.100e-2 / 1.043e-2
    B.0         text_embeds         1.048e-3 / 1.122e-3            1.176e-2 / 1.125e-2
    B.1         last_hidden_state   1.206e-3 / 1.298e-3            1.110e-2 / 1.398e-2
    B.1         hidden_states[-2]   1.127e-3 / 1.212e-3            1.055e-2 / 1.304e-2
    B.1         pooler_output       1.487e-3 / 1.469e-3            1.715e-2 / 2.258e-2
    B.1         text_embeds         1.458e-3 / 1.468e-3            1.682e-2 / 2.157e-2

The worst ratio is 1.05 (bf16 B.0 pooler_output / text_embeds), the best 0.76; hidden_states[0] (the embedding sum) equals transformers' error
exactly (2.2e-4 fp16, 2.5e-3 bf16: the same single rounding), every later hidden state is 0.80 ... 0.95 of it.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_clip_text_golden', os.path.join(HERE, 'golden', 'make_clip_text_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

OUTPUTS = ('last_hidden_state', 'penultimate', 'pooler_output', 'text_embeds')
INPUTS = [('A', 0), ('B', 0), ('B', 1)]
_cache = {}


def golden():
    if 'npz' not in _cache:
        _cache['npz'] = (dict(np.load(G.REF)), dict(np.load(G.HIDDEN_REF)))
    return _cache['npz']


def engine(case, dtype):
    """one engine per (case, dtype), shared by the tests"""
    from mvedit_amd.text_encoder import CLIPTextEngine
    key = (case, dtype)
    if key not in _cache:
        sd = G.make_weights(case)
        assert G.weights_digest(sd) == str(golden()[0][f'{case}.weights_sha256']), 'the regenerated weights are not the ones the golden was made with'
        eng = CLIPTextEngine(G.config_dict(case), dtype=dtype, device='cuda', with_projection=G.CASES[case]['with_projection'])
        eng.load_state_dict({k: torch.from_numpy(v).float() for k, v in sd.items()})
        _cache[key] = eng
    return _cache[key]


def rel_l2(a, ref):
    a = a.double().cpu().numpy()
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize('dtype,tag', [(torch.float16, 'fp16'), (torch.bfloat16, 'bf16')])
@pytest.mark.parametrize('case,i', INPUTS)
def test_engine_against_transformers_float64(case, i, dtype, tag):
    head, hidden = golden()
    eng, key = engine(case, dtype), f'{case}.{i}.'
    ids = torch.from_numpy(head[key + 'ids'])
    out = eng(ids.cuda(), output_hidden_states=True)
    last, pooled, embeds, hs = eng.run(ids, output_hidden_states=True)
    got = dict(last_hidden_state=out.last_hidden_state, penultimate=out.hidden_states[-2], pooler_output=pooled, text_embeds=embeds)
    assert torch.equal(out.last_hidden_state, last) and len(out.hidden_states) == len(hs) == G.CASES[case]['num_hidden_layers'] + 1
    if G.CASES[case]['with_projection']:
        assert torch.equal(out[0], out.text_embeds) and torch.equal(out.text_embeds, embeds) and not hasattr(out, 'pooler_output')
    else:
        assert torch.equal(out[0], out.last_hidden_state) and torch.equal(out.pooler_output, pooled) and embeds is None
    assert torch.equal(out[-1][-2], out.hidden_states[-2])
    # every hidden state, so that a fault is located by layer: held to 1.5 x transformers' own error on that hidden state
    n, failures = len(hs), []
    theirs_hs = head[key + f'err_{tag}.hidden_states']
    for k in range(n):
        ref = head[key + 'penultimate'] if k == n - 2 else hidden[key + f'hidden_states.{k}']
        err = rel_l2(out.hidden_states[k], ref)
        print(f'{case}.{i} {tag} hidden_states[{k}]: engine {err:.3e}  transformers {float(theirs_hs[k]):.3e}')
        if not err <= 1.5 * float(theirs_hs[k]):
            failures.append((f'hidden_states[{k}]', err, float(theirs_hs[k])))
    for o in OUTPUTS:
        if key + o not in head:
            continue
        err, theirs = rel_l2(got[o], head[key + o]), float(head[key + f'err_{tag}.' + o])
        print(f'{case}.{i} {tag} {o}: engine {err:.3e}  transformers {theirs:.3e}  ratio {err / theirs:.2f}')
        if not err <= 1.5 * theirs:
            failures.append((o, err, theirs))
    assert not failures, failures


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_causality_batch_independence_and_clip_skip(dtype):
    head, _ = golden()
    eng = engine('A', dtype)
    ids = torch.from_numpy(head['A.0.ids']).cuda()
    out = eng(ids, output_hidden_states=True)
    # ids behind position p do not reach rows <= p
    for p in (0, 15, 16, 40):
        other = ids.clone()
        other[:, p + 1:] = torch.randint(1, 500, other[:, p + 1:].shape, generator=torch.Generator().manual_seed(p)).cuda()
        got = eng(other).last_hidden_state
        assert torch.equal(got[:, :p + 1], out.last_hidden_state[:, :p + 1]), p
        assert not torch.equal(got[:, p + 1:], out.last_hidden_state[:, p + 1:]), p
    # an item's result does not depend on its neighbours
    for b in range(ids.shape[0]):
        alone = eng(ids[b:b + 1], output_hidden_states=True)
        assert torch.equal(alone.last_hidden_state[0], out.last_hidden_state[b]) and torch.equal(alone.pooler_output[0], out.pooler_output[b]), b
        assert all(torch.equal(x[0], y[b]) for x, y in zip(alone.hidden_states, out.hidden_states)), b
    pair = eng(ids[[2, 0]])
    assert torch.equal(pair.last_hidden_state[0], out.last_hidden_state[2]) and torch.equal(pair.last_hidden_state[1], out.last_hidden_state[0])
    # diffusers' clip_skip path: the final norm applied by hand to a hidden state
    assert torch.equal(eng.text_model.final_layer_norm(out.hidden_states[-1]), out.last_hidden_state)
    # two runs agree, and the tuple form carries the same tensors
    again = eng(ids, output_hidden_states=True, return_dict=False)
    assert torch.equal(again[0], out.last_hidden_state) and torch.equal(again[1], out.pooler_output) and torch.equal(again[2][-2], out.hidden_states[-2])


def test_engine_refuses_what_it_does_not_implement_on_the_gpu_too():
    eng = engine('A', torch.float16)
    ids = torch.zeros(1, 8, dtype=torch.long, device='cuda')
    with pytest.raises(ValueError, match='vocab_size'):
        eng(torch.full((1, 8), 512, device='cuda'))
    with pytest.raises(NotImplementedError, match='attention_mask'):
        eng(ids, attention_mask=torch.tensor([[1, 1, 1, 1, 0, 0, 0, 0]], device='cuda'))
    assert eng(ids, attention_mask=torch.ones(1, 8, device='cuda')).last_hidden_state.shape == (1, 8, 128)
    assert eng.to('cuda') is eng and eng.to(torch.float16) is eng and eng.eval() is eng
    with pytest.raises(NotImplementedError):
        eng.to('cpu')
