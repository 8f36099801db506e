"""SamMaskDecoderEngine against the pinned reference: transformers' own prompt encoder + mask decoder in float64 (tests/golden/make_sam_decoder_golden.py
-> sam_decoder_ref.npz; nothing here imports transformers).

Bar: every tap, `low_res_masks` and `iou` sit within 4 x the error the golden records for torch's fp32 CPU module on the same tensor, with an absolute
floor of 2e-6 (rel-L2 against float64) -- the bar of LoFTR's fp32 kernels, against a reference that is not the code under test.  `iou` is pooled over
all cases into one vector (a case alone has 4 to 16 values).  Tensors of more than 8192 values are compared on the positions the golden stores.

Measured on an MI355X (engine / torch's fp32 CPU module, rel-L2 against float64):

    case  tap             engine / fp32 CPU module
    A     dense_pe        2.512e-07 / 2.329e-07
    A     tokens          1.082e-07 / 9.523e-08
    A     queries.0       3.309e-07 / 5.835e-07
    A     keys.0          2.188e-07 / 3.897e-07
    A     queries.1       3.850e-07 / 6.831e-07
    A     keys.1          2.752e-07 / 5.033e-07
    A     queries.final   3.344e-07 / 5.973e-07
    A     upscaled        3.442e-07 / 6.815e-07
    A     hyper_in        3.313e-07 / 5.761e-07
    A     low_res_masks   4.572e-07 / 8.225e-07
    B     dense_pe        3.965e-07 / 3.774e-07
    B     tokens          1.415e-07 / 1.367e-07
    B     queries.0       3.361e-07 / 6.022e-07
    B     keys.0          2.104e-07 / 3.765e-07
    B     queries.1       3.525e-07 / 6.608e-07
    B     keys.1          2.566e-07 / 5.072e-07
    B     queries.final   3.295e-07 / 6.066e-07
    B     upscaled        3.508e-07 / 6.887e-07
    B     hyper_in        3.583e-07 / 6.153e-07
    B     low_res_masks   5.567e-07 / 1.046e-06
    C     dense_pe        3.621e-07 / 3.459e-07
    C     tokens          1.509e-07 / 1.439e-07
    C     queries.0       3.363e-07 / 3.597e-07
    C     keys.0          2.004e-07 / 2.558e-07
    C     queries.1       3.285e-07 / 3.423e-07
    C     keys.1          2.374e-07 / 3.128e-07
    C     queries.final   2.864e-07 / 3.553e-07
    C     upscaled        2.656e-07 / 4.510e-07
    C     hyper_in        2.852e-07 / 3.273e-07
    C     low_res_masks   3.946e-07 / 5.347e-07
    all   iou             3.400e-07 / 1.249e-06 (the largest of the cases)

The worst ratio is 1.14 (tokens: sinf / cosf of arguments up to 40, where one fp32 rounding of the argument is the whole error); behind the first
GEMM the engine sits at 0.5 .. 0.95 of the module (the GEMM's two-level sum).  Binary low-res masks: 8192 of 8192 stored pixels agree in every case.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_sam_decoder_golden', os.path.join(HERE, 'golden', 'make_sam_decoder_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

FLOOR, FACTOR = 2e-6, 4.0
_cache = {}


def golden():
    if 'npz' not in _cache:
        _cache['npz'] = dict(np.load(G.REF))
    return _cache['npz']


def weights(case, variant=None):
    key = ('sd', case, variant)
    if key not in _cache:
        sd = G.make_weights(case, variant)
        if variant is None:
            assert G.digest(sd) == str(golden()[f'{case}.weights_sha256']), 'the regenerated weights are not the ones the golden was made with'
        _cache[key] = {k: torch.from_numpy(v).float() for k, v in sd.items()}
    return _cache[key]


def engine(case, layout='transformers', variant=None):
    """one engine per (case, key layout, weight variant), shared by the tests"""
    from mvedit_amd.sam import SamMaskDecoderEngine
    key = (case, layout, variant)
    if key not in _cache:
        sd = weights(case, variant)
        if layout == 'segment_anything':
            sd = G.segment_anything_keys(sd)
        _cache[key] = SamMaskDecoderEngine(G.config_dict(case), device='cuda').load_state_dict(sd)
    return _cache[key]


def inputs(case):
    if ('in', case) not in _cache:
        inp = G.make_inputs(case)
        assert G.digest(inp) == str(golden()[f'{case}.inputs_sha256']), 'the regenerated inputs are not the ones the golden was made with'
        t = lambda a, d: None if a is None else torch.from_numpy(np.asarray(a)).to(d)
        _cache[('in', case)] = dict(embedding=t(inp['embedding'], torch.float16), boxes=t(inp['boxes'], torch.float32), points=t(inp['points'], torch.float32),
                                    labels=t(inp['labels'], torch.int32))
    return _cache[('in', case)]


def run(case, multimask=True, taps=True, **kw):
    i = inputs(case)
    return engine(case, **kw).run(i['embedding'], i['boxes'], i['points'], i['labels'], multimask_output=multimask, output_taps=taps)


def taps_np(taps):
    """{tap: float64 array}, `low_res_masks` / `iou` with their [B, P] axes joined into the items the other taps (and the golden) count"""
    out = {k: v.double().cpu().numpy() for k, v in taps.items()}
    for k in ('low_res_masks', 'iou'):
        out[k] = out[k].reshape((-1,) + out[k].shape[2:])
    return out


def baseline(case):
    """the taps of one forward per case, computed once and left unchanged"""
    if ('taps', case) not in _cache:
        _cache[('taps', case)] = taps_np(run(case)[2])
    return _cache[('taps', case)]


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


@pytest.mark.parametrize('case', ['A', 'B', 'C'])
def test_taps_against_float64(case):
    ref, got = golden(), baseline(case)
    rows, bad = [], []
    for n in G.tap_names(case):
        if n == 'iou':
            continue
        assert tuple(ref[f'{case}.{n}.shape']) == got[n].shape, (n, got[n].shape)
        err = rel_l2(got[n].reshape(-1)[G.sample_index(case, n, got[n].size)], ref[f'{case}.{n}'])
        bar = max(FACTOR * float(ref[f'{case}.err_fp32.{n}']), FLOOR)
        rows.append(f'    {case}     {n:14s}  {err:.3e} / {float(ref[f"{case}.err_fp32.{n}"]):.3e}')
        if not err <= bar:
            bad.append((n, err, bar))
    print('\n'.join(rows))
    assert not bad, bad


def test_iou_pooled_over_all_cases():
    ref = golden()
    got = np.concatenate([baseline(c)['iou'].reshape(-1) for c in G.CASES])
    want = np.concatenate([ref[f'{c}.iou'].reshape(-1) for c in G.CASES])
    module = max(float(ref[f'{c}.err_fp32.iou']) for c in G.CASES)
    err = rel_l2(got, want)
    print(f'    all   iou             {err:.3e} / {module:.3e} (the largest of the cases)')
    assert err <= max(FACTOR * module, FLOOR), (err, module)


@pytest.mark.parametrize('case', ['A', 'B', 'C'])
def test_multimask_selection(case):
    """multimask_output=True keeps mask tokens 1.., False keeps token 0: slices, bit for bit, of the forward that test_taps_against_float64 holds to the golden
    (whose `low_res_masks` is the module's two outputs joined)"""
    full = baseline(case)
    for multi, sl in ((True, slice(1, None)), (False, slice(0, 1))):
        low, iou, taps = run(case, multimask=multi, taps=False)
        i = inputs(case)
        B, P = i['embedding'].shape[0], (i['boxes'] if i['boxes'] is not None else i['points']).shape[1]
        assert taps is None and low.shape[:2] == (B, P) and low.shape[2] == (3 if multi else 1)
        assert np.array_equal(low.double().cpu().numpy().reshape((B * P,) + tuple(low.shape[2:])), full['low_res_masks'][:, sl])
        assert np.array_equal(iou.double().cpu().numpy().reshape(B * P, -1), full['iou'][:, sl])


@pytest.mark.parametrize('case', ['A', 'B'])
def test_both_key_layouts_load_to_the_same_bits(case):
    a = baseline(case)
    b = taps_np(run(case, layout='segment_anything')[2])
    for n, t in b.items():
        assert np.array_equal(t, a[n]), n


@pytest.mark.parametrize('case', ['A', 'C'])
def test_two_runs_give_the_same_bits(case):
    a = baseline(case)
    b = taps_np(run(case)[2])
    assert sorted(b) == sorted(a)
    for n, t in b.items():
        assert np.array_equal(t, a[n]), n


def test_an_item_does_not_depend_on_batch_or_prompt_count():
    """case A has B = 2 images x P = 2 prompts: every item alone (B = 1, P = 1) gives the bits it has in the batch, and so does each image with its two prompts"""
    full, i, eng = baseline('A'), inputs('A'), engine('A')
    for b in range(2):
        low, iou, _ = eng.run(i['embedding'][b:b + 1], i['boxes'][b:b + 1], multimask_output=True)
        assert np.array_equal(low.double().cpu().numpy()[0], full['low_res_masks'][2 * b:2 * b + 2, 1:])
        for p in range(2):
            low, iou, taps = eng.run(i['embedding'][b:b + 1], i['boxes'][b:b + 1, p:p + 1], multimask_output=True, output_taps=True)
            n = 2 * b + p
            assert np.array_equal(low.double().cpu().numpy()[0, 0], full['low_res_masks'][n, 1:])
            assert np.array_equal(iou.double().cpu().numpy()[0, 0], full['iou'][n, 1:])
            assert np.array_equal(taps['queries.final'].double().cpu().numpy()[0], full['queries.final'][n])


@pytest.mark.parametrize('case,variant', [(c, v) for c in G.CASES for v in G.variants(c)])
def test_weight_variants_move_the_masks_as_float64_does(case, variant):
    """no_mask_embed zeroed / the two box-corner embeddings swapped: the engine lands on the float64 module's masks for the changed weights (the same bar),
    which the golden records to be 0.26 .. 0.67 away from the unchanged ones"""
    ref, base = golden(), baseline(case)
    got = taps_np(run(case, variant=variant)[2])['low_res_masks']
    idx = G.sample_index(case, 'low_res_masks', got.size)
    err = rel_l2(got.reshape(-1)[idx], ref[f'{case}.{variant}.low_res_masks'])
    assert err <= max(FACTOR * float(ref[f'{case}.{variant}.err_fp32']), FLOOR), err
    moved, want = rel_l2(got, base['low_res_masks']), float(ref[f'{case}.{variant}.change'])
    assert want > 1e-3 and abs(moved - want) <= 1e-4 * want, (moved, want)


@pytest.mark.parametrize('case', ['A', 'B', 'C'])
def test_binary_masks_recorded(case):
    """recorded, not asserted: pixels on which `low_res > 0` agrees / differs with the float64 module (on the stored positions)"""
    ref, got = golden(), baseline(case)['low_res_masks']
    idx = G.sample_index(case, 'low_res_masks', got.size)
    a, b = got.reshape(-1)[idx] > 0, ref[f'{case}.low_res_masks'] > 0
    print(f'    {case}     binary masks: {int((a == b).sum())} agree, {int((a != b).sum())} differ of {a.size}')
