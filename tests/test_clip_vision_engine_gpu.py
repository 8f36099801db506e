"""CLIPVisionEngine, ResamplerEngine and ImageProjEngine against the pinned references: transformers' own CLIPVisionModelWithProjection /
CLIPVisionModel and the reference's Resampler / ImageProjModel in float64 (tests/golden/make_clip_vision_golden.py -> clip_vision_ref.npz,
clip_vision_hidden_ref.npz; nothing here imports transformers or reads the reference tree).

Bar: an engine's rel-L2 against float64 is at most 1.5 x the error the golden records for the 16-bit CPU module (.half() / .bfloat16()) on the
same output -- the text engine's bar, for the same reason: the engine rounds at other points (fused bias and residual, fp32 softmax), so
equality is not expected and the factor absorbs summation order; a structural error (a wrong patch order, the class row in the wrong place, the
post norm applied to last_hidden_state, the wrong GELU) shows at 1e-1 or more.

Measured on an MI355X (engine / the 16-bit CPU module, rel-L2 against float64; R = Resampler, P = ImageProjModel):

    case  output              fp16 engine / module           bf16 engine / module
    A     hidden_states[0]    3.422e-04 / 3.422e-04          3.443e-03 / 3.800e-03
    A     hidden_states[1]    1.285e-03 / 1.327e-03          1.278e-02 / 1.449e-02
    A     hidden_states[2]    1.561e-03 / 1.624e-03          1.566e-02 / 1.756e-02
    A     last_hidden_state   1.561e-03 / 1.624e-03          1.566e-02 / 1.756e-02
    A     pooler_output       1.092e-03 / 1.263e-03          1.157e-02 / 1.743e-02
    A     image_embeds        1.134e-03 / 1.389e-03          1.278e-02 / 1.913e-02
    B     hidden_states[0]    3.378e-04 / 3.376e-04          3.409e-03 / 3.972e-03
    B     hidden_states[1]    9.658e-04 / 1.016e-03          9.710e-03 / 1.165e-02
    B     hidden_states[2]    1.050e-03 / 1.117e-03          1.041e-02 / 1.262e-02
    B     hidden_states[3]    1.103e-03 / 1.175e-03          1.081e-02 / 1.304e-02
    B     last_hidden_state   1.103e-03 / 1.175e-03          1.081e-02 / 1.304e-02
    B     pooler_output       1.761e-03 / 1.736e-03          1.167e-02 / 1.035e-02
    B     image_embeds        1.920e-03 / 1.806e-03          1.336e-02 / 1.242e-02
    C     hidden_states[0]    3.358e-04 / 3.358e-04          3.365e-03 / 3.880e-03
    C     hidden_states[1]    1.089e-03 / 1.124e-03          9.067e-03 / 9.829e-03
    C     hidden_states[2]    1.343e-03 / 1.423e-03          1.151e-02 / 1.287e-02
    C     last_hidden_state   1.343e-03 / 1.423e-03          1.151e-02 / 1.287e-02
    C     pooler_output       1.335e-03 / 1.361e-03          1.306e-02 / 1.188e-02
    R     tokens              1.037e-03 / 1.558e-03          1.086e-02 / 1.363e-02
    P     tokens              3.496e-04 / 3.496e-04          3.215e-03 / 3.720e-03

hidden_states[-2] is hidden_states[1] in cases A and C and hidden_states[2] in case B; hidden_states[-1] is last_hidden_state.  The worst ratio is
1.13 (bf16 B pooler_output), the best 0.66; hidden_states[0] (patch GEMM, embedding sum, pre_layrnorm) equals transformers' error in fp16 (ratio 1.00).
mve_attention alone at the new shapes (tests/test_clip_vision_kernels_gpu.py): fp16 2.25e-4 .. 2.28e-4 (bar 1e-3), bf16 1.80e-3 .. 1.83e-3 (bar 8e-3, on max|err| / max|ref| too).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_clip_vision_golden', os.path.join(HERE, 'golden', 'make_clip_vision_golden.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

OUTPUTS = ('image_embeds', 'last_hidden_state', 'penultimate', 'pooler_output')
_cache = {}


def golden():
    if 'npz' not in _cache:
        _cache['npz'] = (dict(np.load(G.REF)), dict(np.load(G.HIDDEN_REF)))
    return _cache['npz']


def engine(case, dtype):
    """one engine per (case, dtype), shared by the tests"""
    from mvedit_amd.vision_encoder import CLIPVisionEngine
    key = (case, dtype)
    if key not in _cache:
        sd = G.make_weights(case)
        assert G.digest(sd) == str(golden()[0][f'{case}.weights_sha256']), 'the regenerated weights are not the ones the golden was made with'
        eng = CLIPVisionEngine(G.config_dict(case), dtype=dtype, device='cuda', with_projection=G.CASES[case]['with_projection'])
        eng.load_state_dict({k: torch.from_numpy(v).float() for k, v in sd.items()})
        _cache[key] = eng
    return _cache[key]


def pixels(case):
    if ('px', case) not in _cache:
        px = G.make_pixels(case)
        assert G.digest({'pixel_values': px}) == str(golden()[0][f'{case}.pixels_sha256']), 'the regenerated pixels are not the ones the golden was made with'
        _cache[('px', case)] = torch.from_numpy(px).float()
    return _cache[('px', case)]


def rel_l2(a, ref):
    a, ref = a.double().cpu().numpy(), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize('dtype,tag', [(torch.float16, 'fp16'), (torch.bfloat16, 'bf16')])
@pytest.mark.parametrize('case', ['A', 'B', 'C'])
def test_engine_against_transformers_float64(case, dtype, tag):
    head, hidden = golden()
    eng, key = engine(case, dtype), f'{case}.'
    px = pixels(case)                                              # float32 in: the engine casts, as IPAdapter.get_image_embeds does itself
    out = eng(px.cuda(), output_hidden_states=True)
    last, pooled, embeds, hs = eng.run(px, output_hidden_states=True)
    got = dict(image_embeds=embeds, last_hidden_state=out.last_hidden_state, penultimate=out.hidden_states[-2], pooler_output=pooled)
    n = G.CASES[case]['num_hidden_layers'] + 1
    assert torch.equal(out.last_hidden_state, last) and len(out.hidden_states) == len(hs) == n
    assert out.last_hidden_state.shape == (G.CASES[case]['B'], G.n_tokens(case), G.CASES[case]['hidden_size']) and out.last_hidden_state.dtype == dtype
    assert torch.equal(out.hidden_states[-1], out.last_hidden_state)           # transformers: no post norm on last_hidden_state
    if G.CASES[case]['with_projection']:
        assert torch.equal(out[0], out.image_embeds) and torch.equal(out.image_embeds, embeds) and not hasattr(out, 'pooler_output')
        assert out.keys() == ['image_embeds', 'last_hidden_state', 'hidden_states']
    else:
        assert torch.equal(out[0], out.last_hidden_state) and torch.equal(out.pooler_output, pooled) and embeds is None
        assert out.keys() == ['last_hidden_state', 'pooler_output', 'hidden_states']
    # every hidden state, so that a fault is located by layer: held to 1.5 x transformers' own error on that hidden state
    failures = []
    theirs_hs = head[key + f'err_{tag}.hidden_states']
    for k in range(n):
        ref = head[key + 'last_hidden_state'] if k == n - 1 else head[key + 'penultimate'] if k == n - 2 else hidden[key + f'hidden_states.{k}']
        err = rel_l2(out.hidden_states[k], ref)
        print(f'{case} {tag} hidden_states[{k}]: engine {err:.3e}  transformers {float(theirs_hs[k]):.3e}  ratio {err / float(theirs_hs[k]):.2f}')
        if not err <= 1.5 * float(theirs_hs[k]):
            failures.append((f'hidden_states[{k}]', err, float(theirs_hs[k])))
    for o in OUTPUTS:
        if key + o not in head:
            continue
        err, theirs = rel_l2(got[o], head[key + o]), float(head[key + f'err_{tag}.' + o])
        print(f'{case} {tag} {o}: engine {err:.3e}  transformers {theirs:.3e}  ratio {err / theirs:.2f}')
        if not err <= 1.5 * theirs:
            failures.append((o, err, theirs))
    assert not failures, failures


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_batch_independence_determinism_and_tuple_form(dtype):
    eng = engine('A', dtype)
    px = pixels('A').cuda()
    out = eng(px, output_hidden_states=True)
    # an item's result does not depend on its neighbours: alone, and permuted
    for b in range(px.shape[0]):
        alone = eng(px[b:b + 1], output_hidden_states=True)
        assert torch.equal(alone.image_embeds[0], out.image_embeds[b]) and torch.equal(alone.last_hidden_state[0], out.last_hidden_state[b]), b
        assert all(torch.equal(x[0], y[b]) for x, y in zip(alone.hidden_states, out.hidden_states)), b
    perm = eng(px[[2, 0, 1]])
    assert torch.equal(perm.image_embeds, out.image_embeds[[2, 0, 1]]) and torch.equal(perm.last_hidden_state, out.last_hidden_state[[2, 0, 1]])
    # two runs agree bit for bit, and the tuple form carries the same tensors
    again = eng(px, output_hidden_states=True, return_dict=False)
    assert isinstance(again, tuple) and len(again) == 3
    assert torch.equal(again[0], out.image_embeds) and torch.equal(again[1], out.last_hidden_state) and all(torch.equal(x, y) for x, y in zip(again[2], out.hidden_states))
    short = eng(px, return_dict=False)
    assert len(short) == 2 and torch.equal(short[0], out.image_embeds)
    # pixel_values of any float dtype are cast to the engine's
    assert torch.equal(eng(px.double()).image_embeds, out.image_embeds) and torch.equal(eng(px.to(dtype)).image_embeds, out.image_embeds)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_hidden_state_0_is_the_pre_layrnorm_output(dtype):
    """Built by hand from the engine's own kernels' definitions: unfold, the patch GEMM in float64, the class row and the position table, then
    pre_layrnorm -- within a few 16-bit roundings of the engine's hidden_states[0]."""
    case = 'C'
    eng, sd, px = engine(case, dtype), G.make_weights(case), pixels(case)
    c = G.config_dict(case)
    P, C = c['patch_size'], c['hidden_size']
    x = px.to(dtype).double()
    rows = torch.nn.functional.unfold(x, kernel_size=P, stride=P).transpose(1, 2)                      # [B, G2, 3 P P]
    w = {k: torch.from_numpy(v).to(dtype).double() for k, v in sd.items()}
    em = 'vision_model.embeddings.'
    patch = rows @ w[em + 'patch_embedding.weight'].reshape(C, -1).T
    tok = torch.cat([w[em + 'class_embedding'].expand(x.shape[0], 1, C), patch], 1) + w[em + 'position_embedding.weight']
    ref = torch.nn.functional.layer_norm(tok, (C,), w['vision_model.pre_layrnorm.weight'], w['vision_model.pre_layrnorm.bias'], c['layer_norm_eps'])
    h0 = eng(px, output_hidden_states=True).hidden_states[0]
    err = rel_l2(h0, ref.numpy())
    eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8                                          # half an ulp, relative
    print(f'{dtype} hidden_states[0] against a float64 pre_layrnorm: {err:.3e} (unit roundoff {eps:.3e})')
    assert err <= 4 * eps            # three roundings (patch GEMM, embedding sum, LayerNorm output), the first amplified by the normalisation: 4 units, not sqrt(3)


def test_engine_refuses_what_it_does_not_implement_on_the_gpu_too():
    eng = engine('A', torch.float16)
    px = pixels('A').cuda()
    with pytest.raises(NotImplementedError, match='output_attentions'):
        eng(px, output_attentions=True)
    with pytest.raises(NotImplementedError, match='interpolate_pos_encoding'):
        eng(px, interpolate_pos_encoding=True)
    with pytest.raises(ValueError, match=r'\[B, 3, 112, 112\]'):
        eng(torch.zeros(1, 3, 224, 224, device='cuda'))
    assert eng.to('cuda') is eng and eng.to(torch.float16) is eng and eng.eval() is eng and eng.requires_grad_(False) is eng
    assert next(eng.parameters()).dtype == torch.float16 and next(eng.parameters()).is_cuda
    with pytest.raises(NotImplementedError):
        eng.to('cpu')
    from mvedit_amd.ip_adapter import ResamplerEngine
    with pytest.raises(NotImplementedError, match='dim_head'):
        ResamplerEngine(**dict(G.RESAMPLER, dim_head=32))


def _proj_engines(dtype):
    from mvedit_amd.ip_adapter import ImageProjEngine, ResamplerEngine
    if ('proj', dtype) not in _cache:
        head = golden()[0]
        rsd, psd = G.make_resampler_weights(), G.make_image_proj_weights()
        assert G.digest(rsd) == str(head['R.weights_sha256']) and G.digest(psd) == str(head['P.weights_sha256'])
        r = ResamplerEngine(dtype=dtype, **G.RESAMPLER).load_state_dict({k: torch.from_numpy(v).float() for k, v in rsd.items()})
        p = ImageProjEngine(dtype=dtype, **G.IMAGE_PROJ).load_state_dict({k: torch.from_numpy(v).float() for k, v in psd.items()})
        _cache[('proj', dtype)] = (r, p)
    return _cache[('proj', dtype)]


@pytest.mark.parametrize('dtype,tag', [(torch.float16, 'fp16'), (torch.bfloat16, 'bf16')])
def test_image_projection_engines_against_the_reference_float64(dtype, tag):
    head = golden()[0]
    r, p = _proj_engines(dtype)
    failures = []
    for name, eng, x in (('R', r, head['B.penultimate']), ('P', p, head['A.image_embeds'])):
        x = torch.from_numpy(x).cuda()
        out = eng(x)
        assert out.dtype == dtype and tuple(out.shape) == tuple(head[name + '.tokens'].shape)
        assert torch.equal(out, eng(x))                                                            # two runs agree
        if x.shape[0] > 1:
            assert torch.equal(eng(x[1:2])[0], out[1])                                             # an item does not depend on its neighbours
        err, theirs = rel_l2(out, head[name + '.tokens']), float(head[f'{name}.err_{tag}.tokens'])
        print(f'{name} {tag} tokens: engine {err:.3e}  reference module {theirs:.3e}  ratio {err / theirs:.2f}')
        if not err <= 1.5 * theirs:
            failures.append((name, err, theirs))
    two = torch.from_numpy(np.concatenate([head['B.penultimate'], head['B.penultimate'][:, ::-1].copy()])).cuda()
    both = r(two)
    assert torch.equal(both[0], r(two[:1])[0]) and torch.equal(both[1], r(two[1:])[0])             # Resampler: batch independence
    assert not failures, failures


def test_tower_to_resampler_to_unet_context_tail():
    """`image_encoder(pixels, output_hidden_states=True).hidden_states[-2] -> image_proj_model` gives [B, 16, 192] tokens that the UNet engine
    takes as the IP tail of encoder_hidden_states (shape and dtype; the UNet's IP branch has its own parity tests)."""
    from oracle import unet_oracle as U
    from mvedit_amd.unet import UNet2DConditionEngine
    dtype = torch.float16
    feats = engine('B', dtype)(pixels('B').cuda(), output_hidden_states=True).hidden_states[-2]
    assert feats.shape == (1, 257, 160)
    tokens = _proj_engines(dtype)[0](feats)
    assert tokens.shape == (1, 16, 192) and tokens.dtype == dtype and torch.isfinite(tokens.float()).all()
    cfg = dict(U.TINY, cross_attention_dim=192)
    sd = dict(U.make_state_dict(cfg, seed=8))
    sd.update(U.make_ip_state_dict(cfg))
    unet = UNet2DConditionEngine.from_state_dict(sd, cfg, dtype)
    unet.set_ip_adapter(16, 0.6)
    g = torch.Generator().manual_seed(3)
    text = torch.randn(1, 77, 192, generator=g).to(dtype).cuda()
    x = torch.randn(1, 4, 16, 16, generator=g).to(dtype).cuda()
    out = unet(x, 250, torch.cat([text, tokens], 1))[0]
    assert out.shape == x.shape and out.dtype == dtype and torch.isfinite(out.float()).all()
    other = unet(x, 250, torch.cat([text, torch.zeros_like(tokens)], 1))[0]
    assert not torch.equal(out, other)                                                              # the tokens reach the IP branch
