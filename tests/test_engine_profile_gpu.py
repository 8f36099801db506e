"""The timed run of every executor engine (`op_ms` of the C forwards: HIP events around each op, one loop for all nine engines), the ranged runs
(UNet phase 1 / phase 2, LPIPS forward / backward) and the hipGraph branch of mve_unet_forward, which go through the same loop.

For each engine: ONE profiled forward at the smallest configuration its own test uses; the per-op times cover every op of the plan, are finite
and not negative; and the outputs of the profiled run pass the comparison of the engine's own test, with that test's references, helpers and
tolerances (imported from it, not restated).  Timing values themselves are not held to anything."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import unet_oracle as U

pytestmark = pytest.mark.gpu


def _timed(ms, n_ops, lo=0, hi=None):
    """ms covers ops [lo, hi) of a plan of n_ops ops: those entries are finite and >= 0, the others are the zeros the array started with"""
    hi = n_ops if hi is None else hi
    ms = list(ms)
    assert len(ms) == n_ops and 0 <= lo < hi <= n_ops
    assert all(math.isfinite(m) and m >= 0 for m in ms[lo:hi]), ms[lo:hi]
    assert all(m == 0.0 for m in ms[:lo] + ms[hi:]), 'an entry outside the range the call covers was written'


# ---------------------------------------------------------------------------------------------------------------------------------------- UNet
@pytest.fixture(scope='module')
def unet(lib):
    """TINY fp16, the case of test_unet.test_engine_tiny: engine, inputs and both oracle outputs, computed once"""
    from test_unet import inputs, residuals
    from mvedit_amd.unet import UNet2DConditionEngine
    cfg, dtype = U.TINY, torch.float16
    sd = {k: v.to(dtype).float() for k, v in U.make_state_dict(cfg, seed=1234).items()}
    x, ctx = (t.to(dtype).float() for t in inputs(cfg, 2, 16))
    down, mid = residuals(cfg, 2, 16)
    down, mid = [d.to(dtype).float() for d in down], mid.to(dtype).float()
    with torch.no_grad():
        refs = (U.unet_forward(sd, cfg, x, 499, ctx, 1, None, None, q=U.quantizer(dtype)), U.unet_forward(sd, cfg, x, 499, ctx, 1, None, None))
    eng = UNet2DConditionEngine.from_state_dict(sd, cfg, dtype)
    return dict(eng=eng, x=x.half().cuda(), ctx=ctx.half().cuda(), down=[d.half().cuda() for d in down], mid=mid.half().cuda(), refs=refs)


def test_unet_profiled_forward(unet):
    from test_unet import _check
    eng, x, ctx = unet['eng'], unet['x'], unet['ctx']
    out, rows = eng.profile(x, 499, ctx)
    n_ops = eng.plan(2, 16, 16, 77)['n_ops']
    assert len(rows) == n_ops == len(eng.op_table())
    _timed([m for *_, m in rows], n_ops)
    _check(out, *unet['refs'])


def test_unet_two_phase_profile_keeps_absolute_op_indices(unet):
    """phase 1 then phase 2 on one workspace, both timed: each fills its own part of the [n_ops] array; the result is the one-call forward's,
    bit for bit (the comparison of test_unet.test_engine_enc_dec_equals_forward_and_fp32_io)"""
    eng, x, ctx, down, mid = (unet[k] for k in ('eng', 'x', 'ctx', 'down', 'mid'))
    full = eng(x, 321, ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid)[0]
    eng._set_attention(None, 2, 16, 16, 77)
    info = eng.plan(2, 16, 16, 77, 1, True, torch.float16)
    ws = torch.empty(info['workspace_bytes'], dtype=torch.uint8, device='cuda')
    table = eng.op_table()
    n_ops, n_forward = info['n_ops'], sum(1 for ph, *_ in table if ph == 1)
    assert 0 < n_forward < n_ops == len(table) and all(ph == 1 for ph, *_ in table[:n_forward])
    dummy = torch.zeros(8, dtype=torch.float16, device='cuda')           # phase 1 never reads the residuals (UNet2DConditionEngine._enc_dec)
    none, ms1 = eng._run(1, x, 321, ctx, 1, [dummy] * len(down), dummy, None, profile=True, workspace=ws)
    assert none is None
    _timed(ms1, n_ops, 0, n_forward)
    out, ms2 = eng._run(2, None, 321, ctx, 1, down, mid, None, profile=True, workspace=ws, shape=tuple(x.shape))
    _timed(ms2, n_ops, n_forward, n_ops)
    assert torch.equal(out, full)


def test_unet_graph_first_sighting_capture_replay(unet):
    """enable_graph on a side stream, three calls with the same plan and addresses: eager, capture + launch, replay -- each equal to the eager
    result bit for bit (the comparison of test_unet.test_engine_graph_replay_equals_eager), which itself passes the oracle comparison"""
    from test_unet import _check
    eng, ctx = unet['eng'], unet['ctx']
    xs = unet['x'].clone()
    t = torch.full((2,), 499.0, device='cuda')
    eager = eng(xs, t, ctx)[0].clone()
    _check(eager, *unet['refs'])
    assert eng.enable_graph(True) is False
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            outs = []
            for what in ('first sighting', 'capture', 'replay'):
                o = eng(xs, t, ctx)[0]
                outs.append(o.clone())                                           # kept, so that the only free block of this size is o's
                del o                                                            # the allocator hands the same block back: addresses repeat
                assert torch.equal(outs[-1], eager), what
        side.synchronize()
    finally:
        eng.enable_graph(False)


# ------------------------------------------------------------------------------------------------------------------------------- ControlNet
def test_controlnet_profiled_forward(lib):
    from test_controlnet import _case
    from test_unet import _rel
    from mvedit_amd.controlnet import ControlNetEngine
    cfg, dtype, B, S = U.TINY, torch.float16, 2, 16
    sd, x, ctx, cond = _case(cfg, B, S, 1)
    with torch.no_grad():
        d32, m32 = U.controlnet_forward(sd, cfg, x, 300, ctx, cond, 0.7)
        d16, m16 = U.controlnet_forward(sd, cfg, x, 300, ctx, cond, 0.7, q=U.quantizer(dtype))
    eng = ControlNetEngine.from_state_dict(sd, cfg, dtype)
    down, mid = eng.new_outputs(B, S, S)
    rows = eng.run(x.half().cuda(), 300, ctx.half().cuda(), cond.half().cuda(), 0.7, down, mid, False, profile=True)
    n_ops = eng.plan(B, S, S, 77)['n_ops']
    assert len(rows) == n_ops
    _timed([m for *_, m in rows], n_ops)
    for got, r16, r32 in zip(list(down) + [mid], list(d16) + [m16], list(d32) + [m32]):
        assert got.shape == r32.shape and got.dtype == dtype
        l2_16, mx_16 = _rel(got, r16)
        l2_32, _ = _rel(got, r32)
        emu, _ = _rel(r16, r32)
        assert l2_16 <= 3e-3 and mx_16 <= 6e-3, (l2_16, mx_16)
        assert l2_32 <= 1.05 * emu + 1e-4, (l2_32, emu)


# -------------------------------------------------------------------------------------------------------------------------------- VAE, SRVGG
def test_vae_halves_profiled(lib):
    from oracle import vae_oracle as V
    from test_vae import _check, _engine
    cfg, dtype = V.TINY_VAE, torch.float16
    eng, sd = _engine(cfg, dtype, 11)
    g = torch.Generator().manual_seed(4)
    z = torch.randn(3, 4, 16, 8, generator=g).to(dtype).float()
    x = (torch.rand(3, 3, 32, 16, generator=g) * 2 - 1).to(dtype).float()
    q = V.quantizer(dtype)
    with torch.no_grad():
        d32, d16 = V.decode(sd, cfg, z), V.decode(sd, cfg, z, q)
        m32, m16 = V.encode_moments(sd, cfg, x), V.encode_moments(sd, cfg, x, q)
    for half, inp, r16, r32, what in ((eng.decoder, z, d16, d32, 'decode'), (eng.encoder, x, m16, m32, 'encode moments')):
        out, prof = half.run(inp.to(dtype).cuda(), profile=True)
        n_ops = half.plan(3, inp.shape[2], inp.shape[3], dtype)['n_ops']
        assert len(prof) == 1 and len(prof[0]) == n_ops
        _timed([m for *_, m in prof[0]], n_ops)
        _check(out, r16, r32, dtype, what)


def test_srvgg_profiled_forward(lib):
    from oracle import srvgg_oracle as S
    from test_image_enhancer import CASES, GOLDEN, _rel
    from mvedit_amd import _lib
    from mvedit_amd.image_enhancer import SRVGGNetCompactEngine
    from mvedit_amd.ops import dt
    tag, dtype = 'small', torch.float16
    g, kw = np.load(GOLDEN), CASES[tag]
    sd = {k: v.to(dtype).float() for k, v in S.random_params(seed=7, **kw).items()}
    x = torch.from_numpy(g[f'{tag}_x']).to(dtype).float()
    with torch.no_grad():
        y32, y16 = S.forward(sd, x, kw['upscale']), S.forward(sd, x, kw['upscale'], q=lambda t: t.to(dtype).float())
    eng = SRVGGNetCompactEngine(3, 3, dtype=dtype, **kw).load_state_dict(sd)
    xg = x.to(dtype).cuda().contiguous()
    B, _, H, W = xg.shape
    info = eng.plan(B, H, W, dtype)                                      # the engine's __call__ has no profile switch: the C call, as it makes it
    ws = torch.empty(info['workspace_bytes'], dtype=torch.uint8, device='cuda')
    out = torch.empty(B, 3, H * kw['upscale'], W * kw['upscale'], dtype=dtype, device='cuda')
    ms = (ctypes.c_float * info['n_ops'])()
    _lib.call('mve_srvgg_forward', eng._h, _lib.ptr(xg), dt(dtype), B, H, W, _lib.ptr(out), _lib.ptr(ws), ws.numel(), ms, _lib.stream_ptr(xg.device))
    _timed(ms, info['n_ops'])
    assert out.shape == y32.shape and torch.isfinite(out).all()
    l2_16, mx_16 = _rel(out, y16)
    l2_32, _ = _rel(out, y32)
    emu, _ = _rel(y16, y32)
    assert l2_16 <= 3e-3 and mx_16 <= 6e-3, (l2_16, mx_16)
    assert l2_32 <= 1.05 * emu + 1e-4, (l2_32, emu)
    assert _rel(out, torch.from_numpy(g[f'{tag}_y']))[0] < 4e-3


# ------------------------------------------------------------------------------------------------------------------------------------- LPIPS
def test_lpips_forward_then_backward(lib):
    """no op_ms here: the two calls are the ranged runs [0, n_forward) and [n_forward, n_ops) of one plan.  The comparison, references and bars of
    test_lpips.test_forward_and_gradient_vs_oracle."""
    import torch.nn.functional as F
    from oracle import lpips_oracle as L
    from test_lpips import _case
    from mvedit_amd.lpips import LPIPSEngine
    dtype = torch.bfloat16
    sd, pred, target = _case()
    sdq = {k: v.to(dtype).float() for k, v in sd.items()}
    coef = torch.tensor([1.0, 0.5, 2.0])
    p32 = pred.to(dtype).float().requires_grad_(True)
    d32 = L.lpips(sdq, p32, target.to(dtype).float())
    (d32 * coef).sum().backward()
    ph = pred.to(dtype).requires_grad_(True)
    dh = L.lpips_half(sdq, ph, target, dtype)
    (dh * coef).sum().backward()
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()
    emu_loss, emu_grad = ((dh.detach() - d32.detach()).abs() / d32.detach()).max().item(), rel(ph.grad, p32.grad)
    eng = LPIPSEngine.from_state_dict(sdq, dtype)
    info = eng.plan(3, 32, 32)
    assert 0 < info['n_forward_ops'] < info['n_ops']
    pg = pred.to(dtype).float().cuda().requires_grad_(True)
    d = eng(pg, target.to(dtype).float().cuda())
    (d * coef.cuda()).sum().backward()
    err_loss = ((d.cpu() - d32.detach()).abs() / d32.detach()).max().item()
    err_grad = rel(pg.grad.cpu(), p32.grad)
    cos = F.cosine_similarity(pg.grad.cpu().flatten(), p32.grad.flatten(), dim=0).item()
    assert err_loss <= 1.25 * emu_loss + 2e-3
    assert err_grad <= 1.25 * emu_grad + 1e-2 and cos > 0.995


# ------------------------------------------------------------------------------------------------------------------- CLIP towers, Resampler
def _held(rows):
    """(name, engine error, 16-bit module error): the engine is held to 1.5 x the module's own error, as in the engines' tests"""
    bad = [(n, e, m) for n, e, m in rows if not e <= 1.5 * m]
    assert not bad, bad


def test_clip_text_profiled_forward(lib):
    import test_clip_text_engine_gpu as T
    case, i, dtype, tag = 'A', 0, torch.float16, 'fp16'
    head, hidden = T.golden()
    eng, key = T.engine(case, dtype), f'{case}.{i}.'
    ids = torch.from_numpy(head[key + 'ids'])
    last, pooled, embeds, hs, ms = eng.run(ids, output_hidden_states=True, profile=True)
    _timed(ms, eng.plan(*ids.shape)['n_ops'])
    n, theirs = len(hs), head[key + f'err_{tag}.hidden_states']
    rows = [(f'hidden_states[{k}]', T.rel_l2(hs[k], head[key + 'penultimate'] if k == n - 2 else hidden[key + f'hidden_states.{k}']), float(theirs[k])) for k in range(n)]
    got = dict(last_hidden_state=last, penultimate=hs[-2], pooler_output=pooled, text_embeds=embeds)
    rows += [(o, T.rel_l2(got[o], head[key + o]), float(head[key + f'err_{tag}.' + o])) for o in T.OUTPUTS if key + o in head]
    _held(rows)


def test_clip_vision_profiled_forward(lib):
    import test_clip_vision_engine_gpu as T
    case, dtype, tag = 'A', torch.float16, 'fp16'
    head, hidden = T.golden()
    eng, key, px = T.engine(case, dtype), f'{case}.', T.pixels(case)
    last, pooled, embeds, hs, ms = eng.run(px, output_hidden_states=True, profile=True)
    _timed(ms, eng.plan(px.shape[0])['n_ops'])
    n, theirs = len(hs), head[key + f'err_{tag}.hidden_states']
    ref = lambda k: head[key + 'last_hidden_state'] if k == n - 1 else head[key + 'penultimate'] if k == n - 2 else hidden[key + f'hidden_states.{k}']
    rows = [(f'hidden_states[{k}]', T.rel_l2(hs[k], ref(k)), float(theirs[k])) for k in range(n)]
    got = dict(image_embeds=embeds, last_hidden_state=last, penultimate=hs[-2], pooler_output=pooled)
    rows += [(o, T.rel_l2(got[o], head[key + o]), float(head[key + f'err_{tag}.' + o])) for o in T.OUTPUTS if key + o in head]
    _held(rows)


def test_resampler_profiled_forward(lib):
    import test_clip_vision_engine_gpu as T
    dtype, tag = torch.float16, 'fp16'
    head = T.golden()[0]
    r, _ = T._proj_engines(dtype)
    x = torch.from_numpy(head['B.penultimate']).cuda()
    out, ms = r.run(x, profile=True)
    _timed(ms, r.plan(x.shape[0], x.shape[1])['n_ops'])
    assert out.dtype == dtype and tuple(out.shape) == tuple(head['R.tokens'].shape)
    _held([('R', T.rel_l2(out, head['R.tokens']), float(head[f'R.err_{tag}.tokens']))])


# ------------------------------------------------------------------------------------------------------------------------------- DPT, LoFTR
def test_dpt_profiled_forward(lib):
    import test_dpt_normal_engine_gpu as T
    case, tag = 'A', 'fp16'
    g, eng = T.golden(), T.engine(case, tag)
    out, feats, ms = eng.run(T.pixels(case), output_features=True, profile=True)
    _timed(ms, eng.plan(T.pixels(case).shape[0])['n_ops'])
    rows = []
    for t in T.G.TAPS:
        got = feats[t].double().cpu().numpy()
        assert tuple(got.shape) == tuple(g[f'{case}.{t}.shape']), (t, got.shape)
        idx = T.G.sample_index(case, t, got.size)
        rows.append((t, T.G.rel_l2(np.ascontiguousarray(got).reshape(-1)[idx], g[f'{case}.{t}'].astype(np.float64)), float(g[f'{case}.err_{tag}.{t}'])))
    assert T.FACTOR == 1.5
    _held(rows)


def test_loftr_profiled_coarse_and_fine(lib):
    """one call, both plans timed: the coarse taps do not depend on the matches handed in, the fine taps are taken on the float64 matches (as
    test_loftr_engine_gpu.test_fine_stage_on_the_float64_matches does)"""
    import test_loftr_engine_gpu as T
    case, dt = 'A', 'fp16'
    g, px, eng = T.golden(), T.inputs(case)[1], T.engine(lib, case, dt)
    ids = tuple(torch.from_numpy(g[f'{case}/{k}']) for k in ('b_ids', 'i_ids', 'j_ids'))
    out, feats, ms = eng.run(px[0], px[1], coarse_matches=ids, output_features=True, profile=True)
    assert len(ms) == 2
    N, _, H, W = px[0].shape
    for phase, (table, times) in zip((1, 2), ms):
        n_ops = eng.plan(N, H, W, phase)['n_ops']
        assert len(table) == n_ops
        _timed(times, n_ops)
    _held(T.tap_errors(case, dt, T.COARSE, feats, out))
    _held(T.tap_errors(case, dt, T.FINE, feats, out))
    assert np.array_equal(out['mkpts1_c'].cpu().numpy().astype(np.float64), g[f'{case}/mkpts1_c'])
    assert float((out['mkpts1_f'] - out['mkpts1_c']).abs().max()) <= 4.0
