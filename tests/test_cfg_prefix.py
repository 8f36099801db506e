"""CFG prefix of the UNet executor (mve_unet_tune_cfg_prefix): under classifier-free guidance both halves of the batch carry the same
latents and timesteps, so the ops in front of the first cross-attention run for the first half alone whenever a device-side probe finds the halves
identical.  The launches are the full-batch problem's either way, so the criterion is exact: the engine with the switch on equals the same engine with it
off, bit for bit (torch.equal), for identical AND for distinct halves; cfg_prefix_state() tells which way the device decided.

Every switch-on run starts from a workspace filled with NaN patterns: a tensor whose second half the prefix neither computes nor broadcasts would
otherwise be read back correct from the switch-off run in front of it (same plan layout).
"""
import pytest
import torch

from oracle import unet_oracle as U

DTYPE = torch.float16


# ------------------------------------------------------------------------------------------------ CPU
def test_plan_is_the_same_with_the_switch_on_and_off(lib):
    from mvedit_amd.unet import SD15_CONFIG, UNet2DConditionEngine
    eng = UNet2DConditionEngine(SD15_CONFIG, DTYPE, device='cpu')
    assert eng.cfg_prefix is True                                   # on by default
    for B in (2, 64):
        seen = []
        for on in (True, False):
            eng.set_cfg_prefix(on)
            info = eng.plan(B, 64, 64, 77)
            seen.append((info['n_ops'], info['workspace_bytes'], info['flops'], [row[1:] for row in eng.op_table()], [row[0] for row in eng.op_table()]))
        assert seen[0] == seen[1]
    assert eng.set_cfg_prefix(True) is False                        # returns the previous setting
    eng.plan(2, 64, 64, 77)
    assert len(eng.op_table()) == 282


# ------------------------------------------------------------------------------------------------ GPU
_ENGINES = {}


def _engine(name):
    """one engine per synthetic network for the whole module (IP-Adapter weights loaded, adapter off)"""
    from mvedit_amd.unet import UNet2DConditionEngine
    if name not in _ENGINES:
        cfg = getattr(U, name)
        sd = {k: v.to(DTYPE).float() for k, v in U.make_state_dict(cfg, seed=21).items()}
        sd.update({k: v.to(DTYPE).float() for k, v in U.make_ip_state_dict(cfg).items()})
        _ENGINES[name] = UNet2DConditionEngine.from_state_dict(sd, cfg, DTYPE)
    eng = _ENGINES[name]
    eng.set_cfg_prefix(True)
    eng.set_residual_pair(True)
    eng.set_ip_adapter(0)
    return eng


def _cfg_batch(cfg, B, S, seed=0, ctx_len=77):
    """[uncond | text]: the latents of B / 2 views twice, one context per item"""
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B // 2, cfg['in_channels'], S, S, generator=g)
    ctx = torch.randn(B, ctx_len, cfg['cross_attention_dim'], generator=g)
    return torch.cat([lat, lat], 0).to(DTYPE).cuda(), ctx.to(DTYPE).cuda()


def _residuals(cfg, B, S, seed=3, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    ch = cfg['block_out_channels']
    shapes, s = [(ch[0], S, S)], S
    for i, c in enumerate(ch):
        shapes += [(c, s, s)] * cfg['layers_per_block']
        if i + 1 < len(ch):
            s //= 2
            shapes.append((c, s, s))
    return [scale * torch.randn(B, *sh, generator=g) for sh in shapes], scale * torch.randn(B, ch[-1], s, s, generator=g)


def _on_vs_off(eng, x, t, ctx, want_state, **kw):
    """switch off, then switch on over a poisoned workspace: equal bits; -> the output"""
    eng.set_cfg_prefix(False)
    off = eng(x, t, ctx, **kw)[0].clone()
    assert eng.cfg_prefix_state() == -1
    eng.set_cfg_prefix(True)
    eng._ws.fill_(0x7e)                                             # 0x7e7e: a NaN in fp16 and in bf16
    on = eng(x, t, ctx, **kw)[0].clone()
    state = eng.cfg_prefix_state()
    print(f'cfg_prefix_state={state} max|on - off|={(on.float() - off.float()).abs().max().item():.3e}')
    assert torch.isfinite(off).all()
    assert state == want_state
    assert torch.equal(on, off)
    return on


@pytest.mark.gpu
@pytest.mark.parametrize('pair', [True, False])
@pytest.mark.parametrize('name,B,S', [('TINY', 2, 16), ('TINY', 6, 16), ('SMALL', 4, 32), ('TINY', 6, 8)])
def test_identical_halves(lib, name, B, S, pair):
    """B = 2: one image per half (the K-slice decisions of M and M / 2 rows differ); B = 6: odd half; 8 x 8 at B = 6: 192 rows per half, a 256-row tile
    straddles the middle"""
    eng = _engine(name)
    eng.set_residual_pair(pair)
    x, ctx = _cfg_batch(getattr(U, name), B, S, seed=B + S)
    _on_vs_off(eng, x, 499, ctx, 1)


@pytest.mark.gpu
def test_predicate_false(lib):
    eng = _engine('TINY')
    x, ctx = _cfg_batch(U.TINY, 4, 16, seed=3)
    same = _on_vs_off(eng, x, 300, ctx, 1)
    x2 = x.clone()
    x2[-1, -1, -1, -1] += 1.0                                       # one element of the last image
    out = _on_vs_off(eng, x2, 300, ctx, 0)
    assert not torch.equal(out, same)
    t = torch.tensor([300.0, 300.0, 300.0, 301.0])                  # timesteps differ between the halves
    out = _on_vs_off(eng, x, t, ctx, 0)
    assert not torch.equal(out, same)
    _on_vs_off(eng, x, torch.tensor([300.0, 40.0, 300.0, 40.0]), ctx, 1)       # per-image timesteps, equal halves


@pytest.mark.gpu
def test_cross_image_pairing(lib):
    eng = _engine('TINY')
    x, ctx = _cfg_batch(U.TINY, 4, 16, seed=5)
    _on_vs_off(eng, x, 499, ctx, 1, cross_attention_kwargs=dict(num_cross_attn_imgs=2))
    # groups of two across the middle of a batch of two: not planned
    x, ctx = _cfg_batch(U.TINY, 2, 16, seed=5)
    eng(x, 499, ctx, cross_attention_kwargs=dict(num_cross_attn_imgs=2))
    assert eng.cfg_prefix_state() == -1


@pytest.mark.gpu
def test_controlnet_residuals_that_differ_between_the_halves(lib):
    eng = _engine('TINY')
    x, ctx = _cfg_batch(U.TINY, 2, 16, seed=6)
    down, mid = _residuals(U.TINY, 2, 16)
    assert not torch.equal(down[0][0], down[0][1])
    _on_vs_off(eng, x, 499, ctx, 1, down_block_additional_residuals=[d.to(DTYPE).cuda() for d in down], mid_block_additional_residual=mid.to(DTYPE).cuda())


@pytest.mark.gpu
def test_ip_adapter_tokens(lib):
    eng = _engine('TINY')
    eng.set_ip_adapter(16, 0.6)
    x, ctx = _cfg_batch(U.TINY, 2, 16, seed=7, ctx_len=77 + 16)
    _on_vs_off(eng, x, 250, ctx, 1)
    eng.set_ip_adapter(0)


@pytest.mark.gpu
def test_enc_dec_equals_the_one_pass_forward(lib):
    from mvedit_amd.unet import unet_dec
    eng = _engine('TINY')
    x, ctx = _cfg_batch(U.TINY, 2, 16, seed=8)
    full = _on_vs_off(eng, x, 321, ctx, 1)
    ws = torch.empty(eng.plan(2, 16, 16, 77, 1, True, DTYPE)['workspace_bytes'], dtype=torch.uint8, device='cuda').fill_(0x7e)
    st = eng.enc(x, 321, ctx, workspace=ws)
    assert eng.cfg_prefix_state() == 1
    two = unet_dec(eng, st, st, st, ctx)
    assert eng.cfg_prefix_state() == 1 and torch.equal(two, full)


@pytest.mark.gpu
def test_reference_attention_is_not_planned(lib):
    eng = _engine('TINY')
    x, ctx = _cfg_batch(U.TINY, 2, 16, seed=9)
    outs = []
    for on in (False, True):
        eng.set_cfg_prefix(on)
        d = {}
        eng(x, 300, ctx, cross_attention_kwargs=dict(mode='w', ref_dict=d, is_cfg_guidance=True))
        assert eng.cfg_prefix_state() == -1
        outs.append(eng(x, 300, ctx, cross_attention_kwargs=dict(mode='r', ref_dict=d, is_cfg_guidance=True))[0].clone())
        assert eng.cfg_prefix_state() == -1
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
def test_graph_replay_re_evaluates_the_flag(lib):
    eng = _engine('TINY')
    x, ctx = _cfg_batch(U.TINY, 2, 16, seed=10)
    t = torch.full((2,), 999.0, device='cuda')
    eager_same = eng(x, t, ctx)[0].clone()
    x_new = x.clone()
    x_new[1].mul_(0.5)
    eager_new = eng(x_new, t, ctx)[0].clone()
    assert eng.cfg_prefix_state() == 0 and not torch.equal(eager_new, eager_same)
    xs = x.clone()
    eng.enable_graph(True)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):                                      # eager, capture + launch, replay
                o = eng(xs, t, ctx)[0]
                assert torch.equal(o, eager_same) and eng.cfg_prefix_state() == 1
                del o                                               # the allocator hands the same block back: addresses repeat
            xs[1].mul_(0.5)                                         # same addresses, the second half changed in place
            o = eng(xs, t, ctx)[0].clone()
            assert eng.cfg_prefix_state() == 0
        side.synchronize()
    finally:
        eng.enable_graph(False)
    assert torch.equal(o, eager_new)
