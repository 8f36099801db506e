"""Loading a state dict is order-independent: an engine filled in the state dict's own order and one filled in reversed order hold the same slab,
so their outputs are bit-equal.  Several slots are filled by more than one tensor (qkv.w, the VAE's qk.w, ctx_kv.w, temb_proj.w, conv2.w with a
fused shortcut, the CLIP towers' qkv.w / qkv.b); a source of such a slot that cleared the slot before packing would wipe what an earlier tensor
left there, and no test that loads in state_dict() order would see it.  No tolerance: torch.equal."""
import importlib.util
import os

import pytest
import torch

from oracle import unet_oracle as U
from oracle import vae_oracle as V

HERE = os.path.dirname(os.path.abspath(__file__))


def _reversed(sd):
    out = dict(reversed(list(sd.items())))
    assert list(out) == list(sd)[::-1] and list(out)[0] != list(sd)[0]
    return out


def _unet(lib):
    """TINY's widths (320, 640) are multiples of 64: conv_shortcut lands in the tail columns of conv2's rows"""
    from mvedit_amd.unet import UNet2DConditionEngine
    cfg, dtype = U.TINY, torch.float16
    sd = {k: v.to(dtype) for k, v in U.make_state_dict(cfg, seed=1234).items()}
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, cfg['in_channels'], 16, 16, generator=g).to(dtype).cuda()
    ctx = torch.randn(2, 77, cfg['cross_attention_dim'], generator=g).to(dtype).cuda()
    return [(UNet2DConditionEngine.from_state_dict(d, cfg, dtype)(x, 499, ctx)[0],) for d in (sd, _reversed(sd))]


def _unet_unfused(lib):
    """the same network laid out with `.sc.w` slots of their own (mve_unet_tune(0) applies to handles created afterwards)"""
    tune = lib.raw('mve_unet_tune')
    assert tune(0) == 1
    try:
        return _unet(lib)
    finally:
        tune(1)


def _vae_decoder(lib):
    from mvedit_amd.vae import AutoencoderKLEngine
    cfg, dtype = V.TINY_VAE, torch.float16
    sd = {k: v.to(dtype) for k, v in V.random_params(cfg, 11).items()}
    z = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(4)).to(dtype).cuda()
    return [(AutoencoderKLEngine.from_state_dict(d, cfg, dtype).decode(z, return_dict=False)[0],) for d in (sd, _reversed(sd))]


def _clip_text(lib):
    from mvedit_amd.text_encoder import CLIPTextEngine
    spec = importlib.util.spec_from_file_location('make_clip_text_golden', os.path.join(HERE, 'golden', 'make_clip_text_golden.py'))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    sd = {k: torch.from_numpy(v).float() for k, v in G.make_weights('A').items()}
    ids = torch.from_numpy(G.make_ids('A', 0)).cuda()
    outs = []
    for d in (sd, _reversed(sd)):
        eng = CLIPTextEngine(G.config_dict('A'), dtype=torch.float16, device='cuda', with_projection=G.CASES['A']['with_projection'])
        eng.load_state_dict(d)
        o = eng(ids, output_hidden_states=True)
        outs.append((o.last_hidden_state, o.pooler_output) + tuple(o.hidden_states))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize('case', [_unet, _unet_unfused, _vae_decoder, _clip_text], ids=['unet_tiny', 'unet_tiny_unfused_shortcut', 'vae_decoder', 'clip_text_A'])
def test_loading_is_order_independent(lib, case):
    forward, backward = case(lib)
    assert len(forward) == len(backward)
    for a, b in zip(forward, backward):
        assert torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b)
