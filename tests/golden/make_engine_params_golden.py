"""Golden for the parameter layout of the nine executor engines: everything a handle reports about its slab before a tensor is loaded.

    python tests/golden/make_engine_params_golden.py         (host only: layouts are made without a GPU; writes tests/golden/engine_params.json)

The layout is pure host work, so a change that is meant to leave every slot where it is (a refactor of the layout or of the loader) regenerates
nothing: tests/test_engine_params.py calls `build_cases()` below on the current tree and asks for exact equality with the file recorded BEFORE the
change.  Run this script only on a commit whose layout is the intended one (a new slot, a new engine, a renamed state-dict key).

One entry per case, from a handle created with device='cpu' and nothing loaded: `weight_bytes` (mve_unet_weight_bytes: the slab size, which moves
when any slot's size, order or padding does), `missing` (the count mve_unet_missing_params answers: the number of required state-dict names) and
`first_missing` (the first of them in the layout's order).
"""
import ctypes
import json
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'engine_params.json')


def _entry(lib, handle):
    buf = ctypes.create_string_buffer(256)
    missing = lib.raw('mve_unet_missing_params')(handle, buf, 256)
    return dict(weight_bytes=int(lib.raw('mve_unet_weight_bytes')(handle)), missing=int(missing), first_missing=buf.value.decode())


def build_cases():
    """{case name: entry} from the library of the tree this file lies in."""
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    from mvedit_amd import _lib as lib
    from mvedit_amd.controlnet import ControlNetEngine
    from mvedit_amd.image_enhancer import SRVGGNetCompactEngine
    from mvedit_amd.ip_adapter import ResamplerEngine
    from mvedit_amd.lpips import LPIPSEngine
    from mvedit_amd.matcher import LoFTREngine
    from mvedit_amd.normal_model import DPTNormalEngine
    from mvedit_amd.text_encoder import CLIPTextEngine
    from mvedit_amd.unet import SD15_CONFIG, SDXL_CONFIG, UNet2DConditionEngine
    from mvedit_amd.vae import AutoencoderKLEngine
    from mvedit_amd.vision_encoder import CLIPVisionEngine
    from oracle import unet_oracle as U
    import make_clip_text_golden as GT
    import make_clip_vision_golden as GV
    import make_dpt_normal_golden as GD
    f16 = torch.float16
    cases = {}
    keep = []                                               # the handles live until every entry is read

    def add(name, eng):
        keep.append(eng)
        cases[name] = _entry(lib, eng._h)

    add('unet_sd15', UNet2DConditionEngine(SD15_CONFIG, f16, device='cpu'))
    add('unet_sdxl', UNet2DConditionEngine(SDXL_CONFIG, f16, device='cpu'))
    add('controlnet', ControlNetEngine(SD15_CONFIG, f16, device='cpu'))
    vae = AutoencoderKLEngine(None, f16, 'cpu')
    add('vae_decoder', vae.decoder)
    add('vae_encoder', vae.encoder)
    add('srvgg', SRVGGNetCompactEngine(dtype=f16, device='cpu'))
    add('lpips', LPIPSEngine(torch.bfloat16, device='cpu'))
    for k in ('A', 'B'):
        add('clip_text_' + k, CLIPTextEngine(SimpleNamespace(**GT.config_dict(k)), device='cpu', with_projection=GT.CASES[k]['with_projection']))
    for k in ('A', 'B', 'C'):
        add('clip_vision_' + k, CLIPVisionEngine(SimpleNamespace(**GV.config_dict(k)), device='cpu', with_projection=GV.CASES[k]['with_projection']))
    add('resampler', ResamplerEngine(device='cpu', **GV.RESAMPLER))
    for k in ('A', 'B'):
        add('dpt_' + k, DPTNormalEngine(dict(GD.engine_config(k)), device='cpu'))
    add('loftr', LoFTREngine(None, f16, device='cpu'))

    # an addition embedding declared on a handle whose configuration has none (mve_unet_set_addition_embed appends its slots)
    eng = UNet2DConditionEngine(SD15_CONFIG, f16, device='cpu')
    lib.call('mve_unet_set_addition_embed', eng._h, 1, 256, 2816)
    add('unet_sd15_addition_embed', eng)
    add('unet_tiny', UNet2DConditionEngine(U.TINY, f16, device='cpu'))
    # the unfused-shortcut layout (`.sc.w` slots): mve_unet_tune applies to handles created afterwards
    tune = lib.raw('mve_unet_tune')
    tune(0)
    try:
        add('unet_sd15_unfused_shortcut', UNet2DConditionEngine(SD15_CONFIG, f16, device='cpu'))
    finally:
        tune(1)
    return cases


if __name__ == '__main__':
    with open(OUT, 'w') as fh:
        json.dump(build_cases(), fh, indent=1)
        fh.write('\n')
    print(OUT, os.path.getsize(OUT), 'bytes')
