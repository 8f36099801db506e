"""Golden for the plans of the nine executor engines: what `plan()` answers and the whole op list, recorded from the library itself.

    python tests/golden/make_engine_plans_golden.py          (host only: plans are built without a GPU; writes tests/golden/engine_plans.json)

Plans are pure host work, so a change that is meant to leave every engine's op list alone (a refactor of the executor's entry points, of its
configuration or of the Python handles) regenerates nothing: tests/test_engine_plans.py calls `build_cases()` below on the current tree and asks
for exact equality with the file recorded BEFORE the change -- integers as they are, doubles through JSON's repr round trip, no tolerance.  Run
this script only on a commit whose plans are the intended ones (a new op, a new engine, a changed flop count).

One entry per case: `workspace_bytes`, `n_ops`, `flops` (the five class sums in the order conv3x3 / linear / attention / norm / other) and `ops`,
one `[phase, class, flops, label]` per op as mve_unet_op_info describes it (read through the C call, so the entry does not depend on the tuple shape
of any engine's own op_table()); LPIPS entries also carry `n_forward_ops`.
"""
import ctypes
import json
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'engine_plans.json')


def _ops(lib, handle):
    out, i = [], 0
    cls, fl, lab = ctypes.c_int(), ctypes.c_double(), ctypes.create_string_buffer(96)
    info = lib.raw('mve_unet_op_info')
    while True:
        ph = info(handle, i, ctypes.byref(cls), ctypes.byref(fl), lab, 96)
        if ph < 0:
            return out
        out.append([ph, cls.value, fl.value, lab.value.decode()])
        i += 1


def _entry(lib, eng, info):
    e = dict(workspace_bytes=info['workspace_bytes'], n_ops=info['n_ops'])
    if 'flops' in info:
        e['flops'] = list(info['flops'].values())
    else:                                                     # LPIPSEngine.plan reports the conv sum alone
        e['flops'] = [info['conv_flops']]
        e['n_forward_ops'] = info['n_forward_ops']
    e['ops'] = _ops(lib, eng._h)
    assert len(e['ops']) == e['n_ops']
    return e


def build_cases():
    """{case name: entry} from the library of the tree this file lies in."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    sys.path.insert(0, HERE)
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
    import make_clip_text_golden as GT
    import make_clip_vision_golden as GV
    import make_dpt_normal_golden as GD
    f16 = torch.float16
    cases = {}

    unet = UNet2DConditionEngine(SD15_CONFIG, f16, device='cpu')
    cases['unet_sd15'] = _entry(lib, unet, unet.plan(2, 16, 16, 77))
    cases['unet_sd15_residuals'] = _entry(lib, unet, unet.plan(2, 16, 16, 77, has_residuals=True))
    cases['unet_sd15_cross_imgs2'] = _entry(lib, unet, unet.plan(2, 16, 16, 77, num_cross_attn_imgs=2))
    xl = UNet2DConditionEngine(SDXL_CONFIG, f16, device='cpu')
    cases['unet_sdxl'] = _entry(lib, xl, xl.plan(2, 16, 16, 77))

    cn = ControlNetEngine(SD15_CONFIG, f16, device='cpu')
    cases['controlnet'] = _entry(lib, cn, cn.plan(2, 16, 16, 77))
    tail = lib.raw('mve_unet_set_context_tail')
    assert tail(cn._h, 4) == 0
    cases['controlnet_ctx93_tail4'] = _entry(lib, cn, cn.plan(2, 16, 16, 93))
    assert tail(cn._h, 0) == 4

    vae = AutoencoderKLEngine(None, f16, 'cpu')
    cases['vae_decoder'] = _entry(lib, vae.decoder, vae.decoder.plan(1, 8, 8, f16))
    cases['vae_encoder'] = _entry(lib, vae.encoder, vae.encoder.plan(1, 64, 64, f16))
    sr = SRVGGNetCompactEngine(dtype=f16, device='cpu')
    cases['srvgg'] = _entry(lib, sr, sr.plan(1, 8, 8))
    lp = LPIPSEngine(torch.bfloat16, device='cpu')
    cases['lpips'] = _entry(lib, lp, lp.plan(1, 32, 32))

    text = CLIPTextEngine(SimpleNamespace(**GT.config_dict('A')), device='cpu', with_projection=GT.CASES['A']['with_projection'])
    cases['clip_text'] = _entry(lib, text, text.plan(1, 77))
    vision = CLIPVisionEngine(SimpleNamespace(**GV.config_dict('A')), device='cpu', with_projection=GV.CASES['A']['with_projection'])
    cases['clip_vision'] = _entry(lib, vision, vision.plan(1))
    rs = ResamplerEngine(device='cpu', **GV.RESAMPLER)
    rs_tokens = vision.num_tokens
    cases['resampler'] = _entry(lib, rs, rs.plan(1, rs_tokens))
    dpt = DPTNormalEngine(dict(GD.engine_config('A')), device='cpu')
    cases['dpt'] = _entry(lib, dpt, dpt.plan(1))
    loftr = LoFTREngine(None, f16, device='cpu')
    cases['loftr_coarse'] = _entry(lib, loftr, loftr.plan(1, 64, 64, 1))
    cases['loftr_fine'] = _entry(lib, loftr, loftr.plan(1, 64, 64, 2))

    # branches of the plan builders that the cases above do not take (appended, so the entries above keep their place in the file)
    text = CLIPTextEngine(SimpleNamespace(**GT.config_dict('B')), device='cpu', with_projection=GT.CASES['B']['with_projection'])
    cases['clip_text_B'] = _entry(lib, text, text.plan(1, 77))
    for k in ('B', 'C'):
        vision = CLIPVisionEngine(SimpleNamespace(**GV.config_dict(k)), device='cpu', with_projection=GV.CASES[k]['with_projection'])
        cases['clip_vision_' + k] = _entry(lib, vision, vision.plan(1))
    cases['resampler_b2'] = _entry(lib, rs, rs.plan(2, rs_tokens))
    dpt = DPTNormalEngine(dict(GD.engine_config('B')), device='cpu')
    cases['dpt_B'] = _entry(lib, dpt, dpt.plan(2))
    cases['vae_decoder_b2'] = _entry(lib, vae.decoder, vae.decoder.plan(2, 8, 8, f16))
    cases['unet_sd15_residuals_nhwc'] = _entry(lib, unet, unet.plan(2, 16, 16, 77, has_residuals=True, residuals_nhwc=True))
    cases['loftr_coarse_n2'] = _entry(lib, loftr, loftr.plan(2, 64, 64, 1))
    cases['loftr_fine_n2'] = _entry(lib, loftr, loftr.plan(2, 64, 64, 2))
    return cases


if __name__ == '__main__':
    with open(OUT, 'w') as fh:
        json.dump(build_cases(), fh, separators=(',', ':'))
        fh.write('\n')
    print(OUT, os.path.getsize(OUT), 'bytes')
