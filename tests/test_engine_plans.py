"""Plans of the nine executor engines against tests/golden/engine_plans.json (host only, no GPU): workspace size, op count, the five flop sums and
the whole op list -- phase, class, flops, label of every op -- are EXACTLY what was recorded.  Integers compare as integers and doubles survive
JSON's repr round trip, so there is no tolerance: a change to the executor's entry points, configuration or Python handles that moves one byte of
workspace or one op shows here before any GPU is involved.  tests/golden/make_engine_plans_golden.py names the cases and rewrites the file when a
plan is meant to change."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ('unet_sd15', 'unet_sd15_residuals', 'unet_sd15_cross_imgs2', 'unet_sdxl', 'controlnet', 'controlnet_ctx93_tail4', 'vae_decoder', 'vae_encoder',
         'srvgg', 'lpips', 'clip_text', 'clip_vision', 'resampler', 'dpt', 'loftr_coarse', 'loftr_fine',
         'clip_text_B', 'clip_vision_B', 'clip_vision_C', 'resampler_b2', 'dpt_B', 'vae_decoder_b2', 'unet_sd15_residuals_nhwc', 'loftr_coarse_n2',
         'loftr_fine_n2')


@pytest.fixture(scope='module')
def plans(lib):
    spec = importlib.util.spec_from_file_location('make_engine_plans_golden', os.path.join(HERE, 'golden', 'make_engine_plans_golden.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.OUT) as fh:
        golden = json.load(fh)
    return json.loads(json.dumps(gen.build_cases())), golden          # the same round trip on both sides


def test_the_golden_covers_the_cases(plans):
    now, golden = plans
    assert tuple(golden) == CASES and tuple(now) == CASES


@pytest.mark.parametrize('case', CASES)
def test_plan_is_exactly_the_recorded_one(plans, case):
    now, golden = plans
    got, want = now[case], golden[case]
    assert got['workspace_bytes'] == want['workspace_bytes'] and got['n_ops'] == want['n_ops'] == len(want['ops'])
    assert got['flops'] == want['flops'] and got.get('n_forward_ops') == want.get('n_forward_ops')
    for i, (a, b) in enumerate(zip(got['ops'], want['ops'])):
        assert a == b, f'{case}: op {i} is {a}, recorded {b}'
    assert got == want
