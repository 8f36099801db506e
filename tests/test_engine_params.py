"""Parameter layout of the nine executor engines against tests/golden/engine_params.json (host only, no GPU): the slab size, the number of required
state-dict names and the first of them are EXACTLY what was recorded before the layout became the loader's table.  A slot that changes its size,
its place in the order or its padding moves the slab size; a required name that is dropped, added or reordered moves the count or the first
missing name.  tests/golden/make_engine_params_golden.py names the cases and rewrites the file when a layout is meant to change."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ('unet_sd15', 'unet_sdxl', 'controlnet', 'vae_decoder', 'vae_encoder', 'srvgg', 'lpips', 'clip_text_A', 'clip_text_B', 'clip_vision_A',
         'clip_vision_B', 'clip_vision_C', 'resampler', 'dpt_A', 'dpt_B', 'loftr', 'unet_sd15_addition_embed', 'unet_tiny', 'unet_sd15_unfused_shortcut')


@pytest.fixture(scope='module')
def layouts(lib):
    spec = importlib.util.spec_from_file_location('make_engine_params_golden', os.path.join(HERE, 'golden', 'make_engine_params_golden.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.OUT) as fh:
        golden = json.load(fh)
    return gen.build_cases(), golden


def test_the_golden_covers_the_cases(layouts):
    now, golden = layouts
    assert tuple(golden) == CASES and tuple(now) == CASES


@pytest.mark.parametrize('case', CASES)
def test_layout_is_exactly_the_recorded_one(layouts, case):
    now, golden = layouts
    assert now[case] == golden[case]
    assert now[case]['weight_bytes'] > 0 and now[case]['missing'] > 0 and now[case]['first_missing']


def test_the_shortcut_switch_is_left_on(lib, layouts):
    assert lib.raw('mve_unet_tune')(-1) == 1
