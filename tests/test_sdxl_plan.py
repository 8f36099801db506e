"""SDXL topology and its 'text_time' added-condition embedding at plan time (device='cpu': no device memory is touched).

The forward itself runs in tests/test_unet_sdxl.py on the GPU.  PARITY UNPINNED: diffusers is not importable here and the reference has no SDXL
pipeline; the published configuration is written out below."""
import math

import pytest
import torch

# unet/config.json of stabilityai/stable-diffusion-xl-base-1.0 as published (the keys the engine reads, and the ones it must refuse when set)
SDXL_PUBLISHED = dict(
    act_fn='silu', addition_embed_type='text_time', addition_embed_type_num_heads=64, addition_time_embed_dim=256,
    attention_head_dim=[5, 10, 20], block_out_channels=[320, 640, 1280], center_input_sample=False, class_embed_type=None,
    class_embeddings_concat=False, conv_in_kernel=3, conv_out_kernel=3, cross_attention_dim=2048, cross_attention_norm=None,
    down_block_types=['DownBlock2D', 'CrossAttnDownBlock2D', 'CrossAttnDownBlock2D'], downsample_padding=1, dual_cross_attention=False,
    encoder_hid_dim=None, encoder_hid_dim_type=None, flip_sin_to_cos=True, freq_shift=0, in_channels=4, layers_per_block=2,
    mid_block_only_cross_attention=None, mid_block_scale_factor=1, mid_block_type='UNetMidBlock2DCrossAttn', norm_eps=1e-05,
    norm_num_groups=32, num_attention_heads=None, num_class_embeds=None, only_cross_attention=False, out_channels=4,
    projection_class_embeddings_input_dim=2816, resnet_out_scale_factor=1.0, resnet_skip_time_act=False, resnet_time_scale_shift='default',
    sample_size=128, time_cond_proj_dim=None, time_embedding_act_fn=None, time_embedding_dim=None, time_embedding_type='positional',
    timestep_post_act=None, transformer_layers_per_block=[1, 2, 10], up_block_types=['CrossAttnUpBlock2D', 'CrossAttnUpBlock2D', 'UpBlock2D'],
    upcast_attention=None, use_linear_projection=True)


def _tflop(info):
    return sum(info['flops'][k] for k in ('conv3x3', 'linear', 'attention')) / 1e12


def test_sdxl_plan_flops_attention_ops_and_add_embedding(lib):
    from mvedit_amd.unet import SDXL_CONFIG, UNet2DConditionEngine
    eng = UNet2DConditionEngine(SDXL_CONFIG, torch.float16, device='cpu')
    assert eng.config.addition_embed_type == 'text_time'
    B = 1
    info = eng.plan(B, 96, 96, 77)
    assert abs(_tflop(info) - 3.64) <= 2e-3, _tflop(info)                                # 3.64 TFLOP per 768 x 768 forward
    table = eng.op_table()
    assert sum(c == 'attention' for _, c, _, _ in table) == 140
    labels = [lab for _, _, _, lab in table]
    assert labels.count('add_embedding.linear_1') == 1 and labels.count('add_embedding.linear_2') == 1
    assert labels.count('add_embedding.text_time') == 1
    # prologue order: time_embedding.linear_2 -> the operand row -> linear_1 -> SiLU -> linear_2 (+ emb) -> SiLU -> the merged time_emb_proj GEMM
    i = labels.index('time_embedding.linear_2')
    assert labels[i + 1:i + 7] == ['add_embedding.text_time', 'add_embedding.linear_1', 'silu', 'add_embedding.linear_2', 'silu',
                                   'time_emb_proj (all resnets, one GEMM)']
    assert all(c == 'linear' for _, c, _, lab in table if lab.startswith('add_embedding.linear'))
    plain = UNet2DConditionEngine({k: v for k, v in SDXL_CONFIG.items() if not k.startswith(('addition_', 'projection_'))}, torch.float16, device='cpu')
    assert plain.config.addition_embed_type is None
    base = plain.plan(B, 96, 96, 77)
    assert info['flops']['linear'] - base['flops']['linear'] == 2 * B * (2816 * 1280 + 1280 ** 2)
    assert info['n_ops'] == base['n_ops'] + 4 and info['flops']['conv3x3'] == base['flops']['conv3x3']
    assert info['flops']['attention'] == base['flops']['attention']
    assert not any('add_embedding' in lab for _, _, _, lab in plain.op_table())
    B = 2
    assert eng.plan(B, 96, 96, 77)['flops']['linear'] - plain.plan(B, 96, 96, 77)['flops']['linear'] == 2 * B * (2816 * 1280 + 1280 ** 2)


def test_sdxl_parameter_inventory():
    from mvedit_amd import synthetic
    from mvedit_amd.unet import SDXL_CONFIG
    shapes = synthetic.param_shapes(SDXL_CONFIG)
    assert sum(math.prod(s) for s in shapes.values()) == 2_567_463_684                      # the SDXL base UNet's published size
    assert shapes['add_embedding.linear_1.weight'] == (1280, 2816) and shapes['add_embedding.linear_2.weight'] == (1280, 1280)
    cn = synthetic.controlnet_param_shapes(SDXL_CONFIG)
    assert cn['add_embedding.linear_1.weight'] == (1280, 2816) and 'add_embedding.linear_2.bias' in cn
    from mvedit_amd.unet import SD15_CONFIG
    assert not any(k.startswith('add_embedding') for k in synthetic.param_shapes(SD15_CONFIG))
    assert not any(k.startswith('add_embedding') for k in synthetic.controlnet_param_shapes(SD15_CONFIG))


def test_config_from_diffusers_translates_sdxl_and_refuses_what_it_cannot_run():
    from mvedit_amd.unet import SDXL_CONFIG, config_from_diffusers
    assert config_from_diffusers(SDXL_PUBLISHED) == SDXL_CONFIG
    assert SDXL_CONFIG['transformer_layers'] == (0, 2, 10)                                # 0 where the level has no attention
    with pytest.raises(NotImplementedError, match='addition_embed_type'):
        config_from_diffusers(dict(SDXL_PUBLISHED, addition_embed_type='text'))
    with pytest.raises(NotImplementedError, match='class_embed_type'):
        config_from_diffusers(dict(SDXL_PUBLISHED, class_embed_type='timestep'))
    with pytest.raises(NotImplementedError, match='encoder_hid_dim_type'):
        config_from_diffusers(dict(SDXL_PUBLISHED, encoder_hid_dim_type='text_proj'))
    with pytest.raises(NotImplementedError, match='up_block_types'):
        config_from_diffusers(dict(SDXL_PUBLISHED, up_block_types=['UpBlock2D', 'CrossAttnUpBlock2D', 'CrossAttnUpBlock2D']))
    # an SD-1.5 style config (no addition keys at all) translates as before: no addition keys appear, the mid block's depth survives
    sd15 = dict(in_channels=4, out_channels=4, block_out_channels=[320, 640, 1280, 1280], layers_per_block=2, attention_head_dim=8,
                down_block_types=['CrossAttnDownBlock2D'] * 3 + ['DownBlock2D'], up_block_types=['UpBlock2D'] + ['CrossAttnUpBlock2D'] * 3,
                cross_attention_dim=768, norm_num_groups=32, norm_eps=1e-5)
    from mvedit_amd.unet import SD15_CONFIG
    assert config_from_diffusers(sd15) == SD15_CONFIG


def test_controlnet_plan_carries_the_same_prologue(lib):
    from mvedit_amd.controlnet import ControlNetEngine
    from mvedit_amd.unet import SDXL_CONFIG
    cn = ControlNetEngine(SDXL_CONFIG, torch.float16, device='cpu')
    cn.plan(1, 32, 32, 77)
    labels = [lab for _, _, _, lab in cn.op_table()]
    assert labels.count('add_embedding.linear_1') == 1 and labels.count('add_embedding.linear_2') == 1


def test_addition_embed_is_declared_once_and_is_part_of_the_plan_key(lib):
    from mvedit_amd.unet import SD15_CONFIG, UNet2DConditionEngine
    eng = UNet2DConditionEngine(dict(SD15_CONFIG, block_out_channels=(320, 640), layers_per_block=1, down_attn=(True, False), num_heads=(8, 8),
                                     transformer_layers=(1, 1)), torch.float16, device='cpu')
    a = eng.plan(1, 16, 16, 77)
    lib.call('mve_unet_set_addition_embed', eng._h, 1, 256, 2816)                          # a plan exists already: the declared type re-plans
    b = eng.plan(1, 16, 16, 77)
    assert b['n_ops'] == a['n_ops'] + 4 and any('add_embedding' in lab for _, _, _, lab in eng.op_table())
    with pytest.raises(lib.MveError, match='already'):
        lib.call('mve_unet_set_addition_embed', eng._h, 1, 256, 2816)
    with pytest.raises(lib.MveError, match='text width'):
        lib.call('mve_unet_bind_added_cond', eng._h, 16, 1, 1281, 16, 6, 1)                # 1281 + 6 * 256 != 2816 (the pointers are never read)
    for bad in ((2, 256, 2816), (1, 255, 2816), (1, 256, 2812)):
        fresh = UNet2DConditionEngine(SD15_CONFIG, torch.float16, device='cpu')
        with pytest.raises(lib.MveError):
            lib.call('mve_unet_set_addition_embed', fresh._h, *bad)


def test_sd15_plan_is_unchanged(lib):
    """Engines without addition_embed_type plan exactly as before this feature: op count and workspace of SD-1.5 as recorded on the parent commit."""
    from mvedit_amd.unet import SD15_CONFIG, UNet2DConditionEngine
    eng = UNet2DConditionEngine(SD15_CONFIG, torch.float16, device='cpu')
    info = eng.plan(2, 64, 64, 77)
    assert not any('add_embedding' in lab for _, _, _, lab in eng.op_table())
    assert (info['n_ops'], info['workspace_bytes']) == PARENT_SD15_B2_64, (info['n_ops'], info['workspace_bytes'])
    eng.set_residual_pair(False)
    info = eng.plan(2, 64, 64, 77)
    assert (info['n_ops'], info['workspace_bytes']) == PARENT_SD15_B2_64_PLAIN, (info['n_ops'], info['workspace_bytes'])


# (n_ops, workspace_bytes) of SD15_CONFIG.plan(2, 64, 64, 77) on the parent commit: default (residual pair) mode, and the 16-bit stream
PARENT_SD15_B2_64 = (282, 106295808)
PARENT_SD15_B2_64_PLAIN = (282, 84668928)
