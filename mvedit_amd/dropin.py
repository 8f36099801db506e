"""Zero-edit drop-in under the reference (Lakonik/MVEdit): ONE import line ahead of the reference's own imports.

    import mvedit_amd.dropin; mvedit_amd.dropin.install()        # first line of app.py / of the serving entry point
    from lib.apis.adapter3d import Adapter3DRunner               # ... the reference, unchanged

What `install()` rebinds -- the operator seams of SURVEY.md section 8(b), nothing else of the reference:

  1. `lib.ops.raymarching` and `lib.ops.shencoder` (pybind11 / CUDA extensions, lib/ops/raymarching/src/bindings.cpp:5-19): the module names
     are pre-seeded in `sys.modules` with modules that export the reference's names (`__all__` of lib/ops/raymarching/__init__.py:1-8) bound to
     `mvedit_amd.raymarching` / `mvedit_amd.shencoder`, so `from .raymarching import *` in lib/ops/__init__.py:2 picks them up and the CUDA
     extension is never built or loaded.
  2. `lib.pipelines.adapter3d_mixin.Adapter3DMixin.get_noise_pred / get_noise_pred_p1 / get_noise_pred_p2` (adapter3d_mixin.py:68-317) and
     `lib.models.architecture.diffusers.unet_enc / unet_dec` (diffusers.py:57-164): rebound to this package's mirrors right after those
     modules are executed (a post-import hook on `sys.meta_path`; modules that are already imported are patched at once).
  3. The four classes `lib.pipelines` exports (lib/pipelines/__init__.py:1-7) get their `__init__` wrapped: after the reference's own
     constructor has registered the loaded torch modules (lib/apis/adapter3d.py:971-975), `pipe.unet`, `pipe.controlnet`, `pipe.vae`,
     `pipe.image_enhancer`, `pipe.segmentation` and `pipe.mesh_renderer` are replaced by engines built from those modules' own configs and
     state dicts, and `pipe.nerf.render` by the native renderer.  Engines are cached on the source module (`Adapter3DRunner` builds a pipeline
     object per request from the same loaded modules), and rebuilt when the module's parameters have been replaced or moved.  A UNet / ControlNet
     engine keeps its source module and treats that module's attention-processor table as the single source of truth: `attn_processors` /
     `set_attn_processor` delegate to the module and every forward translates the module's current table (mvedit_amd/attn_processors.py), so
     the runner's `unload_ip_adapter` (lib/apis/adapter3d.py:325-336), which talks to the modules and not to `pipe.unet`, reaches the engines.
     `Zero123PlusPipeline` is the exception: `from_pretrained` constructs it on the CPU and `prepare()` (zero123plus.py:316-319) wraps the UNet
     only while it still is a `UNet2DConditionModel`, so nothing is swapped at `__init__`; when `prepare()` returns with the parameters on an
     accelerator, the inner `.unet` of `RefOnlyNoisedUNet` (and the `.controlnet` of a `DepthControlUNet`) and `pipe.vae` are replaced, past
     `nn.Module.__setattr__` -- the wrappers keep their own `forward`, whose `mode` / `ref_dict` / `is_cfg_guidance` kwargs the engine
     understands, and the `ReferenceOnlyAttnProc` table `RefOnlyNoisedUNet.__init__` installed on the module is what the engine translates.
  4. `tinycudann` (CUDA-only, imported by lib/models/decoders/ingp_decoder.py:5-8 and triplane_ingp_decoder.py:5-8): seeded in `sys.modules`
     with `Encoding` bound to `mvedit_amd.tinycudann.Encoding`, so the reference's decoders construct and train unchanged.  Decoder
     modules imported before `install()` (their `tcnn` is None after the failed import) get `tcnn` rebound.
  5. `nvdiffrast` and `nvdiffrast.torch` (CUDA-only, imported at module level by lib/models/decoders/mesh_renderer/base_mesh_renderer.py:5, whose
     MeshRenderer the runner constructs and calls itself, lib/apis/adapter3d.py:88): seeded in `sys.modules` with `mvedit_amd.nvdiffrast` and
     `mvedit_amd.nvdiffrast.torch` (parent first), so `import nvdiffrast.torch as dr` resolves and `dr.*` computes on the native kernels.  A
     base_mesh_renderer imported before `install()` gets `dr` rebound.

Not part of `install()`: `swap_text_encoder(pipe)` puts native CLIP text towers (mvedit_amd/text_encoder.py) behind `pipe.text_encoder` /
`pipe.text_encoder_2` of ONE pipeline object, on request; `swap_image_encoder(obj)` puts the native CLIP vision tower
(mvedit_amd/vision_encoder.py) behind `image_encoder` / `vision_encoder` and the native image projection (mvedit_amd/ip_adapter.py) behind
`image_proj_model` of ONE object (an `IPAdapter`, a `Zero123PlusPipeline`, a `Zero123Pipeline`), on request; `swap_normal_model(pipe)` puts the
native DPT-hybrid normal predictor (mvedit_amd/normal_model.py) behind `pipe.normal_model`, on request; `swap_matcher(runner)` puts the native
LoFTR matcher (mvedit_amd/matcher.py) behind a loaded `runner.matcher`, on request; `swap_sam_image_encoder(runner)` puts the native SAM image
encoder (mvedit_amd/sam.py) behind `runner.predictor.model.image_encoder`, on request (prompt encoder and mask decoder stay torch);
`swap_sam_predictor(runner)` replaces the whole `runner.predictor` by the native `SamPredictorEngine`, on request.

Nothing here computes: every replacement is one of the engines / mirrors INTEGRATION.md documents seam by seam, and a conversion that fails
raises -- there is no fallback to the torch module.  `uninstall()` restores everything (tests).
"""
import importlib.abc
import importlib.util
import sys
import types

RAYMARCHING_NAMES = ('near_far_from_aabb', 'sph_from_ray', 'morton3D', 'morton3D_invert', 'packbits', 'march_rays_train',
                     'composite_rays_train', 'march_rays', 'composite_rays', 'batch_near_far_from_aabb', 'batch_composite_rays_train')
SHENCODER_NAMES = ('SHEncoder', 'sh_encode')
TCNN_NAMES = ('Encoding',)
TCNN_DECODERS = ('lib.models.decoders.ingp_decoder', 'lib.models.decoders.triplane_ingp_decoder')
NVDR_RENDERER = 'lib.models.decoders.mesh_renderer.base_mesh_renderer'
MIXIN_METHODS = ('get_noise_pred', 'get_noise_pred_p1', 'get_noise_pred_p2')
PIPELINE_CLASSES = {'lib.pipelines.mvedit_3d_pipeline': 'MVEdit3DPipeline',
                    'lib.pipelines.mvedit_texture_pipeline': 'MVEditTexturePipeline',
                    'lib.pipelines.mvedit_texture_superres_pipeline': 'MVEditTextureSuperResPipeline',
                    'lib.pipelines.zero123plus': 'Zero123PlusPipeline'}
SWAPPED_ATTRS = ('unet', 'controlnet', 'vae', 'image_enhancer', 'segmentation', 'mesh_renderer')

ZERO123_WRAPPERS = ('RefOnlyNoisedUNet', 'DepthControlUNet')          # lib/pipelines/zero123plus.py:80, :178 (recognised by class name)

_state = dict(installed=False, finder=None, undo=[], seeded=[], instances=[])


# ---------------------------------------------------------------------------------------------------------------------------------------
# engine construction from the reference's loaded torch modules
# ---------------------------------------------------------------------------------------------------------------------------------------
def _module_dtype_device(m):
    import torch
    p = next(iter(m.parameters()))
    if p.device.type == 'cpu':
        raise RuntimeError(f'{type(m).__name__}: its parameters are on the CPU -- an engine is built from weights that sit on the accelerator '
                           f'(move the module first; Zero123PlusPipeline is swapped at prepare() for this reason)')
    dtype = p.dtype if p.dtype in (torch.float16, torch.bfloat16) else torch.float16
    return dtype, p.device


def _fingerprint(m):
    """Identity of a module's parameter storage: a reloaded / re-typed / moved module gets a new engine."""
    return tuple((k, v.data_ptr(), v._version, str(v.device)) for k, v in list(m.state_dict().items())[:4])


def _on_accelerator(m):
    p = next(iter(m.parameters()), None)
    return p is not None and p.device.type != 'cpu'


def _follow_module_table(eng, module):
    """The module's attention-processor table becomes the engine's (AttnProcessorTable._attn_source); MultiControlNetModel: net by net."""
    nets = getattr(eng, 'nets', None)
    if nets is not None and hasattr(module, 'nets'):
        for e, n in zip(nets, module.nets):
            _follow_module_table(e, n)
    elif hasattr(eng, '_attn_resolve') and hasattr(module, 'attn_processors') and hasattr(module, 'set_attn_processor'):
        eng._attn_source = module


def make_unet(m):
    from .unet import UNet2DConditionEngine, config_from_diffusers
    dtype, device = _module_dtype_device(m)
    return UNet2DConditionEngine.from_state_dict(m.state_dict(), config_from_diffusers(m.config), dtype=dtype, device=device)


def make_controlnet(m):
    """`pipe.controlnet` is a diffusers MultiControlNetModel (`.nets`) or one ControlNetModel."""
    from .controlnet import ControlNetEngine, MultiControlNetEngine
    from .unet import config_from_diffusers
    nets = list(m.nets) if hasattr(m, 'nets') else [m]
    engines = []
    for n in nets:
        dtype, device = _module_dtype_device(n)
        engines.append(ControlNetEngine.from_state_dict(n.state_dict(), config_from_diffusers(n.config), dtype=dtype, device=device))
    return MultiControlNetEngine(engines) if hasattr(m, 'nets') else engines[0]


def make_vae(m):
    from .vae import AutoencoderKLEngine
    dtype, device = _module_dtype_device(m)
    return AutoencoderKLEngine.from_state_dict(m.state_dict(), dict(m.config), dtype=dtype, device=device)


def make_image_enhancer(m):
    """SRVGGNetCompact (lib/models/decoders/image_space_ss.py:8-70): body = conv, [act, conv] x num_conv, act?, conv -> pixel shuffle."""
    from .image_enhancer import SRVGGNetCompactEngine
    dtype, device = _module_dtype_device(m)
    eng = SRVGGNetCompactEngine(num_in_ch=m.num_in_ch, num_out_ch=m.num_out_ch, num_feat=m.num_feat, num_conv=m.num_conv, upscale=m.upscale,
                                act_type=getattr(m, 'act_type', 'prelu'), dtype=dtype, device=device)
    return eng.load_state_dict(m.state_dict())


def make_segmentation(m):
    """TracerUniversalB7 (lib/models/segmentors/tracer_b7.py:17-25)."""
    from .segmentor import TracerUniversalB7Engine
    dtype, device = _module_dtype_device(m)
    eng = TracerUniversalB7Engine(input_image_size=getattr(m, 'input_image_size', 640), batch_size=getattr(m, 'batch_size', 8),
                                  torch_dtype=dtype, erosion=getattr(m, 'erosion', 1), device=device)
    eng.load_state_dict(m.state_dict())
    return eng


def make_mesh_renderer(m):
    from .mesh_ops import MeshRenderer
    return MeshRenderer(near=m.near, far=m.far, ssaa=m.ssaa, texture_filter=getattr(m, 'texture_filter', 'linear-mipmap-linear'))


def decoder_params(decoder):
    """iNGPDecoder (lib/models/decoders/ingp_decoder.py:44-120) -> mvedit_amd.nerf.INGPDecoderParams: tcnn's flat hash table as [rows, 2], the two
    MLP layers."""
    from .nerf import INGPDecoderParams
    table = decoder.encoder.params.detach().float().reshape(-1, 2)
    l1, l2 = decoder.mlp.net[0], decoder.mlp.net[1]
    return INGPDecoderParams(table, l1.weight.detach(), l1.bias.detach(), l2.weight.detach(), l2.bias.detach(), n_levels=decoder.n_levels,
                             max_resolution=decoder.max_resolution, bound=getattr(decoder, 'bound', 1.0), blob_density=decoder.blob_density,
                             blob_radius=decoder.blob_radius, sigmoid_saturation=decoder.sigmoid_saturation, device=table.device)


def make_text_encoder(m):
    """transformers CLIPTextModel / CLIPTextModelWithProjection (`text_encoder`, `text_encoder_2`; lib/pipelines/utils.py:244-283)."""
    from .text_encoder import CLIPTextEngine
    dtype, device = _module_dtype_device(m)
    return CLIPTextEngine.from_module(m, dtype=dtype, device=device)


TEXT_ENCODER_ATTRS = ('text_encoder', 'text_encoder_2')


def swap_text_encoder(pipe):
    """Opt-in (install() / swap_engines leave the text towers alone): replaces `pipe.text_encoder` and, when present, `pipe.text_encoder_2` by
    native engines built from those modules.  Idempotent; the engine is cached on the source module like the other seams'."""
    for name in TEXT_ENCODER_ATTRS:
        m = getattr(pipe, name, None)
        if m is None or getattr(m, '_mve_is_engine', False) or not hasattr(m, 'state_dict'):
            continue
        fp = _fingerprint(m)
        cached = getattr(m, '_mve_engine', None)
        if cached is None or cached[0] != fp:
            eng = make_text_encoder(m)
            object.__setattr__(eng, '_mve_is_engine', True)
            cached = (fp, eng)
            object.__setattr__(m, '_mve_engine', cached)
        object.__setattr__(pipe, name, cached[1])
    return pipe


def make_image_encoder(m):
    """transformers CLIPVisionModelWithProjection / CLIPVisionModel (`IPAdapter.image_encoder`, lib/models/architecture/ip_adapter/ip_adapter.py:51-53;
    `Zero123PlusPipeline.vision_encoder`, lib/pipelines/zero123plus.py:372; `Zero123Pipeline.image_encoder`, lib/pipelines/zero123.py:260)."""
    from .vision_encoder import CLIPVisionEngine
    dtype, device = _module_dtype_device(m)
    return CLIPVisionEngine.from_module(m, dtype=dtype, device=device)


IMAGE_PROJ_CLASSES = ('Resampler', 'ImageProjModel')          # lib/models/architecture/ip_adapter/{resampler.py:77, ip_adapter.py:15} (recognised by class name)


def make_image_proj(m):
    """`IPAdapter.image_proj_model`: the reference's Resampler ("plus" checkpoints) or ImageProjModel (ip_adapter.py:58, :64-83)."""
    from .ip_adapter import ImageProjEngine, ResamplerEngine
    kind = type(m).__name__
    if kind not in IMAGE_PROJ_CLASSES:
        raise TypeError(f'{kind} is not an IP-Adapter image projection model ({" / ".join(IMAGE_PROJ_CLASSES)})')
    dtype, device = _module_dtype_device(m)
    return (ResamplerEngine if kind == 'Resampler' else ImageProjEngine).from_module(m, dtype=dtype, device=device)


IMAGE_ENCODER_ATTRS = ('image_encoder', 'vision_encoder')


def swap_image_encoder(obj):
    """Opt-in (install() / swap_engines leave the image towers alone): replaces `obj.image_encoder` / `obj.vision_encoder` and, when it is a
    Resampler or an ImageProjModel, `obj.image_proj_model` by native engines built from those modules -- an IPAdapter, a Zero123PlusPipeline or a
    Zero123Pipeline.  Idempotent; the engine is cached on the source module like the other seams'.  An `image_proj_model` of any other class is
    left alone."""
    for name in IMAGE_ENCODER_ATTRS + ('image_proj_model',):
        m = getattr(obj, name, None)
        if m is None or getattr(m, '_mve_is_engine', False) or not hasattr(m, 'state_dict'):
            continue
        if name == 'image_proj_model' and type(m).__name__ not in IMAGE_PROJ_CLASSES:
            continue
        fp = _fingerprint(m)
        cached = getattr(m, '_mve_engine', None)
        if cached is None or cached[0] != fp:
            eng = (make_image_proj if name == 'image_proj_model' else make_image_encoder)(m)
            object.__setattr__(eng, '_mve_is_engine', True)
            cached = (fp, eng)
            object.__setattr__(m, '_mve_engine', cached)
        object.__setattr__(obj, name, cached[1])
    return obj


def make_normal_model(m):
    """Omnidata's `DPTDepthModel(backbone='vitb_rn50_384', num_channels=3)` (`MVEdit3DPipeline.normal_model`, lib/apis/adapter3d.py:338-352;
    called by `enable_normals`, lib/pipelines/mvedit_3d_pipeline.py:262-273), or a transformers `DPTForDepthEstimation` of the same architecture."""
    from .normal_model import DPTNormalEngine
    dtype, device = _module_dtype_device(m)
    return DPTNormalEngine.from_module(m, dtype=dtype, device=device)


def swap_normal_model(pipe):
    """Opt-in (install() / swap_engines leave `normal_model` alone): replaces `pipe.normal_model` by a native engine built from that module.
    A pipeline without a normal predictor (`normal_model=None`) keeps `None`.  Idempotent; the engine is cached on the source module like the
    other seams'."""
    m = getattr(pipe, 'normal_model', None)
    if m is None or getattr(m, '_mve_is_engine', False) or not hasattr(m, 'state_dict'):
        return pipe
    fp = _fingerprint(m)
    cached = getattr(m, '_mve_engine', None)
    if cached is None or cached[0] != fp:
        eng = make_normal_model(m)
        object.__setattr__(eng, '_mve_is_engine', True)
        cached = (fp, eng)
        object.__setattr__(m, '_mve_engine', cached)
    object.__setattr__(pipe, 'normal_model', cached[1])
    return pipe


def make_matcher(m):
    """The reference's `LoFTR(config=default_cfg)` (`init_matcher`, lib/core/utils/pose_estimation.py; held as `runner.matcher`,
    lib/apis/adapter3d.py:411-415)."""
    from .matcher import LoFTREngine
    dtype, device = _module_dtype_device(m)
    return LoFTREngine.from_module(m, dtype=dtype, device=device)


def swap_matcher(obj):
    """Opt-in (install() / swap_engines leave `matcher` alone): replaces a loaded `obj.matcher` by a native engine built from that module.
    `matcher=None` (the runner before `load_matcher`, or after `unload_matcher`) stays `None`.  Idempotent; the engine is cached on the source
    module like the other seams'."""
    m = getattr(obj, 'matcher', None)
    if m is None or getattr(m, '_mve_is_engine', False) or not hasattr(m, 'state_dict'):
        return obj
    fp = _fingerprint(m)
    cached = getattr(m, '_mve_engine', None)
    if cached is None or cached[0] != fp:
        eng = make_matcher(m)
        object.__setattr__(eng, '_mve_is_engine', True)
        cached = (fp, eng)
        object.__setattr__(m, '_mve_engine', cached)
    object.__setattr__(obj, 'matcher', cached[1])
    return obj


def make_sam_image_encoder(m):
    """segment_anything's `ImageEncoderViT` (`predictor.model.image_encoder`, lib/apis/adapter3d.py:363-372) or transformers' `SamVisionEncoder` /
    `SamVisionModel`."""
    from .sam import SamImageEncoderEngine
    dtype, device = _module_dtype_device(m)
    return SamImageEncoderEngine.from_module(m, dtype=dtype, device=device)


def swap_sam_image_encoder(obj):
    """Opt-in (install() / swap_engines leave the SAM predictor alone): replaces the `image_encoder` of a `Sam`-like object by a native engine
    built from that module.  `obj` is the runner (through `.predictor`), a `SamPredictor` (through `.model`) or the `Sam` model itself; a
    `predictor` that is `None` (not loaded yet) stays `None`.  `Sam` is an `nn.Module`: the engine is set past `nn.Module.__setattr__`, so the
    torch encoder stays registered in `_modules` (and `uninstall()` puts it back in view).  The prompt encoder and the mask decoder are not
    touched.  Idempotent; the engine is cached on the source module like the other seams'."""
    sam = obj
    if hasattr(sam, 'predictor') and not hasattr(sam, 'image_encoder'):
        sam = sam.predictor
    if sam is not None and hasattr(sam, 'model') and not hasattr(sam, 'image_encoder'):
        sam = sam.model
    if sam is None:
        return obj
    m = getattr(sam, 'image_encoder', None)
    if m is None or getattr(m, '_mve_is_engine', False) or not hasattr(m, 'state_dict'):
        return obj
    fp = _fingerprint(m)
    cached = getattr(m, '_mve_engine', None)
    if cached is None or cached[0] != fp:
        eng = make_sam_image_encoder(m)
        object.__setattr__(eng, '_mve_is_engine', True)
        cached = (fp, eng)
        object.__setattr__(m, '_mve_engine', cached)
    _set_instance(sam, 'image_encoder', cached[1])
    return obj


def swap_sam_predictor(obj):
    """Opt-in (install() / swap_engines leave the SAM predictor alone): replaces `obj.predictor` -- the runner's `SamPredictor`
    (lib/apis/adapter3d.py:363-372) -- by a `mvedit_amd.sam.SamPredictorEngine` built from its model: image encoder, prompt encoder, mask decoder and
    the mask post-processing all run natively.  A `predictor` that is `None` (not loaded yet) stays `None`; `uninstall()` puts the original back.
    Idempotent; the engine is cached on the source predictor.  `swap_sam_image_encoder` is independent of it and keeps working."""
    from .sam import SamPredictorEngine
    p = getattr(obj, 'predictor', None)
    if p is None or isinstance(p, SamPredictorEngine):
        return obj
    cached = getattr(p, '_mve_predictor_engine', None)
    if cached is None:
        cached = SamPredictorEngine.from_predictor(p)
        object.__setattr__(p, '_mve_predictor_engine', cached)
    _set_instance(obj, 'predictor', cached)
    return obj


MAKERS = dict(unet=make_unet, controlnet=make_controlnet, vae=make_vae, image_enhancer=make_image_enhancer, segmentation=make_segmentation,
              mesh_renderer=make_mesh_renderer)


def engine_for(kind, module):
    """The engine standing in for `module` (cached on it)."""
    if module is None or getattr(module, '_mve_is_engine', False) or not hasattr(module, 'state_dict') and kind != 'mesh_renderer':
        return module
    fp = _fingerprint(module) if hasattr(module, 'state_dict') else None
    cached = getattr(module, '_mve_engine', None)
    if cached is not None and cached[0] == fp:
        return cached[1]
    eng = MAKERS[kind](module)
    if kind in ('unet', 'controlnet'):
        _follow_module_table(eng, module)
    try:
        object.__setattr__(eng, '_mve_is_engine', True)
    except (AttributeError, TypeError):
        pass
    object.__setattr__(module, '_mve_engine', (fp, eng))
    return eng


def _native_nerf_render(nerf):
    """Bound replacement for `BaseNeRF.render` (lib/models/autoencoders/base_nerf.py:489-560) on ONE nerf object."""
    from .nerf import NeRFRenderer

    def render(decoder, code, density_bitfield, h, w, intrinsics, poses, cfg=dict(), bg_color=None, perturb=False, normal_bg=(0.5, 0.5, 1.0)):
        cached = getattr(decoder, '_mve_engine', None)
        fp = _fingerprint(decoder)
        if cached is None or cached[0] != fp:
            cached = (fp, decoder_params(decoder))
            object.__setattr__(decoder, '_mve_engine', cached)
        r = NeRFRenderer(grid_size=getattr(nerf, 'grid_size', 128), bg_color=nerf.bg_color)
        return r.render(cached[1], code, density_bitfield, h, w, intrinsics, poses, cfg=cfg, bg_color=bg_color, perturb=perturb, normal_bg=normal_bg)
    return render


def swap_engines(pipe):
    """After the reference constructor: the seams of one pipeline object."""
    for name in SWAPPED_ATTRS:
        m = getattr(pipe, name, None)
        if m is not None:
            object.__setattr__(pipe, name, engine_for(name, m))       # (object.__setattr__: past DiffusionPipeline's config bookkeeping)
    nerf = getattr(pipe, 'nerf', None)
    if nerf is not None and not getattr(nerf, '_mve_render_bound', False):
        object.__setattr__(nerf, 'render', _native_nerf_render(nerf))
        object.__setattr__(nerf, '_mve_render_bound', True)
    return pipe


def _set_instance(obj, name, value):
    """Instance attribute past nn.Module.__setattr__ (the torch module stays registered in `_modules`, so `.to()` / `state_dict()` of a wrapper
    still see it); remembered for uninstall()."""
    if obj.__dict__.get(name) is value:
        return
    _state['instances'].append((obj, name, name in obj.__dict__, obj.__dict__.get(name)))
    object.__setattr__(obj, name, value)


def swap_zero123(pipe):
    """After `Zero123PlusPipeline.prepare()`: idempotent; members whose parameters are still on the CPU are left for the next call."""
    vae = getattr(pipe, 'vae', None)
    if vae is not None and not getattr(vae, '_mve_is_engine', False) and _on_accelerator(vae):
        _set_instance(pipe, 'vae', engine_for('vae', vae))
    w = getattr(pipe, 'unet', None)
    while type(w).__name__ in ZERO123_WRAPPERS:
        for name, kind in (('controlnet', 'controlnet'), ('unet', 'unet')):
            inner = w.__dict__.get(name) or w.__dict__.get('_modules', {}).get(name)
            if inner is None or getattr(inner, '_mve_is_engine', False) or type(inner).__name__ in ZERO123_WRAPPERS:
                continue
            if _on_accelerator(inner):
                _set_instance(w, name, engine_for(kind, inner))
        w = w.__dict__.get('_modules', {}).get('unet') if type(w).__name__ == 'DepthControlUNet' else None
    return pipe


# ---------------------------------------------------------------------------------------------------------------------------------------
# patches
# ---------------------------------------------------------------------------------------------------------------------------------------
def _set(obj, name, value):
    had = name in vars(obj) if isinstance(obj, type) else hasattr(obj, name)
    old = vars(obj).get(name) if isinstance(obj, type) else getattr(obj, name, None)
    setattr(obj, name, value)
    _state['undo'].append((obj, name, had, old))


def _patch_mixin(mod):
    from .pipelines import Adapter3DMixin as Ours
    cls = getattr(mod, 'Adapter3DMixin')
    for n in MIXIN_METHODS:
        _set(cls, n, vars(Ours)[n])
    # helpers the mirrors call on `self` / class attributes they read
    for n, v in vars(Ours).items():
        if n.startswith('_') and not n.startswith('__') and n not in vars(cls):
            _set(cls, n, v)
    for n in ('fuse_chunks', 'detect_repeated_cond'):
        if hasattr(Ours, n) and n not in vars(cls):
            _set(cls, n, getattr(Ours, n))


def _patch_arch_diffusers(mod):
    from . import unet as U
    _set(mod, 'unet_enc', U.unet_enc)
    _set(mod, 'unet_dec', U.unet_dec)


def _patch_pipeline(mod):
    cls = getattr(mod, PIPELINE_CLASSES[mod.__name__])
    orig = cls.__init__
    if getattr(orig, '_mve_wrapped', False):
        return

    zero123 = cls.__name__ == 'Zero123PlusPipeline'

    def __init__(self, *args, **kwargs):
        orig(self, *args, **kwargs)
        if not zero123:              # from_pretrained builds Zero123++ on the CPU and prepare() must still find a UNet2DConditionModel
            swap_engines(self)
    __init__._mve_wrapped = True
    __init__.__wrapped__ = orig
    _set(cls, '__init__', __init__)
    prepare = vars(cls).get('prepare')
    if zero123 and prepare is not None:
        def prepare_and_swap(self, *args, **kwargs):
            out = prepare(self, *args, **kwargs)
            swap_zero123(self)
            return out
        prepare_and_swap.__wrapped__ = prepare
        _set(cls, 'prepare', prepare_and_swap)


def _patch_tcnn_decoder(mod):
    _set(mod, 'tcnn', sys.modules['tinycudann'])


def _patch_nvdr_renderer(mod):
    _set(mod, 'dr', sys.modules['nvdiffrast.torch'])


PATCHERS = {'lib.pipelines.adapter3d_mixin': _patch_mixin, 'lib.models.architecture.diffusers': _patch_arch_diffusers}
PATCHERS.update({k: _patch_pipeline for k in PIPELINE_CLASSES})
PATCHERS.update({k: _patch_tcnn_decoder for k in TCNN_DECODERS})
PATCHERS[NVDR_RENDERER] = _patch_nvdr_renderer


class _PostImport(importlib.abc.MetaPathFinder):
    """Runs the patcher of a target module right after the module has been executed."""

    def find_spec(self, name, path=None, target=None):
        if name not in PATCHERS:
            return None
        for f in sys.meta_path:
            if f is self or not hasattr(f, 'find_spec'):
                continue
            spec = f.find_spec(name, path, target)
            if spec is not None and spec.loader is not None and hasattr(spec.loader, 'exec_module'):
                spec.loader = _Loader(spec.loader, PATCHERS[name])
                return spec
        return None


class _Loader(importlib.abc.Loader):
    def __init__(self, inner, patch):
        self.inner, self.patch = inner, patch

    def create_module(self, spec):
        return self.inner.create_module(spec)

    def exec_module(self, module):
        self.inner.exec_module(module)
        self.patch(module)

    def __getattr__(self, n):
        return getattr(self.inner, n)


def _seed_module(name, names, source):
    m = types.ModuleType(name)
    m.__doc__ = f'mvedit_amd.dropin: {source.__name__} under the reference name {name}'
    for n in names:
        setattr(m, n, getattr(source, n))
    m.__all__ = list(names)
    m.__path__ = []           # a package in the reference (lib/ops/raymarching/): submodule imports resolve to nothing rather than to the CUDA build
    m._mve_seeded = True
    _state['seeded'].append((name, sys.modules.get(name)))
    sys.modules[name] = m
    parent = sys.modules.get(name.rpartition('.')[0])
    if parent is not None:
        setattr(parent, name.rpartition('.')[2], m)
        for n in names:       # `from .raymarching import *` already ran in lib/ops/__init__.py: rebind the star-imported names too
            if hasattr(parent, n):
                _set(parent, n, getattr(source, n))


def _seed_as(name, module):
    """`module` itself under the reference's name (a package with a submodule: the objects are shared, not copied)."""
    _state['seeded'].append((name, sys.modules.get(name)))
    sys.modules[name] = module


def install():
    """Idempotent.  Call before the reference's modules are imported (already-imported ones are patched in place)."""
    if _state['installed']:
        return
    from . import nvdiffrast, raymarching, shencoder, tinycudann
    _seed_module('lib.ops.raymarching', RAYMARCHING_NAMES, raymarching)
    _seed_module('lib.ops.shencoder', SHENCODER_NAMES, shencoder)
    _seed_module('tinycudann', TCNN_NAMES, tinycudann)
    _seed_as('nvdiffrast', nvdiffrast)                  # parent first: `import nvdiffrast.torch as dr` looks both up
    _seed_as('nvdiffrast.torch', nvdiffrast.torch)
    for name, patch in PATCHERS.items():
        if name in sys.modules:
            patch(sys.modules[name])
    _state['finder'] = _PostImport()
    sys.meta_path.insert(0, _state['finder'])
    _state['installed'] = True


def uninstall():
    # instance swaps first: the opt-in swap_sam_image_encoder records one whether or not install() ran
    for obj, name, had, old in reversed(_state['instances']):
        if had:
            object.__setattr__(obj, name, old)
        else:
            obj.__dict__.pop(name, None)
    _state['instances'] = []
    if not _state['installed']:
        return
    if _state['finder'] in sys.meta_path:
        sys.meta_path.remove(_state['finder'])
    for obj, name, had, old in reversed(_state['undo']):
        if had:
            setattr(obj, name, old)
        else:
            try:
                delattr(obj, name)
            except AttributeError:
                pass
    for name, old in reversed(_state['seeded']):
        if old is None:
            sys.modules.pop(name, None)
        else:
            sys.modules[name] = old
    _state.update(installed=False, finder=None, undo=[], seeded=[], instances=[])
