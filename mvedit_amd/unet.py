"""Host-side mirror of the reference's UNet seam on top of the native executor (csrc/unet.hip).

`UNet2DConditionEngine` is called exactly like the diffusers `UNet2DConditionModel` the reference
pipelines hold as `self.unet` (lib/pipelines/adapter3d_mixin.py:117-125):

    unet(sample, t, encoder_hidden_states=..., cross_attention_kwargs=dict(num_cross_attn_imgs=2),
         down_block_additional_residuals=[...12...], mid_block_additional_residual=..., return_dict=False)[0]

and `unet_enc(unet, ...)` / `unet_dec(unet, ...)` below mirror lib/models/architecture/diffusers.py:57-164.
PyTorch tensors are storage only: one C-ABI call runs the whole forward on the current HIP stream.
There is no torch fallback -- construction fails if libmvedit_amd.so is missing.
"""
import ctypes
import os
from types import SimpleNamespace

import torch

from . import _lib
from .attn_processors import AttnProcessorTable, attn_processor_names
from .module_surface import EngineHandle
from .ops import dt as _dt

SD15_CONFIG = dict(
    in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
    down_attn=(True, True, True, False), num_heads=(8, 8, 8, 8), cross_attention_dim=768, norm_num_groups=32,
    norm_eps=1e-5, transformer_layers=(1, 1, 1, 1), use_linear_projection=False)

# Stable Diffusion 2.1 topology (the Zero123++ base model, lib/pipelines/zero123plus.py): head_dim 64, linear projections, ctx 1024
SD21_CONFIG = dict(
    in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
    down_attn=(True, True, True, False), num_heads=(5, 10, 20, 20), cross_attention_dim=1024, norm_num_groups=32,
    norm_eps=1e-5, transformer_layers=(1, 1, 1, 1), use_linear_projection=True)

# Stable Diffusion XL base 1.0 topology, restated from the published unet/config.json of stabilityai/stable-diffusion-xl-base-1.0 (three levels, no
# attention at level 0, transformer depth 2 / 10, head_dim 64, ctx 2048, linear projections, 'text_time' added-condition embedding of
# 6 time ids x 256 + 1280 pooled text = 2816 -> 1280).  PARITY UNPINNED: diffusers is not importable here and the reference ships no SDXL pipeline
# (SURVEY.md F9), so this topology is checked against the repository's own oracle only.  transformer_layers is 0 where down_attn is false.
SDXL_CONFIG = dict(
    in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280), layers_per_block=2,
    down_attn=(False, True, True), num_heads=(5, 10, 20), cross_attention_dim=2048, norm_num_groups=32,
    norm_eps=1e-5, transformer_layers=(0, 2, 10), use_linear_projection=True,
    addition_embed_type='text_time', addition_time_embed_dim=256, projection_class_embeddings_input_dim=2816)

ADDITION_TYPES = {None: 0, 'text_time': 1}

OP_CLASSES = ('conv3x3', 'linear', 'attention', 'norm', 'other')


def config_from_diffusers(cfg):
    """Translate a diffusers UNet2DConditionModel config (dict / FrozenDict) into the engine's topology dict."""
    g = cfg.get if hasattr(cfg, 'get') else (lambda k, d=None: getattr(cfg, k, d))
    ch = tuple(g('block_out_channels'))
    n = len(ch)
    heads = g('num_attention_heads') or g('attention_head_dim')      # diffusers 0.27.2 unet_2d_condition.py naming quirk
    heads = tuple(heads) if isinstance(heads, (list, tuple)) else (heads,) * n
    tl = g('transformer_layers_per_block', 1)
    tl = tuple(tl) if isinstance(tl, (list, tuple)) else (tl,) * n
    down_types = tuple(g('down_block_types'))
    up_types = g('up_block_types')
    if up_types is not None and tuple('CrossAttn' in t for t in up_types) != tuple('CrossAttn' in t for t in reversed(down_types)):
        raise NotImplementedError(f'up_block_types {tuple(up_types)} do not mirror down_block_types {down_types}')
    for key in ('class_embed_type', 'encoder_hid_dim_type'):
        if g(key) is not None:
            raise NotImplementedError(f'{key}={g(key)!r} is not implemented by the engine')
    add = g('addition_embed_type')
    if add not in ADDITION_TYPES:
        raise NotImplementedError(f'addition_embed_type={add!r} is not implemented by the engine (None and \'text_time\' are)')
    down_attn = tuple('CrossAttn' in t for t in down_types)
    # a level without attention has no transformer layers (the last entry stays: it is the mid block's depth too)
    tl = tuple(int(l) if (a or i == n - 1) else 0 for i, (l, a) in enumerate(zip(tl, down_attn)))
    extra = {}
    if add == 'text_time':
        extra = dict(addition_embed_type=add, addition_time_embed_dim=int(g('addition_time_embed_dim')),
                     projection_class_embeddings_input_dim=int(g('projection_class_embeddings_input_dim')))
    return dict(in_channels=g('in_channels'), out_channels=g('out_channels'), block_out_channels=ch,
                layers_per_block=g('layers_per_block'), down_attn=down_attn,
                num_heads=heads, cross_attention_dim=g('cross_attention_dim'), norm_num_groups=g('norm_num_groups'),
                norm_eps=g('norm_eps'), transformer_layers=tl, use_linear_projection=bool(g('use_linear_projection', False)), **extra)


class UNet2DConditionEngine(AttnProcessorTable, EngineHandle):
    OP_CLASSES = OP_CLASSES

    def __init__(self, config=None, dtype=torch.float16, device='cuda'):
        self.cfg = dict(config or SD15_CONFIG)
        assert dtype in (torch.float16, torch.bfloat16)
        self.dtype = dtype
        self.device = torch.device(device)
        c = self.cfg
        n = len(c['block_out_channels'])
        arr = lambda xs: (ctypes.c_int * n)(*[int(x) for x in xs])
        self._h = ctypes.c_void_p()
        _lib.call('mve_unet_create', ctypes.byref(self._h), _dt(dtype), c['in_channels'], c['out_channels'], n,
                  arr(c['block_out_channels']), c['layers_per_block'], arr(c['down_attn']), arr(c['num_heads']),
                  arr(c['transformer_layers']), c['cross_attention_dim'], c['norm_num_groups'], float(c['norm_eps']),
                  int(c['use_linear_projection']))
        self._declare_addition_embed()
        self._ws = None
        self._ip = (0, 1.0)          # IP-Adapter: (num_tokens, scale); see set_ip_adapter
        self._ref_keep = None
        # the attributes the reference's pipelines / runner read from a diffusers model
        self.config = SimpleNamespace(in_channels=c['in_channels'], out_channels=c['out_channels'], sample_size=64,
                                      center_input_sample=False, addition_embed_type=c.get('addition_embed_type'), **{
                                          'block_out_channels': c['block_out_channels'],
                                          'cross_attention_dim': c['cross_attention_dim']})

    def _declare_addition_embed(self):
        """Declare the SDXL 'text_time' added-condition embedding on the fresh native handle (before any parameter is loaded)."""
        add = self.cfg.get('addition_embed_type')
        if add not in ADDITION_TYPES:
            raise NotImplementedError(f'addition_embed_type={add!r} is not implemented by the engine')
        self._ack_keep = None
        if add is not None:
            _lib.call('mve_unet_set_addition_embed', self._h, ADDITION_TYPES[add], int(self.cfg['addition_time_embed_dim']),
                      int(self.cfg['projection_class_embeddings_input_dim']))

    def _bind_added_cond(self, added_cond_kwargs, B):
        """Validate diffusers' added_cond_kwargs={'text_embeds': [B, D], 'time_ids': [B, n]} (any float dtype) and bind them for the forwards
        that follow (mve_unet_bind_added_cond).  Tensors the kernel can read as they are (device, contiguous; text_embeds f32 / f16 / bf16,
        time_ids f32) are bound in place, so a caller that updates them in place needs no new binding."""
        add = self.cfg.get('addition_embed_type')
        if add is None:
            if added_cond_kwargs:
                raise ValueError('added_cond_kwargs given to an engine without an addition embedding (config addition_embed_type is None)')
            return
        if not added_cond_kwargs:
            raise ValueError("this engine has addition_embed_type='text_time': added_cond_kwargs={'text_embeds', 'time_ids'} is required")
        for key in ('text_embeds', 'time_ids'):
            if key not in added_cond_kwargs:
                raise ValueError(f"added_cond_kwargs lacks '{key}' (addition_embed_type='text_time' needs text_embeds and time_ids)")
        text, ids = added_cond_kwargs['text_embeds'], added_cond_kwargs['time_ids']
        td, P = int(self.cfg['addition_time_embed_dim']), int(self.cfg['projection_class_embeddings_input_dim'])
        for key, t in (('text_embeds', text), ('time_ids', ids)):
            if not torch.is_tensor(t) or t.dim() != 2 or not t.is_floating_point():
                raise ValueError(f"added_cond_kwargs['{key}'] must be a 2-D floating-point tensor [batch, width]")
            if t.shape[0] != B:
                raise ValueError(f"added_cond_kwargs['{key}'] has batch {t.shape[0]}, the sample has {B}")
        if text.shape[1] + ids.shape[1] * td != P:
            raise ValueError(f'added_cond_kwargs widths: text_embeds {text.shape[1]} + time_ids {ids.shape[1]} x {td} != '
                             f'projection_class_embeddings_input_dim {P}')
        if text.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            text = text.float()
        text = text.to(self.device).contiguous()
        ids = ids.to(device=self.device, dtype=torch.float32).contiguous()
        self._ack_keep = (text, ids)
        _lib.call('mve_unet_bind_added_cond', self._h, _lib.ptr(text), _dt(text), text.shape[1], _lib.ptr(ids), ids.shape[1], B)

    def set_residual_pair(self, flag=True):
        """Carry the residual stream (x + f(x) of ResnetBlock2D / BasicTransformerBlock / Transformer2DModel) as an unrounded pair -- the 16-bit tensor
        every matrix-core operand read sees plus an 8-bit E5M2 remainder (lo8, csrc/common.h) -- instead of rounding it after every block as the
        reference's half modules do (mve_unet_set_residual_mode): the end-to-end error against fp32 arithmetic falls below north_star's 1e-3
        (1.23e-3 without) for 1 more byte per stream element written and read.  ON by default for the UNet since round 5 (the native handle is
        created in this mode; MVE_RESIDUAL_PAIR=0 in the environment -- read by UNet handles only -- or set_residual_pair(False) give the reference's
        rounding points); a ControlNetEngine keeps the 16-bit stream unless its own set_residual_pair(True) is called.  Returns the previous setting."""
        return bool(_lib.raw('mve_unet_set_residual_mode')(self._h, int(bool(flag))))

    @property
    def residual_pair(self):
        return bool(_lib.raw('mve_unet_set_residual_mode')(self._h, -1))

    def set_cfg_prefix(self, flag=True):
        """Run the ops in front of the first cross-attention once for both halves of a classifier-free-guidance batch whenever a device-side probe
        finds the halves of `sample` and of the time embedding identical (mve_unet_tune_cfg_prefix; ON by default, bit-identical output either
        way, part of the plan key).  Returns the previous setting."""
        return bool(_lib.raw('mve_unet_tune_cfg_prefix')(self._h, int(bool(flag))))

    @property
    def cfg_prefix(self):
        return bool(_lib.raw('mve_unet_tune_cfg_prefix')(self._h, -1))

    def cfg_prefix_state(self):
        """Tests / tools: 1 when the last forward found its halves identical and ran the prefix once, 0 when they differed, -1 when its plan had
        no prefix (odd batch, reference attention, cross-image groups across the middle).  Synchronises."""
        rc = int(_lib.raw('mve_unet_cfg_prefix_state')(self._h))
        if rc < -1:
            raise RuntimeError('mve_unet_cfg_prefix_state: ' + _lib.last_error())
        return rc

    def enable_graph(self, flag=True):
        """Opt-in hipGraph replay of forwards whose plan and tensors (addresses) repeat -- for launch-bound small batches (mve_unet_graph)."""
        return bool(_lib.raw('mve_unet_graph')(self._h, int(bool(flag))))

    # ------------------------------------------------------------------ weights
    @classmethod
    def from_state_dict(cls, state_dict, config=None, dtype=torch.float16, device='cuda'):
        eng = cls(config, dtype, device)
        eng.load_state_dict(state_dict)
        return eng

    def load_state_dict(self, state_dict, strict=True):
        """Copy a diffusers-format state dict into engine-owned packed device storage."""
        with torch.cuda.device(self.device):
            s = _lib.stream_ptr(self.device)
            for name, t in state_dict.items():
                self._push_param(name, t, s)
            torch.cuda.current_stream(self.device).synchronize()   # source tensors may die after return
        if strict:
            missing, first = self._missing_params()
            if missing:
                raise KeyError(f'{missing} UNet parameters missing from the state dict (first: {first})')
        return self

    # ------------------------------------------------------------------ attention processors
    _REF_KEY = '__mvedit_amd_ref_store__'

    def set_ip_adapter(self, num_tokens=16, scale=1.0):
        """Install / remove (num_tokens=0) the IPAttnProcessor2_0 behaviour on every cross-attention
        (lib/models/architecture/ip_adapter/ip_adapter.py:85-110, :154-160 `set_scale`).  The to_k_ip / to_v_ip weights arrive
        through load_state_dict under their diffusers names `<block>.attn2.processor.to_{k,v}_ip.weight`."""
        self._ip = (int(num_tokens), float(scale))

    # the diffusers processor table (attn_processors / set_attn_processor: mvedit_amd/attn_processors.py) ------------------------
    def _attn_names(self):
        return attn_processor_names(self.cfg)

    def _attn_push(self, name, tensor):
        """One to_k_ip / to_v_ip weight of an installed IPAttnProcessor into the executor (stream-ordered: no synchronisation)."""
        with torch.cuda.device(self.device):
            self._push_param(name, tensor, _lib.stream_ptr(self.device))

    def _set_attention(self, cak, B, H, W, ctx_len=None):
        """Translate the reference's cross_attention_kwargs (mode / ref_dict / is_cfg_guidance) into engine state.  The
        reference fills ref_dict with one tensor per attention layer; here ref_dict receives ONE entry, the K/V store.
        Once a processor table governs (set_attn_processor was called, or the engine follows a source module) the IP branch and the
        right to use reference attention come from the table, resolved here at every forward."""
        cak = cak or {}
        mode, ref_dict = cak.get('mode'), cak.get('ref_dict')
        ip = self._ip
        if self._attn_governs:
            tr = self._attn_resolve()
            ip = (tr.ip_tokens, tr.ip_scale)
            if (mode is not None or ref_dict is not None) and not tr.reference:
                raise ValueError(f'cross_attention_kwargs mode={mode!r} / ref_dict given, but the installed attention processors hold no '
                                 f'enabled ReferenceOnlyAttnProc / ReferenceAttnProc')
            if ip[0] and ctx_len is not None and ctx_len <= ip[0]:
                raise ValueError(f'the installed IP-Adapter processors take the last {ip[0]} rows of encoder_hidden_states, which has {ctx_len}')
        skip = 1 if cak.get('is_cfg_guidance') else 0
        store, ref_mode, rH, rW = None, 0, 0, 0
        if mode is not None and ref_dict is not None:
            if mode == 'w':
                nbytes = _lib.raw('mve_unet_ref_store_bytes')(self._h, B, H, W, skip)
                store = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                ref_dict[self._REF_KEY] = (store, B, H, W, skip)
                ref_mode = 1
            elif mode in ('r', 'm'):
                store, Bs, rH, rW, sk = ref_dict.pop(self._REF_KEY) if mode == 'r' else ref_dict[self._REF_KEY]
                assert Bs == B and sk == skip, 'reference pass and read pass must have the same batch layout'
                ref_mode = 2
            else:
                raise AssertionError(mode)
        self._ref_keep = store
        _lib.call('mve_unet_set_attention', self._h, ip[0], ip[1], ref_mode, rH, rW, skip, _lib.ptr(store),
                  store.numel() if store is not None else 0)

    @property
    def weight_bytes(self):
        return _lib.raw('mve_unet_weight_bytes')(self._h)

    # ------------------------------------------------------------------ planning
    def plan(self, B, H, W, ctx_len=77, num_cross_attn_imgs=1, has_residuals=False, io_dtype=None, residuals_nhwc=False):
        ws = ctypes.c_size_t()
        n_ops = ctypes.c_int()
        flops = (ctypes.c_double * 5)()
        _lib.call('mve_unet_plan', self._h, B, H, W, ctx_len, num_cross_attn_imgs, int(has_residuals),
                  _dt(io_dtype or self.dtype), int(residuals_nhwc), ctypes.byref(ws), ctypes.byref(n_ops), flops)
        return self._plan_result(ws, n_ops, flops)

    def op_table(self):
        """[(phase, class, flops, label)] of the currently cached plan."""
        return list(self._op_rows())

    # ------------------------------------------------------------------ execution
    def _run(self, phase, sample, timestep, ctx, n_img, down_res, mid_res, out, profile=False, workspace=None,
             residuals_nhwc=False, shape=None):
        B, _, H, W = shape if shape is not None else sample.shape
        io_dtype = ctx.dtype
        assert io_dtype in (torch.float32, torch.float16, torch.bfloat16)
        ctx = ctx.to(self.device).contiguous()
        assert ctx.shape[0] == B and ctx.shape[2] == self.cfg['cross_attention_dim'], ctx.shape
        if sample is not None:
            sample = sample.to(device=self.device, dtype=io_dtype).contiguous()
        t = torch.as_tensor(timestep, dtype=torch.float32, device=self.device).reshape(-1)
        t = t.expand(B).contiguous() if t.numel() == 1 else t.contiguous()
        assert t.numel() == B
        has_res = down_res is not None and mid_res is not None
        keep = []
        res_arr = None
        if has_res:
            want = len(self.cfg['block_out_channels']) * (self.cfg['layers_per_block'] + 1)
            assert len(down_res) == want, f'expected {want} down-block residuals, got {len(down_res)}'
            # residuals produced by mvedit_amd.controlnet are logical NCHW over channels-last storage in the engine dtype:
            # hand the storage over as NHWC without a copy
            cl = lambda r: r.dim() == 4 and r.dtype == self.dtype and r.is_cuda and r.permute(0, 2, 3, 1).is_contiguous()
            if not residuals_nhwc and all(cl(r) for r in down_res) and cl(mid_res):
                residuals_nhwc = True
                down_res = [r.permute(0, 2, 3, 1) for r in down_res]
                mid_res = mid_res.permute(0, 2, 3, 1)
            rdt = self.dtype if residuals_nhwc else io_dtype
            keep = [r.to(device=self.device, dtype=rdt).contiguous() for r in down_res]
            mid_res = mid_res.to(device=self.device, dtype=rdt).contiguous()
            res_arr = (ctypes.c_void_p * want)(*[r.data_ptr() for r in keep])
        info = self.plan(B, H, W, ctx.shape[1], n_img, has_res, io_dtype, residuals_nhwc)
        ws = workspace if workspace is not None else self._workspace(info['workspace_bytes'])
        if out is None and phase != 1:
            out = torch.empty(B, self.cfg['out_channels'], H, W, dtype=io_dtype, device=self.device)
        op_ms = (ctypes.c_float * info['n_ops'])() if profile else None
        with torch.cuda.device(self.device):
            _lib.call('mve_unet_forward', self._h, phase, _lib.ptr(sample), _dt(io_dtype), _lib.ptr(t), _lib.ptr(ctx), B, H, W,
                      ctx.shape[1], n_img, res_arr, _lib.ptr(mid_res) if has_res else None, int(residuals_nhwc),
                      _lib.ptr(out), _lib.ptr(ws), ws.numel(), op_ms, _lib.stream_ptr(self.device))
        if profile:
            return out, list(op_ms)
        return out

    def __call__(self, sample, timestep, encoder_hidden_states, cross_attention_kwargs=None,
                 down_block_additional_residuals=None, mid_block_additional_residual=None, added_cond_kwargs=None,
                 return_dict=False, out=None, **unused):
        """diffusers UNet2DConditionModel.forward signature subset used by the reference."""
        self._bind_added_cond(added_cond_kwargs, sample.shape[0])
        n_img = int((cross_attention_kwargs or {}).get('num_cross_attn_imgs', 1))
        self._set_attention(cross_attention_kwargs, sample.shape[0], sample.shape[2], sample.shape[3], encoder_hidden_states.shape[1])
        res = self._run(0, sample, timestep, encoder_hidden_states, n_img, down_block_additional_residuals,
                        mid_block_additional_residual, out)
        if return_dict:
            return SimpleNamespace(sample=res)
        return (res,)

    forward = __call__

    def profile(self, sample, timestep, encoder_hidden_states, num_cross_attn_imgs=1, added_cond_kwargs=None):
        """-> (out, [(class, label, flops, ms)]) with HIP-event timing around every launch."""
        self._bind_added_cond(added_cond_kwargs, sample.shape[0])
        self._set_attention(None, *[sample.shape[i] for i in (0, 2, 3)], encoder_hidden_states.shape[1])
        out, ms = self._run(0, sample, timestep, encoder_hidden_states, num_cross_attn_imgs, None, None, None, profile=True)
        return out, [(c, lab, fl, m) for (ph, c, fl, lab), m in zip(self.op_table(), ms)]

    # 2-pass mode ---------------------------------------------------------------------------------------
    def enc(self, sample, timestep, encoder_hidden_states, cross_attention_kwargs=None, workspace=None, added_cond_kwargs=None):
        """unet_enc: runs conv_in + down blocks; the returned state handle owns the workspace holding
        (emb, down_block_res_samples, sample) for a later dec().  added_cond_kwargs (SDXL) enter here: dec() reuses the state's emb."""
        self._bind_added_cond(added_cond_kwargs, sample.shape[0])
        n_img = int((cross_attention_kwargs or {}).get('num_cross_attn_imgs', 1))
        B, _, H, W = sample.shape
        self._set_attention(cross_attention_kwargs, B, H, W, encoder_hidden_states.shape[1])
        # residual-carrying decode needs the same plan: decided at dec() time, so enc always plans with residual slots
        info = self.plan(B, H, W, encoder_hidden_states.shape[1], n_img, True, encoder_hidden_states.dtype)
        ws = workspace if workspace is not None else torch.empty(info['workspace_bytes'], dtype=torch.uint8, device=self.device)
        st = SimpleNamespace(ws=ws, shape=tuple(sample.shape), timestep=timestep, n_img=n_img)
        self._enc_dec(1, st, sample, encoder_hidden_states, None, None)
        return st

    def dec(self, state, encoder_hidden_states, down_block_additional_residuals=None, mid_block_additional_residual=None,
            cross_attention_kwargs=None):
        self._set_attention(cross_attention_kwargs, state.shape[0], state.shape[2], state.shape[3], encoder_hidden_states.shape[1])
        return self._enc_dec(2, state, None, encoder_hidden_states, down_block_additional_residuals,
                             mid_block_additional_residual)

    def _enc_dec(self, phase, st, sample, ctx, down_res, mid_res):
        B, _, H, W = st.shape
        if phase == 2 and (down_res is None or mid_res is None):
            # unet_dec without ControlNet: feed zero residuals so that the plan (and the enc state layout) is unchanged
            ch = self.cfg['block_out_channels']
            shapes = [(ch[0], H, W)]
            h, w = H, W
            for i, c in enumerate(ch):
                shapes += [(c, h, w)] * self.cfg['layers_per_block']
                if i + 1 < len(ch):
                    h, w = h // 2, w // 2
                    shapes.append((c, h, w))
            down_res = [torch.zeros(B, *s, dtype=ctx.dtype, device=self.device) for s in shapes]
            mid_res = torch.zeros(B, ch[-1], h, w, dtype=ctx.dtype, device=self.device)
        if phase == 1:
            # plan with residual slots, but phase 1 never touches them: pass dummies
            dummy = torch.zeros(8, dtype=ctx.dtype, device=self.device)
            down_res = [dummy] * (len(self.cfg['block_out_channels']) * (self.cfg['layers_per_block'] + 1))
            mid_res = dummy
            return self._run_raw(1, st, sample, ctx, down_res, mid_res)
        return self._run_raw(2, st, None, ctx, down_res, mid_res)

    def _run_raw(self, phase, st, sample, ctx, down_res, mid_res):
        if phase == 1:
            keep_checks = [r for r in down_res]   # dummies: bypass shape validation in _run
            B, _, H, W = st.shape
            io = ctx.dtype
            ctx_c = ctx.to(self.device).contiguous()
            sample = sample.to(device=self.device, dtype=io).contiguous()
            t = torch.as_tensor(st.timestep, dtype=torch.float32, device=self.device).reshape(-1)
            t = t.expand(B).contiguous() if t.numel() == 1 else t.contiguous()
            res_arr = (ctypes.c_void_p * len(keep_checks))(*[r.data_ptr() for r in keep_checks])
            with torch.cuda.device(self.device):
                _lib.call('mve_unet_forward', self._h, 1, _lib.ptr(sample), _dt(io), _lib.ptr(t), _lib.ptr(ctx_c), B, H, W,
                          ctx_c.shape[1], st.n_img, res_arr, _lib.ptr(mid_res), 0, None, _lib.ptr(st.ws), st.ws.numel(), None,
                          _lib.stream_ptr(self.device))
            return None
        return self._run(2, None, st.timestep, ctx, st.n_img, down_res, mid_res, None, workspace=st.ws, shape=st.shape)


def unet_enc(unet, sample, timestep, encoder_hidden_states, cross_attention_kwargs=None, added_cond_kwargs=None):
    """lib/models/architecture/diffusers.py:57-99.  Returns (emb, down_block_res_samples, sample) in the reference;
    here the three live inside one opaque state object, returned in the same 3-tuple positions for drop-in use."""
    st = unet.enc(sample, timestep, encoder_hidden_states, cross_attention_kwargs, added_cond_kwargs=added_cond_kwargs)
    return st, st, st


def unet_dec(unet, emb, down_block_res_samples, sample, encoder_hidden_states, cross_attention_kwargs=None,
             down_block_additional_residuals=None, mid_block_additional_residual=None):
    """lib/models/architecture/diffusers.py:102-164."""
    return unet.dec(emb, encoder_hidden_states, down_block_additional_residuals, mid_block_additional_residual,
                    cross_attention_kwargs)
