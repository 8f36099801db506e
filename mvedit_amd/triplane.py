"""Mirrors of the reference's tri-plane radiance decoders for one scene, forward only: `TriPlaneDecoder.point_decode` /
`point_density_decode` (lib/models/decoders/triplane_decoder.py:107-204) and `TriPlaneiNGPDecoder.point_decode`
(lib/models/decoders/triplane_ingp_decoder.py:142-212) -> mve_triplane_decode (csrc/triplane.hip): plane fetches, the base / density /
colour MLPs, the SH direction encoding and (iNGP variant) the hash-grid branch in ONE launch, one wave per 64 points.
Two topologies are built, recognised from the state dict's keys (or from the layer lists of `from_config`):
  default   the classes' constructor defaults: one Linear in base_net / density_net / ingp_base_net, Linear-act-Linear colour net over
            cat[act(base), SH_4(dir)], dir_layers=None;
  dir-net   what every config file of the reference asks for (base_layers=[3C, H], density_layers=[H, 1], color_layers=[H, 3],
            dir_layers=[16, H]): dir_net = Linear(16 -> H), rgb = sat(sigmoid(color_net(act(base_x + dir_net(SH_4(dir)))))), color_net = one
            Linear(H -> 3).  H in {64, 128}.
Anything else (deeper stacks, a mixture of the two, scene_base, code dropout, other widths) raises NotImplementedError -- it is never computed
another way.  Out of scope: the `preprocessor` (VAEDecoder) / code_activation in front of point_decode (the planes handed in are already
pre-processed, as in the reference's own point_decode), 16-bit code planes, more than one scene per call, second-order grid_sample.
Rendering: `render_rays` is VolumeRenderer.forward's eval branch (lib/models/decoders/base_volume_renderer.py:264-329) as ONE launch
(mve_triplane_render_rays: march + decode + composite per ray, the direction-only part of the colour path computed once per ray), which is
what `NeRFRenderer.render(decoder, code, ...)` calls for a tri-plane decoder; `render_rays(..., fused=False)` is the reference-shaped host loop
over march_rays / point_decode / composite_rays / compact_alive.  `TriPlaneVolumeRenderer` adds the training branch (march -> density ->
cull -> decode -> composite) and `update_extra_state(code, ...)`; it refuses capacity=, compute_normal in training, more than one scene and
pre_gamma / post_gamma.
Gradients: `point_decode_autograd` carries autograd history w.r.t. the code planes and `parameters()` (every Linear and the hash table)
through mve_triplane_backward -- what nerf_optim (lib/pipelines/mvedit_3d_pipeline.py:507-633) needs to optimise a TriPlaneiNGPDecoder
scene.  Plain `point_decode` is forward only and refuses tensors that require grad instead of silently cutting the graph.  No gradient
w.r.t. xyzs / dirs (the sample positions are not optimised)."""
import ctypes

import numpy as np
import torch

from . import _lib
from .nerf import grid_meta

_ACT = dict(relu=0, silu=1, softplus=2, trunc_exp=3)


class _Desc(ctypes.Structure):
    _fields_ = [('d_xyz', ctypes.c_void_p), ('d_dirs', ctypes.c_void_p), ('d_code', ctypes.c_void_p),
                ('N', ctypes.c_int32), ('C', ctypes.c_int32), ('h', ctypes.c_int32), ('w', ctypes.c_int32),
                ('axes', ctypes.c_int32 * 6), ('flip_z', ctypes.c_int32),
                ('d_base_wT', ctypes.c_void_p), ('d_base_b', ctypes.c_void_p), ('hidden', ctypes.c_int32), ('hidden2', ctypes.c_int32),
                ('d_ingp_wT', ctypes.c_void_p), ('d_ingp_b', ctypes.c_void_p), ('d_table', ctypes.c_void_p),
                ('n_levels', ctypes.c_int32), ('bound', ctypes.c_float),
                ('level_scale', ctypes.c_void_p), ('level_res', ctypes.c_void_p), ('level_offset', ctypes.c_void_p), ('level_size', ctypes.c_void_p),
                ('d_dens_w', ctypes.c_void_p), ('d_dens_b', ctypes.c_void_p), ('d_col1_wT', ctypes.c_void_p), ('d_col1_b', ctypes.c_void_p),
                ('d_col2_w', ctypes.c_void_p), ('d_col2_b', ctypes.c_void_p),
                ('activation', ctypes.c_int32), ('sigma_activation', ctypes.c_int32), ('sigmoid_saturation', ctypes.c_float),
                ('d_sigmas', ctypes.c_void_p), ('d_rgbs', ctypes.c_void_p),
                ('topology', ctypes.c_int32), ('d_dir_wT', ctypes.c_void_p), ('d_dir_b', ctypes.c_void_p)]


class _Grads(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ('d_code', 'd_table', 'd_base_w', 'd_base_b', 'd_ingp_w', 'd_ingp_b', 'd_dens_w', 'd_dens_b',
                                                'd_col1_w', 'd_col1_b', 'd_col2_w', 'd_col2_b', 'd_dir_w', 'd_dir_b')]


TOPOLOGY_DEFAULT, TOPOLOGY_DIRNET = 0, 1
_NETS = ('base_net.', 'density_net.', 'color_net.', 'dir_net.', 'ingp_base_net.')


class TriPlaneDecoder:
    """plane_cfg / flip_z / activation / sigma_activation / sigmoid_saturation as the reference constructor; weights come in through
    load_state_dict with the reference module's names (base_net.0.*, density_net.0.*, color_net.0.*, color_net.2.*)."""

    takes_code = True                   # NeRFRenderer.render hands `code` to render_rays

    def __init__(self, plane_cfg=('xy', 'xz', 'yz'), activation='silu', sigma_activation='trunc_exp', sigmoid_saturation=0.001, flip_z=False,
                 bound=1.0, min_near=0.2, max_steps=256, device='cuda'):
        assert len(plane_cfg) == 3 and all(len(p) == 2 and set(p) <= set('xyz') for p in plane_cfg), plane_cfg
        self.axes = [dict(x=0, y=1, z=2)[a] for p in plane_cfg for a in p]
        self.activation, self.sigma_activation = _ACT[activation.lower()], _ACT[sigma_activation.lower()]
        assert self.activation < 3
        self.sigmoid_saturation, self.flip_z, self.bound, self.device = float(sigmoid_saturation), bool(flip_z), float(bound), torch.device(device)
        self.min_near, self.max_steps = float(min_near), int(max_steps)          # VolumeRenderer's defaults (base_volume_renderer.py:35-36)
        self.w = {}
        self.hash = None
        self._aabb = None

    # ---- parameters ------------------------------------------------------------------------------------------------------------
    _NAMES = {'base_net.0.weight': ('base_wT', True), 'base_net.0.bias': ('base_b', False),
              'density_net.0.weight': ('dens_w', False), 'density_net.0.bias': ('dens_b', False),
              'color_net.0.weight': ('col1_wT', True), 'color_net.0.bias': ('col1_b', False),
              'color_net.2.weight': ('col2_w', False), 'color_net.2.bias': ('col2_b', False),
              'ingp_base_net.0.weight': ('ingp_wT', True), 'ingp_base_net.0.bias': ('ingp_b', False)}

    # the dir-net topology: its one-Linear colour net is the kernel's output layer (col2), dir_net goes in transposed like every [in][out] weight
    _NAMES_DIRNET = {'base_net.0.weight': ('base_wT', True), 'base_net.0.bias': ('base_b', False),
                     'density_net.0.weight': ('dens_w', False), 'density_net.0.bias': ('dens_b', False),
                     'dir_net.0.weight': ('dir_wT', True), 'dir_net.0.bias': ('dir_b', False),
                     'color_net.0.weight': ('col2_w', False), 'color_net.0.bias': ('col2_b', False),
                     'ingp_base_net.0.weight': ('ingp_wT', True), 'ingp_base_net.0.bias': ('ingp_b', False)}
    _UNBUILT = ('only two tri-plane decoder topologies are built: the default (one Linear per base / density / ingp net, Linear-act-Linear colour '
                'net over cat[act(base), SH], no dir_net) and the dir-net one (one Linear per base / density / ingp / dir / colour net); widths 64 '
                'or 128, no scene_base')
    topology, _names = TOPOLOGY_DEFAULT, _NAMES
    cfg_layers = None                   # from_config: (topology, 3C, hidden, hidden2 or None) the state dict has to agree with

    def load_state_dict(self, sd):
        keys = [k for k in sd if k.startswith(_NETS) or k.startswith('scene_base')]          # preprocessor.* and the like: not read by point_decode
        for name in keys:
            if name.startswith('scene_base'):
                raise NotImplementedError(f'{name}: {self._UNBUILT}')
        dirnet = any(k.startswith('dir_net.') for k in keys)
        names = self._NAMES_DIRNET if dirnet else self._NAMES
        for name in keys:
            if name not in names:            # a deeper stack (base_net.2.*, dir_net.2.*, a third colour Linear) or, with dir_net.*, the default's color_net.2.*
                raise NotImplementedError(f'{name}: {self._UNBUILT}')
        need = [n for n in names if not n.startswith('ingp_base_net.') or self.hash is not None]
        if self.hash is not None:
            need.append('encoder.params')
        missing = [n for n in need if n not in sd]
        if missing:
            raise KeyError(f'tri-plane decoder ({"dir-net" if dirnet else "default"} topology): missing parameters {missing}')
        shp = {n: tuple(sd[n].shape) for n in need}
        H = shp['base_net.0.weight'][0]
        if H not in (64, 128):
            raise NotImplementedError(f'base_net.0.weight: hidden width {H}; {self._UNBUILT}')
        if dirnet:
            if shp['color_net.0.weight'] != (3, H):
                raise NotImplementedError(f'color_net.0.weight: shape {shp["color_net.0.weight"]}, expected (3, {H}); {self._UNBUILT}')
            assert shp['dir_net.0.weight'] == (H, 16) and shp['dir_net.0.bias'] == (H,), 'unexpected dir_net widths'
            H2 = None
        else:
            H2 = shp['color_net.0.weight'][0]
            if H2 not in (64, 128):
                raise NotImplementedError(f'color_net.0.weight: hidden width {H2}; {self._UNBUILT}')
            assert shp['color_net.0.weight'][1] == H + 16 and shp['color_net.2.weight'] == (3, H2), 'unexpected layer widths'
        assert int(np.prod(shp['density_net.0.weight'])) == H, 'unexpected layer widths'
        if self.cfg_layers is not None:
            got = (TOPOLOGY_DIRNET if dirnet else TOPOLOGY_DEFAULT, shp['base_net.0.weight'][1], H, H2)
            if got != self.cfg_layers:
                raise ValueError(f'tri-plane decoder: the state dict (topology, inputs, hidden, hidden2) = {got} does not match the config {self.cfg_layers}')
        self.topology, self._names = (TOPOLOGY_DIRNET if dirnet else TOPOLOGY_DEFAULT), names
        self.w = {}
        # reference name -> fp32 tensor in the reference's own layout (the leaves of point_decode_autograd)
        self.params = {n: sd[n].detach().to(self.device, torch.float32).clone().contiguous() for n in sd if n in names or n == 'encoder.params'}
        self._packed_sig = None
        self._pack()
        return self

    @classmethod
    def from_config(cls, cfg, device='cuda', **kwargs):
        """The reference's decoder dict as its config files write it (configs/**: model.decoder) -> a decoder waiting for load_state_dict.
        Read: plane_cfg, flip_z, base_layers, density_layers, color_layers, use_dir_enc, dir_layers, activation, sigma_activation,
        sigmoid_saturation, interp_mode, bound, min_near, max_steps (+ base_resolution, max_resolution, n_levels for TriPlaneiNGPDecoder).  What
        point_decode and render_rays do not read (type, preprocessor, code_reshape, preproc_size, weight_culling_th, ...) is ignored; settings that change point_decode
        and are not built are refused.  `kwargs` go to the constructor (e.g. log2_hashmap_size)."""
        cfg = dict(cfg)
        if not cfg.get('use_dir_enc', True):
            raise NotImplementedError('use_dir_enc=False: the colour net without a direction encoding is not built')
        if cfg.get('interp_mode', 'bilinear') != 'bilinear':
            raise NotImplementedError(f'interp_mode={cfg["interp_mode"]!r}: only bilinear plane sampling is built')
        if cfg.get('scene_base_size') is not None:
            raise NotImplementedError('scene_base_size: scene_base is not built')
        if cfg.get('code_dropout', 0.0) > 0:
            raise NotImplementedError('code_dropout > 0 is not built (a training-time Dropout2d on the planes)')
        if cfg.get('ingp_base_layers', 1) != 1:
            raise NotImplementedError(f'ingp_base_layers={cfg["ingp_base_layers"]}: {cls._UNBUILT}')
        base, dens = list(cfg.get('base_layers', [3 * 32, 128])), list(cfg.get('density_layers', [128, 1]))
        col, dirl = list(cfg.get('color_layers', [128, 128, 3])), cfg.get('dir_layers')
        H = base[-1]
        ok = len(base) == 2 and base[0] % 3 == 0 and H in (64, 128) and dens == [H, 1]
        if dirl is None:             # the constructor widens color_layers[0] by the 16 SH features itself
            ok = ok and len(col) == 3 and col[0] == H and col[1] in (64, 128) and col[2] == 3
            layers = (TOPOLOGY_DEFAULT, base[0], H, col[1] if ok else None)
        else:
            ok = ok and list(dirl) == [16, H] and col == [H, 3]
            layers = (TOPOLOGY_DIRNET, base[0], H, None)
        if not ok:
            raise NotImplementedError(f'base_layers={base}, density_layers={dens}, color_layers={col}, dir_layers={dirl}: {cls._UNBUILT}')
        kw = {k: cfg[k] for k in ('plane_cfg', 'activation', 'sigma_activation', 'sigmoid_saturation', 'flip_z', 'bound', 'min_near', 'max_steps') if k in cfg}
        if cls._HASH_KEYS:
            kw.update({k: cfg[k] for k in cls._HASH_KEYS if k in cfg})
        dec = cls(device=device, **kw, **kwargs)
        dec.cfg_layers, dec.topology = layers, layers[0]
        return dec

    _HASH_KEYS = ()

    def _pack(self, tensors=None):
        """kernel-side copies of the parameters: weight matrices transposed to [in][out] (one input's fan-out = one contiguous scalar load).
        Without `tensors` the copies are rebuilt only when a parameter changed -- not on every call of the NeRF sampling hot path.  "Changed" is
        read off (object identity, storage address, torch's version counter): optimiser steps, in-place ops and load_state_dict bump the counter or
        replace the tensor.  Edits THROUGH `.data` (`p.data.copy_()`, `p.data.clamp_()`) and `set_` bump nothing: call `invalidate()` after them
        (ADVICE round 4).  Every packed tensor is a COPY (`.clone()`), never an alias of the parameter, so a missed edit leaves all of them equally
        stale instead of a mix of fresh aliases and stale transposes."""
        src = self.params if tensors is None else tensors
        if tensors is None:
            sig = tuple((n, id(t), t.data_ptr(), t._version) for n, t in src.items())
            if getattr(self, '_packed_sig', None) == sig:
                return
            self._packed_sig = sig
        else:
            self._packed_sig = None
        for name, t in src.items():
            if name in self._names:
                key, transpose = self._names[name]
                t = t.detach()
                self.w[key] = t.t().clone(memory_format=torch.contiguous_format) if transpose else t.clone()      # (.t().contiguous() aliases a [1, N] weight)
            elif name == 'encoder.params':
                self.w['table'] = t.detach().reshape(-1, 2).clone()

    def invalidate(self):
        """Forget the packed copies: the next call repacks from parameters().  Needed only after edits torch's version counter does not see
        (`.data` writes, `set_`)."""
        self._packed_sig = None

    def parameters(self):
        """reference name -> tensor (fp32, the reference module's layout); mark them requires_grad_(True) and optimise them with any torch optimiser"""
        return self.params

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    def point_decode_autograd(self, xyzs, dirs, code, density_only=False):
        """point_decode whose outputs carry autograd history w.r.t. `code` and parameters() (native backward, mve_triplane_backward)"""
        assert len(xyzs) == 1 and code.shape[0] == 1, 'one scene per call (as every MVEdit pipeline)'
        names = sorted(self.params)
        d = None if (density_only or dirs is None) else dirs[0]
        sig, rgb = _TriDecodeFn.apply(self, names, xyzs[0], d, code, *[self.params[n] for n in names])
        return sig, (None if d is None else rgb), [sig.shape[0]]

    def point_decode(self, xyzs, dirs, code, density_only=False, use_2nd_order=False):
        """xyzs: [1, (N, 3)] (list or tensor), dirs likewise or None, code [1, 3, C, h, w] -> (sigmas [N], rgbs [N,3] | None, [N])"""
        assert not use_2nd_order, 'lib/ops/cuda_gridsample (second-order grid_sample) is not part of this engine'
        assert len(xyzs) == 1 and code.shape[0] == 1, 'one scene per call (as every MVEdit pipeline)'
        xyz = xyzs[0]
        d = None if (density_only or dirs is None) else dirs[0]
        # forward only: PARAMETERS that are marked trainable (nerf_optim's optimiser holds them) are read as constants; an input that requires
        # grad is refused -- its gradient would silently be missing
        for t in (xyz, d, code):
            if t is not None and torch.is_grad_enabled() and t.requires_grad:
                raise NotImplementedError('tri-plane decoders: point_decode is the forward only -- use point_decode_autograd for gradients '
                                          '(or call under torch.no_grad())')
        self._pack()
        return self._forward(xyz, d, code)

    def _prep(self, xyz, d, code):
        xyz = xyz.detach().to(self.device, torch.float32).reshape(-1, 3).contiguous()
        N = xyz.shape[0]
        if d is not None:
            d = d.detach().to(self.device, torch.float32).reshape(-1, 3).contiguous()
            assert d.shape[0] == N
        _, _, C, h, w = code.shape
        cl = code[0].detach().to(self.device, torch.float32).permute(0, 2, 3, 1).contiguous()      # [3][h][w][C]
        W = self.w
        assert W['base_wT'].shape[0] == 3 * C, (W['base_wT'].shape, C)
        return xyz, d, cl, N, C, h, w

    def _desc(self, xyz, d, cl, N, C, h, w, sig, rgb):
        W = self.w
        ds = _Desc()
        ds.d_xyz, ds.d_dirs, ds.d_code = (xyz.data_ptr() if xyz is not None else None), (d.data_ptr() if d is not None else None), cl.data_ptr()
        ds.N, ds.C, ds.h, ds.w = N, C, h, w
        for k in range(6):
            ds.axes[k] = self.axes[k]
        ds.flip_z = int(self.flip_z)
        ds.d_base_wT, ds.d_base_b = W['base_wT'].data_ptr(), W['base_b'].data_ptr()
        dirnet = self.topology == TOPOLOGY_DIRNET
        ds.hidden = W['base_wT'].shape[1]
        ds.hidden2 = 0 if dirnet else W['col1_wT'].shape[1]             # ignored by the dir-net topology
        keep = []
        if self.hash is not None:
            meta = self.hash['meta']
            arr = (np.array([m[0] for m in meta], np.float32), np.array([m[1] for m in meta], np.uint32),
                   np.array([m[2] for m in meta], np.uint32), np.array([m[3] for m in meta], np.uint32))
            keep.append(arr)
            ds.d_ingp_wT, ds.d_ingp_b, ds.d_table = W['ingp_wT'].data_ptr(), W['ingp_b'].data_ptr(), W['table'].data_ptr()
            ds.n_levels = len(meta)
            ds.level_scale, ds.level_res, ds.level_offset, ds.level_size = (a.ctypes.data for a in arr)
        ds.bound = self.bound               # the hash grid's normalisation and the marched cube of mve_triplane_render_rays
        ds.d_dens_w, ds.d_dens_b = W['dens_w'].data_ptr(), W['dens_b'].data_ptr()
        ds.d_col2_w, ds.d_col2_b = W['col2_w'].data_ptr(), W['col2_b'].data_ptr()
        if dirnet:
            ds.topology, ds.d_dir_wT, ds.d_dir_b = TOPOLOGY_DIRNET, W['dir_wT'].data_ptr(), W['dir_b'].data_ptr()
        else:
            ds.d_col1_wT, ds.d_col1_b = W['col1_wT'].data_ptr(), W['col1_b'].data_ptr()
        ds.activation, ds.sigma_activation, ds.sigmoid_saturation = self.activation, self.sigma_activation, self.sigmoid_saturation
        ds.d_sigmas, ds.d_rgbs = (sig.data_ptr() if sig is not None else None), (rgb.data_ptr() if rgb is not None else None)
        return ds, keep

    def _forward(self, xyz, d, code):
        xyz, d, cl, N, C, h, w = self._prep(xyz, d, code)
        sig = torch.empty(N, dtype=torch.float32, device=self.device)
        rgb = torch.empty(N, 3, dtype=torch.float32, device=self.device) if d is not None else None
        ds, keep = self._desc(xyz, d, cl, N, C, h, w, sig, rgb)
        with torch.cuda.device(self.device):
            _lib.call('mve_triplane_decode', ctypes.byref(ds), _lib.stream_ptr(self.device))
        del keep
        return sig, rgb, [N]

    def _backward(self, xyz, d, code, g_sig, g_rgb, need_code):
        """-> (grad code [1,3,C,h,w] or None, {reference name: gradient})"""
        xyz, d, cl, N, C, h, w = self._prep(xyz, d, code)
        dev, W = self.device, self.w
        dirnet = self.topology == TOPOLOGY_DIRNET
        H = W['base_wT'].shape[1]
        nl = len(self.hash['meta']) if self.hash is not None else 0
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=dev)
        g = {'base_net.0.weight': z(H, 3 * C), 'base_net.0.bias': z(H), 'density_net.0.weight': z(1, H), 'density_net.0.bias': z(1)}
        if dirnet:
            g.update({'dir_net.0.weight': z(H, 16), 'dir_net.0.bias': z(H), 'color_net.0.weight': z(3, H), 'color_net.0.bias': z(3)})
        else:
            H2 = W['col1_wT'].shape[1]
            g.update({'color_net.0.weight': z(H2, H + 16), 'color_net.0.bias': z(H2), 'color_net.2.weight': z(3, H2), 'color_net.2.bias': z(3)})
        if nl:
            g.update({'ingp_base_net.0.weight': z(H, 2 * nl), 'ingp_base_net.0.bias': z(H), 'encoder.params': torch.zeros_like(self.params['encoder.params'])})
        g_code = z(3, h, w, C) if need_code else None
        gs = _Grads()
        gs.d_code, gs.d_table = (g_code.data_ptr() if need_code else None), (g['encoder.params'].data_ptr() if nl else None)
        gs.d_base_w, gs.d_base_b = g['base_net.0.weight'].data_ptr(), g['base_net.0.bias'].data_ptr()
        if nl:
            gs.d_ingp_w, gs.d_ingp_b = g['ingp_base_net.0.weight'].data_ptr(), g['ingp_base_net.0.bias'].data_ptr()
        gs.d_dens_w, gs.d_dens_b = g['density_net.0.weight'].data_ptr(), g['density_net.0.bias'].data_ptr()
        if dirnet:
            gs.d_dir_w, gs.d_dir_b = g['dir_net.0.weight'].data_ptr(), g['dir_net.0.bias'].data_ptr()
            gs.d_col2_w, gs.d_col2_b = g['color_net.0.weight'].data_ptr(), g['color_net.0.bias'].data_ptr()
        else:
            gs.d_col1_w, gs.d_col1_b = g['color_net.0.weight'].data_ptr(), g['color_net.0.bias'].data_ptr()
            gs.d_col2_w, gs.d_col2_b = g['color_net.2.weight'].data_ptr(), g['color_net.2.bias'].data_ptr()
        ds, keep = self._desc(xyz, d, cl, N, C, h, w, None, None)
        if dirnet:
            nbytes = _lib.raw('mve_triplane_dirnet_backward_workspace_bytes')(N, C, H, nl)
        else:
            nbytes = _lib.raw('mve_triplane_backward_workspace_bytes')(N, C, H, H2, nl)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        g_sig = g_sig.to(dev, torch.float32).contiguous()
        g_rgb = g_rgb.to(dev, torch.float32).contiguous() if (g_rgb is not None and d is not None) else None
        with torch.cuda.device(dev):
            _lib.call('mve_triplane_backward', ctypes.byref(ds), _lib.ptr(g_sig), _lib.ptr(g_rgb), ctypes.byref(gs), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
        del keep
        return (g_code.permute(0, 3, 1, 2)[None].contiguous() if need_code else None), g

    def point_density_decode(self, xyzs, code, **kwargs):
        sigmas, _, num_points = self.point_decode(xyzs, None, code, density_only=True, **kwargs)
        return sigmas, num_points

    # ---- VolumeRenderer.forward, eval branch --------------------------------------------------------------------------------------
    @property
    def aabb(self):
        if self._aabb is None:
            self._aabb = torch.tensor([-self.bound] * 3 + [self.bound] * 3, dtype=torch.float32, device=self.device)
        return self._aabb

    def render_rays(self, rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma=0.0, T_thresh=1e-2, return_counts=False, fused=None):
        """rays_o, rays_d [N,3] of one scene, code [1, 3, C, h, w], density_bitfield [grid_size^3 / 8] u8 -> (weights_sum [N], depth [N] (sum of
        w / t), image [N,3][, counts [N] int32]).  Forward only.  fused=None takes the faster form as measured (profiles/triplane_render.txt): the
        fused launch without a hash branch (1.9 against 2.0 ms), the host loop with one (the H = 64 hash instantiations spill 5-7 KB per lane to
        scratch: 17.9 against 3.5 ms, untuned); True / False force one.  fused=True: one launch (mve_triplane_render_rays); counts are the samples
        each ray decoded.  fused=False: the reference's host loop (base_volume_renderer.py:286-322) on march_rays / point_decode /
        composite_rays / compact_alive, one host read per chunk of at most 8 steps; counts are the samples marched, which include those a
        chunk marched past a ray's termination."""
        assert code.dim() == 5 and code.shape[0] == 1, 'one scene per call (as every MVEdit pipeline)'
        for t in (rays_o, rays_d, code):
            if torch.is_grad_enabled() and t.requires_grad:
                raise NotImplementedError('tri-plane decoders: render_rays is the forward only -- the differentiable path is '
                                          'TriPlaneVolumeRenderer.forward in training mode (or call under torch.no_grad())')
        rays_o = rays_o.detach().to(self.device, torch.float32).contiguous().view(-1, 3)
        rays_d = rays_d.detach().to(self.device, torch.float32).contiguous().view(-1, 3)
        N = rays_o.shape[0]
        assert rays_d.shape[0] == N
        bits = density_bitfield.to(self.device).contiguous().view(-1)
        assert bits.dtype == torch.uint8 and bits.numel() * 8 == int(grid_size) ** 3, (bits.dtype, bits.numel(), grid_size)
        self._pack()
        if fused is None:
            fused = self.hash is None
        if not fused:
            return self._render_rays_loop(rays_o, rays_d, code, bits, int(grid_size), float(dt_gamma), float(T_thresh), return_counts)
        ws = torch.empty(N, dtype=torch.float32, device=self.device)
        depth = torch.empty(N, dtype=torch.float32, device=self.device)
        image = torch.empty(N, 3, dtype=torch.float32, device=self.device)
        counts = torch.empty(N, dtype=torch.int32, device=self.device) if return_counts else None
        _, _, C, h, w = code.shape
        cl = code[0].detach().to(self.device, torch.float32).permute(0, 2, 3, 1).contiguous()      # [3][h][w][C]
        assert self.w['base_wT'].shape[0] == 3 * C, (self.w['base_wT'].shape, C)
        ds, keep = self._desc(None, None, cl, 0, C, h, w, None, None)
        with torch.cuda.device(self.device):
            _lib.call('mve_triplane_render_rays', ctypes.byref(ds), _lib.ptr(rays_o), _lib.ptr(rays_d), N, _lib.ptr(bits), int(grid_size),
                      _lib.ptr(self.aabb), self.min_near, float(dt_gamma), int(self.max_steps), float(T_thresh), _lib.ptr(ws), _lib.ptr(depth),
                      _lib.ptr(image), _lib.ptr(counts), _lib.stream_ptr(self.device))
        del keep
        return (ws, depth, image, counts) if return_counts else (ws, depth, image)

    def _render_rays_loop(self, rays_o, rays_d, code, bits, grid_size, dt_gamma, T_thresh, return_counts):
        from . import raymarching as rm
        dev, N = self.device, rays_o.shape[0]
        ws = torch.zeros(N, dtype=torch.float32, device=dev)
        depth = torch.zeros(N, dtype=torch.float32, device=dev)
        image = torch.zeros(N, 3, dtype=torch.float32, device=dev)
        counts = torch.zeros(N, dtype=torch.int32, device=dev) if return_counts else None
        if N == 0:
            return (ws, depth, image, counts) if return_counts else (ws, depth, image)
        nears, fars = rm.near_far_from_aabb(rays_o, rays_d, self.aabb, self.min_near)
        rays_alive = torch.arange(N, dtype=torch.int32, device=dev)
        rays_t = nears.clone()
        n_alive, step = N, 0
        while step < self.max_steps and n_alive > 0:
            n_step = min(max(N // n_alive, 1), 8)
            xyzs, dirs, ts = rm.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, self.bound, bits, 1, grid_size, nears, fars,
                                           False, dt_gamma, self.max_steps)
            if return_counts:
                counts.index_add_(0, rays_alive[:n_alive].long().repeat_interleave(n_step), (ts[:, 1] > 0).int())
            sigmas, rgbs, _ = self._forward(xyzs, dirs, code)
            rm.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, ts, ws, depth, image, T_thresh)
            rays_alive, n_kept = rm.compact_alive(rays_alive, n_alive)
            n_alive = int(n_kept.item())              # the reference's boolean-mask compaction reads the count here as well
            step += n_step
        return (ws, depth, image, counts) if return_counts else (ws, depth, image)


class TriPlaneiNGPDecoder(TriPlaneDecoder):
    """+ the hash-grid branch: base_x = base_net(plane features) + ingp_base_net(HashGrid((xyz + bound) / (2 bound))); the level table follows
    the constructor (triplane_ingp_decoder.py:102-114: 2 features per level, log2_hashmap_size 19, Smoothstep)."""

    _HASH_KEYS = ('base_resolution', 'max_resolution', 'n_levels')

    def __init__(self, *args, base_resolution=16, max_resolution=320, n_levels=12, log2_hashmap_size=19, **kwargs):
        super().__init__(*args, **kwargs)
        meta, rows = grid_meta(n_levels, base_resolution, max_resolution, self.bound, log2_hashmap_size)
        self.hash = dict(meta=meta, rows=rows)

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        for k in ('ingp_wT', 'ingp_b', 'table'):
            if k not in self.w:
                raise KeyError(f'TriPlaneiNGPDecoder: missing parameter for {k}')
        assert self.w['table'].shape[0] == self.hash['rows'], (self.w['table'].shape, self.hash['rows'])
        assert self.w['ingp_wT'].shape == (2 * len(self.hash['meta']), self.w['base_wT'].shape[1])
        return self


class _TriDecodeFn(torch.autograd.Function):
    """(sigmas, rgbs) = decoder.point_decode with the native backward w.r.t. the code planes and the decoder's parameters"""

    @staticmethod
    def forward(ctx, dec, names, xyz, dirs, code, *params):
        dec._pack(dict(zip(names, params)))
        sig, rgb, _ = dec._forward(xyz, dirs, code)
        ctx.dec, ctx.names, ctx.has_dirs = dec, names, dirs is not None
        ctx.save_for_backward(xyz, dirs if dirs is not None else xyz.new_zeros(0), code, *params)
        if rgb is None:
            rgb = sig.new_zeros(0, 3)
            ctx.mark_non_differentiable(rgb)
        return sig, rgb

    @staticmethod
    def backward(ctx, g_sig, g_rgb):
        xyz, dirs, code, *params = ctx.saved_tensors
        dec = ctx.dec
        dec._pack(dict(zip(ctx.names, params)))
        if g_sig is None:
            g_sig = xyz.new_zeros(xyz.reshape(-1, 3).shape[0])
        g_code, g = dec._backward(xyz, dirs if ctx.has_dirs else None, code, g_sig, g_rgb if ctx.has_dirs else None, ctx.needs_input_grad[4])
        out = [g[n].reshape(p.shape) if ctx.needs_input_grad[5 + k] else None for k, (n, p) in enumerate(zip(ctx.names, params))]
        return (None, None, None, None, g_code.to(code.dtype) if g_code is not None else None, *out)


class TriPlaneVolumeRenderer:
    """Mirror of the reference's VolumeRenderer.forward(rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma, perturb)
    (lib/models/decoders/base_volume_renderer.py:179-343) and update_extra_state (:105-177) for ONE scene over a tri-plane decoder
    (nerf.VolumeRenderer is the iNGP decoder's and stays as it is).  Eval: the decoder's render_rays.  Training: march_rays_train ->
    point_density_decode under no_grad -> composite -> cull_samples -> point_decode -> batch_composite_rays_train; the last decode carries
    autograd history (point_decode_autograd, native backward) when `code` or any of the decoder's parameters() requires grad.
    Refused with NotImplementedError: capacity= (the host-read-free form needs a counted tri-plane decode, which does not exist),
    compute_normal=True in training (second-order grid_sample), more than one scene, pre_gamma / post_gamma."""

    def __init__(self, decoder, weight_culling_th=1e-3, pre_gamma=None, post_gamma=None):
        if pre_gamma is not None or post_gamma is not None:
            raise NotImplementedError('pre_gamma / post_gamma: the gamma pair around the eval compositing is not built')
        self.decoder = decoder
        self.bound, self.min_near, self.max_steps = decoder.bound, decoder.min_near, decoder.max_steps
        self.weight_culling_th = weight_culling_th
        self.training = False

    @staticmethod
    def _one_scene(code, *per_scene):
        """code [1, 3, C, h, w]; rays and the bitfield with or without the leading scene axis -> the single scene's tensors"""
        if not (torch.is_tensor(code) and code.dim() == 5 and code.shape[0] == 1):
            raise NotImplementedError(f'code: one scene of shape [1, 3, C, h, w] per call (got {tuple(code.shape) if torch.is_tensor(code) else type(code)})')
        out = []
        for name, t, nd in per_scene:
            if isinstance(t, (list, tuple)) or t.dim() == nd + 1:
                if len(t) != 1:
                    raise NotImplementedError(f'{name}: more than one scene ({len(t)}) is not built')
                t = t[0]
            out.append(t)
        return out

    def update_extra_state(self, code, density_grid, density_bitfield, iter_density, density_thresh=0.01, decay=0.9, S=128):
        """nerf.VolumeRenderer.update_extra_state with point_density_decode(xyzs, code) as the density source: density_grid [1, H^3] f32 and
        density_bitfield [1, H^3/8] u8 are updated IN PLACE; returns iter_density + 1 and the threshold used.  Random draws (jitter,
        partial-update cells) come from torch's generator, as in the reference."""
        from . import raymarching as rm
        dec, dev = self.decoder, self.decoder.device
        self._one_scene(code)
        assert density_grid.shape[0] == 1 and density_grid.dtype == torch.float32 and density_grid.is_contiguous()
        n_cells = density_grid.shape[-1]
        H = int(round(n_cells ** (1.0 / 3.0)))
        tmp = torch.full_like(density_grid, -1)
        if iter_density < 16:                                         # full update, one launch over the whole grid
            N, coords = n_cells, None
        else:                                                         # partial update: N random cells + N occupied cells
            N = n_cells // 4
            coords = torch.randint(0, H, (N, 3), device=dev)
            occ = torch.nonzero(density_grid[0] > 0).squeeze(-1)
            occ = occ[torch.randint(0, occ.shape[0], [N], dtype=torch.long, device=dev)]
            coords = torch.cat([coords.int(), rm.morton3D_invert(occ.int())], dim=0).contiguous()
            N = coords.shape[0]
        noise = torch.rand(N, 3, dtype=torch.float32, device=dev)
        xyzs = torch.empty(N, 3, dtype=torch.float32, device=dev)
        indices = torch.empty(N, dtype=torch.int32, device=dev)
        mean = torch.empty(1, dtype=torch.float32, device=dev)
        scratch = torch.empty(_lib.raw('mve_density_grid_scratch_bytes')(n_cells), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call('mve_density_grid_points', _lib.ptr(coords), _lib.ptr(noise), N, H, self.bound, _lib.ptr(xyzs),
                      _lib.ptr(indices), _lib.stream_ptr(dev))
            with torch.no_grad():
                sigmas, _ = dec.point_density_decode([xyzs], code)
            _lib.call('mve_density_grid_update', _lib.ptr(density_grid), _lib.ptr(tmp), n_cells, _lib.ptr(sigmas), _lib.ptr(indices),
                      N, float(decay), _lib.ptr(mean), _lib.ptr(scratch), _lib.stream_ptr(dev))
        thresh = min(float(mean.item()), density_thresh)              # the reference reads the mean on the host too (:171-174)
        rm.packbits(density_grid, thresh, density_bitfield)
        return iter_density + 1, thresh

    def forward(self, rays_o, rays_d, code, density_bitfield, grid_size, dt_gamma=0.0, perturb=False, noises=None, capacity=None,
                compute_normal=False):
        """rays_o, rays_d [N,3] (or [1,N,3]) of one scene, code [1, 3, C, h, w].  Returns the reference's result dict (weights, weights_sum,
        depth, image, rays, normal, ts; lists of one entry where the reference returns per-scene lists).  `noises` ([N], training) overrides
        the internally drawn perturbation."""
        from . import raymarching as rm
        if capacity is not None:
            raise NotImplementedError('capacity=: the host-read-free training form needs a counted tri-plane decode, which is not built')
        if compute_normal and self.training:
            raise NotImplementedError('compute_normal=True in training needs second-order grid_sample, which is not built')
        rays_o, rays_d, density_bitfield = self._one_scene(code, ('rays_o', rays_o, 2), ('rays_d', rays_d, 2), ('density_bitfield', density_bitfield, 1))
        if isinstance(grid_size, (list, tuple)):
            grid_size = self._one_scene(code, ('grid_size', grid_size, 0))[0]
        if isinstance(dt_gamma, (list, tuple)):
            dt_gamma = self._one_scene(code, ('dt_gamma', dt_gamma, 0))[0]
        dec = self.decoder
        if not self.training:
            ws, depth, image = dec.render_rays(rays_o, rays_d, code, density_bitfield, grid_size, float(dt_gamma))
            return dict(weights=None, weights_sum=[ws], depth=[depth], image=[image], rays=None, normal=[None], ts=None)
        nears, fars = rm.near_far_from_aabb(rays_o, rays_d, dec.aabb, self.min_near)
        xyzs, dirs, ts, rays = rm.march_rays_train(rays_o, rays_d, self.bound, density_bitfield, 1, grid_size, nears, fars,
                                                   perturb=perturb, dt_gamma=float(dt_gamma), max_steps=self.max_steps, noises=noises)
        if self.weight_culling_th > 0:
            with torch.no_grad():                                      # base_volume_renderer.py:223
                sigmas, _ = dec.point_density_decode([xyzs], code)
                weights, _, _, _ = rm.batch_composite_rays_train(sigmas, sigmas.new_zeros(sigmas.shape[0], 3), [ts], [rays], [ts.shape[0]])
                xyzs, dirs, ts, rays = rm.cull_samples(weights, self.weight_culling_th, xyzs, dirs, ts, rays)
        differentiable = torch.is_grad_enabled() and (code.requires_grad or any(t.requires_grad for t in dec.parameters().values()))
        if differentiable:
            sigmas, rgbs, _ = dec.point_decode_autograd([xyzs], [dirs], code)
        else:
            sigmas, rgbs, _ = dec.point_decode([xyzs], [dirs], code)
        weights, weights_sum, depth, image = rm.batch_composite_rays_train(sigmas, rgbs, [ts], [rays], [ts.shape[0]])
        return dict(weights=weights, weights_sum=weights_sum, depth=depth, image=image, rays=[rays], normal=None, ts=[ts])
