"""The sliver of `torch.nn.Module` the reference reads off the modules the drop-in replaces with engines (mvedit_amd.dropin.swap_engines):
`next(self.image_enhancer.parameters()).dtype` (lib/pipelines/mvedit_3d_pipeline.py:1017) and its like.  The engines' weights live in packed
native storage, so `parameters()` yields one empty tensor that carries the engine's dtype and device."""
import ctypes

import torch

from . import _lib
from .ops import dt as _dt


class ModuleSurface:
    """Mixin for engines with `self.dtype` and `self.device`."""

    def parameters(self, recurse=True):
        p = self.__dict__.get('_param_probe')
        if p is None or p.dtype != self.dtype or p.device != self.device:
            p = self.__dict__['_param_probe'] = torch.empty(0, dtype=self.dtype, device=self.device)
        yield p


class InferenceSurface(ModuleSurface):
    """The inference-only sliver of `torch.nn.Module` the reference's loaders call on what they build: `.eval()`, `.requires_grad_(False)`,
    `.to(device)` answer `self`; anything that would train or re-pack the engine is refused."""

    def eval(self):
        return self

    def requires_grad_(self, requires_grad=False):
        if requires_grad:
            raise NotImplementedError(f'{type(self).__name__}.requires_grad_(True): the engine is inference only')
        return self

    def to(self, *args, **kwargs):
        want_dev, want_dt = kwargs.get('device'), kwargs.get('dtype')
        for a in args:
            if isinstance(a, torch.dtype):
                want_dt = a
            elif a is not None:
                want_dev = a
        if want_dt is not None and want_dt != self.dtype:
            raise NotImplementedError(f'{type(self).__name__}.to(dtype={want_dt}): the engine is packed in {self.dtype}; build a new one')
        if want_dev is not None:
            d = torch.device(want_dev)
            same = d.type == self.device.type and (d.index is None or self.device.index is None or d.index == self.device.index)
            if not same:
                raise NotImplementedError(f'{type(self).__name__}.to(device={d}): the engine lives on {self.device}; build a new one')
        return self


class EngineHandle(InferenceSurface):
    """Base of the engines that own one native executor handle `self._h` (created by the subclass's constructor through its own mve_*_create):
    the handle's lifetime, pushing state-dict tensors into it, reading its plan back and the grow-only workspace."""

    OP_CLASSES = ('conv', 'linear', 'attention', 'norm', 'other')
    _h = None
    _ws = None

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            try:
                _lib.raw('mve_unet_destroy')(h)
            except Exception:
                pass
            self._h = None

    # ---- weights --------------------------------------------------------------------------------------------------------------------------------
    def _push_param(self, name, tensor, stream):
        """One state-dict tensor into its packed place (mve_unet_load_param; stream-ordered).  Returns the device tensor that was read: the
        caller keeps it alive until the stream is synchronised."""
        t = tensor.detach()
        if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            t = t.float()
        t = t.to(self.device).contiguous()
        shape = (ctypes.c_longlong * t.dim())(*t.shape)
        _lib.call('mve_unet_load_param', self._h, name.encode(), _lib.ptr(t), _dt(t), t.dim(), shape, stream)
        return t

    def _missing_params(self):
        """-> (number of expected parameters not loaded yet, the first one's name)"""
        buf = ctypes.create_string_buffer(256)
        return _lib.raw('mve_unet_missing_params')(self._h, buf, 256), buf.value.decode()

    # ---- the current plan -----------------------------------------------------------------------------------------------------------------------
    def _plan_result(self, ws, n_ops, flops):
        return dict(workspace_bytes=ws.value, n_ops=n_ops.value, flops=dict(zip(self.OP_CLASSES, list(flops))))

    def _op_rows(self):
        """(phase, class, flops, label) of every op of the currently cached plan"""
        info = _lib.raw('mve_unet_op_info')
        cls, fl, lab = ctypes.c_int(), ctypes.c_double(), ctypes.create_string_buffer(96)
        i = 0
        while True:
            ph = info(self._h, i, ctypes.byref(cls), ctypes.byref(fl), lab, 96)
            if ph < 0:
                return
            yield ph, self.OP_CLASSES[cls.value], fl.value, lab.value.decode()
            i += 1

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws
