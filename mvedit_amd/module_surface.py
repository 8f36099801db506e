"""The sliver of `torch.nn.Module` the reference reads off the modules the drop-in replaces with engines (mvedit_amd.dropin.swap_engines):
`next(self.image_enhancer.parameters()).dtype` (lib/pipelines/mvedit_3d_pipeline.py:1017) and its like.  The engines' weights live in packed
native storage, so `parameters()` yields one empty tensor that carries the engine's dtype and device."""
import torch


class ModuleSurface:
    """Mixin for engines with `self.dtype` and `self.device`."""

    def parameters(self, recurse=True):
        p = self.__dict__.get('_param_probe')
        if p is None or p.dtype != self.dtype or p.device != self.device:
            p = self.__dict__['_param_probe'] = torch.empty(0, dtype=self.dtype, device=self.device)
        yield p
