"""`nvdiffrast` for the reference on gfx950: the package whose `torch` submodule carries nvdiffrast's public names on native HIP kernels.
`mvedit_amd.dropin.install()` seeds it as `nvdiffrast`, so `import nvdiffrast.torch as dr` resolves to `mvedit_amd.nvdiffrast.torch`."""
from . import torch  # noqa: F401
