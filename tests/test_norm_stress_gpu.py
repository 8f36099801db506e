"""GroupNorm, LayerNorm and the row softmax on the activation statistics real checkpoints produce (tests/hard_stats.py), on every dispatch path.

VERDICT.md ("What's weak", item 1): "a real checkpoint (outlier channels) is untested by construction".  Every family of hard_stats.py x {fp16, bf16}
runs against a float64 reference of the same rounded input, the bar of test_unet_ops.py (TOL) applied per (image, group) for GroupNorm and per block
of 64 rows for LayerNorm.

How each GroupNorm path is selected (gnf_plan / gn_tx / gn_nsplit in csrc/norm.hip; G = 32):
  one-launch, 256 threads      HW * lcm(C / 32, 8) / 8 <= 5120 vectors: (3, 64, 320) groups of 10 channels straddle the 8-lane vectors;
                               (2, 1024, 320) 20 vectors per thread; (2, 64, 2560) groups of 80; (8, 64, 320) B % 8 == 0: the XCD block map
  one-launch, 1024 threads     (2, 400, 640 + 320): 960 channels, groups of 30, 120-channel chunks, 6000 vectors
  three launches, forced       mve_groupnorm_tune(0) at HW = 1100 (ragged against the rows of a split): C = 320 (40-lane blocks), 1024 (64),
                               768 (32), 640 + 320 (40, two sources).  Every one-launch case runs a second time like this as well, and the two
                               paths must agree within TOL
                               (2, 1100, 480): groups of 15 channels.  The statistics pass shifts its sums by one value per channel PAIR, which
                               an odd group size does not allow (a pair would straddle two groups): such tensors -- no engine has one -- keep the
                               plain sums, so this case runs without offset128 / offset256
  three launches, by plan      (1, 4096, 320): HW > 1024
  three launches, VAE form     eps 1e-6, with and without SiLU: (2, 1100, 128) 16-lane blocks (groups of 4: never fused), (2, 1100, 256) 32-lane,
                               (1, 2304, 512)
  stream pair                  mve_groupnorm_silu_pair: (3, 256, 640), (3, 64, 1280 + 1280) one launch (HW <= 256); (2, 1100, 320),
                               (2, 1024, 1280 + 640) three launches
LayerNorm: mve_layernorm at (70, 320), (33, 640), (9, 1280), (5, 2048) -- the four per_lane instantiations with their row tails --,
mve_layernorm_pair at (70, 320), the epilogue of the 320-wide GEMM tile through ops.gemm_ln at (512, 320, 320) with the fusion on and off.
Row softmax: N = 4, 1028, 4096, 5000 in buffers with lds = N + 4 and ldp = N + 8.

Worst max|err| / max|ref| and rel-L2 (the larger of the two) per (path, family, dtype), printed once per run (pytest -s):
  path                                           dtype       benign   offset8  offset32 offset128 offset256     split   outlier  constant      tiny
  gemm_ln epilogue (512,320,320)                 bfloat16   3.1e-03   3.2e-03   3.1e-03   3.2e-03   3.2e-03   3.8e-03   2.8e-03   3.1e-03   3.1e-03
  gemm_ln epilogue (512,320,320)                 float16    3.9e-04   3.8e-04   3.9e-04   3.9e-04   4.0e-04   4.8e-04   3.3e-04   3.7e-04   3.9e-04
  layernorm (33,640)                             bfloat16   2.3e-03   2.3e-03   2.3e-03         -         -   3.6e-03   2.2e-03   2.4e-03   2.4e-03
  layernorm (33,640)                             float16    3.4e-04   3.3e-04   3.1e-04   3.3e-04   3.0e-04   4.5e-04   2.7e-04   3.4e-04   3.4e-04
  layernorm (5,2048)                             bfloat16   2.6e-03   3.0e-03   3.0e-03         -         -   1.9e-03   1.9e-03   2.9e-03   2.9e-03
  layernorm (5,2048)                             float16    3.7e-04   2.8e-04   3.2e-04   3.7e-04   4.0e-04   2.4e-04   1.7e-04   2.6e-04   2.6e-04
  layernorm (70,320)                             bfloat16   3.3e-03   2.1e-03   3.1e-03         -         -   3.6e-03   2.4e-03   1.9e-03   1.9e-03
  layernorm (70,320)                             float16    4.3e-04   3.3e-04   3.0e-04   4.4e-04   3.0e-04   4.6e-04   3.0e-04   3.2e-04   3.2e-04
  layernorm (9,1280)                             bfloat16   2.6e-03   3.2e-03   2.4e-03         -         -   2.6e-03   2.9e-03   2.3e-03   2.3e-03
  layernorm (9,1280)                             float16    3.6e-04   3.6e-04   4.0e-04   3.2e-04   3.9e-04   4.7e-04   3.3e-04   3.4e-04   3.4e-04
  layernorm pair (70,320)                        bfloat16   3.4e-03   3.2e-03   3.0e-03   3.1e-03   3.0e-03   3.5e-03   2.4e-03   3.8e-03   3.8e-03
  layernorm pair (70,320)                        float16    3.2e-04   3.4e-04   3.6e-04   4.0e-04   4.0e-04   4.8e-04   3.3e-04   2.9e-04   2.9e-04
  one launch 1024t cpg30 (2,400,640+320)         bfloat16   3.3e-03   3.6e-03   3.5e-03         -         -   3.7e-03   3.5e-03   3.2e-03   3.2e-03
  one launch 1024t cpg30 (2,400,640+320)         float16    4.5e-04   4.4e-04   4.5e-04   4.5e-04   4.7e-04   4.6e-04   4.1e-04   4.5e-04   4.5e-04
  one launch 256t 20 vec (2,1024,320)            bfloat16   3.8e-03   3.8e-03   3.8e-03         -         -   3.8e-03   3.5e-03   3.6e-03   3.6e-03
  one launch 256t 20 vec (2,1024,320)            float16    4.5e-04   4.2e-04   4.4e-04   4.5e-04   4.5e-04   4.6e-04   4.5e-04   4.6e-04   4.6e-04
  one launch 256t cpg10 (3,64,320)               bfloat16   3.2e-03   3.2e-03   3.8e-03         -         -   3.6e-03   3.6e-03   3.2e-03   3.2e-03
  one launch 256t cpg10 (3,64,320)               float16    4.1e-04   4.3e-04   3.7e-04   4.6e-04   3.9e-04   4.8e-04   4.6e-04   4.0e-04   4.0e-04
  one launch 256t cpg80 (2,64,2560)              bfloat16   3.5e-03   3.7e-03   3.5e-03         -         -   3.4e-03   3.4e-03   3.6e-03   3.6e-03
  one launch 256t cpg80 (2,64,2560)              float16    4.5e-04   4.6e-04   4.3e-04   4.4e-04   4.4e-04   4.5e-04   4.6e-04   4.6e-04   4.6e-04
  one launch 256t xcd map (8,64,320)             bfloat16   3.4e-03   3.6e-03   3.4e-03         -         -   3.7e-03   3.8e-03   3.5e-03   3.5e-03
  one launch 256t xcd map (8,64,320)             float16    4.2e-04   4.8e-04   4.8e-04   4.6e-04   4.6e-04   4.7e-04   4.4e-04   3.9e-04   3.9e-04
  pair one launch (3,256,640)                    bfloat16   3.5e-03   3.5e-03   3.5e-03   3.7e-03   3.4e-03   3.8e-03   3.6e-03   3.5e-03   3.5e-03
  pair one launch (3,256,640)                    float16    4.8e-04   4.7e-04   4.7e-04   4.5e-04   4.6e-04   4.8e-04   4.3e-04   4.8e-04   4.8e-04
  pair one launch (3,64,1280+1280)               bfloat16   3.7e-03   3.7e-03   3.8e-03   3.6e-03   3.7e-03   3.5e-03   3.7e-03   3.7e-03   3.7e-03
  pair one launch (3,64,1280+1280)               float16    4.5e-04   4.4e-04   4.6e-04   4.6e-04   4.8e-04   4.4e-04   4.6e-04   4.5e-04   4.5e-04
  pair three (2,1024,1280+640)                   bfloat16   3.3e-03   3.4e-03   3.3e-03   3.3e-03   3.5e-03   3.7e-03   3.6e-03   3.4e-03   3.4e-03
  pair three (2,1024,1280+640)                   float16    4.5e-04   4.4e-04   4.3e-04   4.4e-04   4.4e-04   4.6e-04   4.5e-04   4.5e-04   4.5e-04
  pair three (2,1100,320)                        bfloat16   3.5e-03   3.6e-03   3.6e-03   3.4e-03   3.5e-03   3.8e-03   3.2e-03   3.5e-03   3.5e-03
  pair three (2,1100,320)                        float16    4.6e-04   4.7e-04   4.5e-04   4.3e-04   4.3e-04   4.8e-04   4.2e-04   4.6e-04   4.6e-04
  three by plan (1,4096,320)                     bfloat16   3.2e-03   3.2e-03   3.3e-03         -         -   3.6e-03   3.1e-03   3.3e-03   3.3e-03
  three by plan (1,4096,320)                     float16    4.5e-04   4.4e-04   4.4e-04   4.2e-04   4.3e-04   4.7e-04   4.3e-04   4.4e-04   4.4e-04
  three forced at 1024t cpg30 (2,400,640+320)    bfloat16   3.3e-03   3.6e-03   3.5e-03         -         -   3.7e-03   3.5e-03   3.2e-03   3.2e-03
  three forced at 1024t cpg30 (2,400,640+320)    float16    4.5e-04   4.4e-04   4.5e-04   4.5e-04   4.6e-04   4.6e-04   4.1e-04   4.5e-04   4.5e-04
  three forced at 256t 20 vec (2,1024,320)       bfloat16   3.8e-03   3.8e-03   3.8e-03         -         -   3.8e-03   3.5e-03   3.6e-03   3.6e-03
  three forced at 256t 20 vec (2,1024,320)       float16    4.5e-04   4.2e-04   4.4e-04   4.5e-04   4.5e-04   4.6e-04   4.5e-04   4.6e-04   4.6e-04
  three forced at 256t cpg10 (3,64,320)          bfloat16   3.2e-03   3.2e-03   3.8e-03         -         -   3.6e-03   3.6e-03   3.2e-03   3.2e-03
  three forced at 256t cpg10 (3,64,320)          float16    4.1e-04   4.3e-04   3.7e-04   4.6e-04   3.9e-04   4.8e-04   4.6e-04   4.0e-04   4.0e-04
  three forced at 256t cpg80 (2,64,2560)         bfloat16   3.5e-03   3.7e-03   3.5e-03         -         -   3.4e-03   3.4e-03   3.6e-03   3.6e-03
  three forced at 256t cpg80 (2,64,2560)         float16    4.5e-04   4.6e-04   4.3e-04   4.4e-04   4.4e-04   4.5e-04   4.6e-04   4.6e-04   4.6e-04
  three forced at 256t xcd map (8,64,320)        bfloat16   3.4e-03   3.6e-03   3.4e-03         -         -   3.7e-03   3.8e-03   3.5e-03   3.5e-03
  three forced at 256t xcd map (8,64,320)        float16    4.2e-04   4.8e-04   4.8e-04   4.6e-04   4.6e-04   4.7e-04   4.4e-04   3.9e-04   3.9e-04
  three forced tx32 (2,1100,768)                 bfloat16   3.6e-03   3.6e-03   3.4e-03         -         -   3.4e-03   3.5e-03   3.7e-03   3.7e-03
  three forced tx32 (2,1100,768)                 float16    4.4e-04   4.3e-04   4.7e-04   4.5e-04   4.3e-04   4.6e-04   4.4e-04   4.8e-04   4.8e-04
  three forced tx40 (2,1100,320)                 bfloat16   3.4e-03   3.4e-03   3.6e-03         -         -   3.8e-03   3.3e-03   3.5e-03   3.5e-03
  three forced tx40 (2,1100,320)                 float16    4.8e-04   4.8e-04   4.4e-04   4.7e-04   4.5e-04   4.7e-04   4.4e-04   4.8e-04   4.8e-04
  three forced tx40 2src (2,1100,640+320)        bfloat16   3.5e-03   3.5e-03   3.6e-03         -         -   3.6e-03   3.5e-03   3.5e-03   3.5e-03
  three forced tx40 2src (2,1100,640+320)        float16    4.7e-04   4.4e-04   4.2e-04   4.1e-04   4.6e-04   4.5e-04   4.6e-04   4.6e-04   4.6e-04
  three forced tx64 (2,1100,1024)                bfloat16   3.4e-03   3.8e-03   3.4e-03         -         -   3.7e-03   3.5e-03   3.4e-03   3.4e-03
  three forced tx64 (2,1100,1024)                float16    4.4e-04   4.4e-04   4.5e-04   4.7e-04   4.4e-04   4.7e-04   4.3e-04   4.3e-04   4.3e-04
  three forced tx64 cpg15 (2,1100,480)           bfloat16   3.6e-03   3.6e-03   3.7e-03         -         -   3.7e-03   3.3e-03   3.4e-03   3.4e-03
  three forced tx64 cpg15 (2,1100,480)           float16    4.6e-04   4.5e-04   4.9e-04         -         -   4.7e-04   4.1e-04   4.7e-04   4.7e-04
  three vae tx16 (2,1100,128)                    bfloat16   3.6e-03   3.7e-03   3.5e-03         -         -   3.6e-03   3.3e-03   3.5e-03   3.5e-03
  three vae tx16 (2,1100,128)                    float16    4.6e-04   4.6e-04   4.6e-04   4.4e-04   4.4e-04   4.8e-04   4.2e-04   4.5e-04   4.5e-04
  three vae tx16 silu (2,1100,128)               bfloat16   3.6e-03   3.8e-03   3.3e-03         -         -   3.7e-03   3.2e-03   3.6e-03   3.6e-03
  three vae tx16 silu (2,1100,128)               float16    4.3e-04   4.6e-04   4.4e-04   4.5e-04   4.4e-04   4.7e-04   4.2e-04   4.4e-04   4.4e-04
  three vae tx32 (2,1100,256)                    bfloat16   3.8e-03   3.6e-03   3.4e-03         -         -   3.7e-03   3.7e-03   3.6e-03   3.6e-03
  three vae tx32 (2,1100,256)                    float16    4.5e-04   4.3e-04   4.5e-04   4.6e-04   4.3e-04   4.6e-04   4.5e-04   4.7e-04   4.7e-04
  three vae tx32 silu (2,1100,256)               bfloat16   3.6e-03   3.6e-03   3.4e-03         -         -   3.7e-03   3.5e-03   3.8e-03   3.8e-03
  three vae tx32 silu (2,1100,256)               float16    4.5e-04   4.5e-04   4.8e-04   4.6e-04   4.5e-04   4.7e-04   4.5e-04   4.3e-04   4.3e-04
  three vae tx64 (1,2304,512)                    bfloat16   3.2e-03   3.5e-03   3.5e-03         -         -   3.4e-03   3.1e-03   3.1e-03   3.1e-03
  three vae tx64 (1,2304,512)                    float16    4.2e-04   4.1e-04   4.3e-04   3.9e-04   4.4e-04   4.7e-04   3.6e-04   4.2e-04   4.2e-04
  three vae tx64 silu (1,2304,512)               bfloat16   3.7e-03   3.5e-03   3.3e-03         -         -   3.4e-03   3.3e-03   3.6e-03   3.6e-03
  three vae tx64 silu (1,2304,512)               float16    4.6e-04   4.5e-04   4.4e-04   4.6e-04   4.1e-04   4.6e-04   4.4e-04   4.6e-04   4.6e-04
  
  path                                           dtype    wide+clust      wide all equal  max last near -1e4     randn
  softmax N=1028                                 bfloat16   1.4e-03   5.3e-27   1.5e-05   2.1e-09   1.2e-03   2.3e-03
  softmax N=1028                                 float16    4.5e-04   4.8e-24   1.5e-05   2.3e-09   1.2e-04   1.5e-04
  softmax N=4                                    bfloat16   1.8e-03   0.0e+00   0.0e+00   2.5e-13   1.7e-03   4.0e-04
  softmax N=4                                    float16    4.1e-04   0.0e+00   0.0e+00   3.6e-13   1.8e-04   8.5e-05
  softmax N=4096                                 bfloat16   1.4e-03   9.2e-04   0.0e+00   4.2e-08   1.3e-03   7.4e-04
  softmax N=4096                                 float16    4.5e-04   8.6e-05   0.0e+00   5.1e-08   1.9e-04   2.5e-04
  softmax N=5000                                 bfloat16   2.2e-03   3.3e-04   1.4e-03   2.0e-08   4.7e-04   2.8e-03
  softmax N=5000                                 float16    3.5e-04   1.6e-04   1.7e-04   2.2e-08   2.5e-04   3.7e-04
"""
import pytest
import torch

import hard_stats as H
from test_unet_ops import TOL, rnd, _pair_tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DEV = 'cuda'
WORST = H.Worst()
SOFTMAX_ROWS = ('wide+clust', 'wide', 'all equal', 'max last', 'near -1e4', 'randn')


@pytest.fixture(scope='module', autouse=True)
def _print_worst():
    yield
    if WORST.t:
        print('\nworst ratio per (path, family, dtype):\n' + WORST.table() + '\n' + WORST.table(SOFTMAX_ROWS))


def _affine(C, seed=3):
    return (1 + 0.2 * rnd((C,), torch.float32, seed)).to(DEV), (0.2 * rnd((C,), torch.float32, seed + 1)).to(DEV)


def _gn_tune(_lib, word):
    return _lib.raw('mve_groupnorm_tune')(word)


def _gn(x1, x2, B, HW, G, gamma, beta, eps, silu, lo1=None, lo2=None):
    """mve_groupnorm_silu_pair (== mve_groupnorm_silu without low halves)"""
    from mvedit_amd import _lib
    from mvedit_amd.ops import dt
    C1, C2 = x1.shape[1], (x2.shape[1] if x2 is not None else 0)
    out = torch.empty(B * HW, C1 + C2, dtype=x1.dtype, device=x1.device)
    ws = torch.empty(_lib.raw('mve_groupnorm_workspace_bytes')(B, HW, C1 + C2, G), dtype=torch.uint8, device=x1.device)
    _lib.call('mve_groupnorm_silu_pair', dt(x1), _lib.ptr(x1), C1, _lib.ptr(x2), C2, B, HW, G, float(eps), _lib.ptr(gamma), _lib.ptr(beta), int(silu),
              _lib.ptr(out), _lib.ptr(ws), _lib.ptr(lo1), _lib.ptr(lo2), _lib.stream_ptr(x1.device))
    return out


def _raise_all(failures):
    if failures:
        raise AssertionError(f'{len(failures)} failure(s):\n' + '\n'.join(failures))


# (path, B, HW, C1, C2, eps, silu, forced three launches)
ONE = 'one launch'
ODD = 'three forced tx64 cpg15 (2,1100,480)'
GN_CASES = [
    (f'{ONE} 256t cpg10 (3,64,320)', 3, 64, 320, 0, 1e-5, True, False),
    (f'{ONE} 256t 20 vec (2,1024,320)', 2, 1024, 320, 0, 1e-5, True, False),
    (f'{ONE} 256t cpg80 (2,64,2560)', 2, 64, 2560, 0, 1e-5, True, False),
    (f'{ONE} 256t xcd map (8,64,320)', 8, 64, 320, 0, 1e-5, True, False),
    (f'{ONE} 1024t cpg30 (2,400,640+320)', 2, 400, 640, 320, 1e-5, True, False),
    ('three forced tx40 (2,1100,320)', 2, 1100, 320, 0, 1e-5, True, True),
    ('three forced tx64 (2,1100,1024)', 2, 1100, 1024, 0, 1e-5, True, True),
    ('three forced tx32 (2,1100,768)', 2, 1100, 768, 0, 1e-5, True, True),
    ('three forced tx40 2src (2,1100,640+320)', 2, 1100, 640, 320, 1e-5, True, True),
    (ODD, 2, 1100, 480, 0, 1e-5, True, True),
    ('three by plan (1,4096,320)', 1, 4096, 320, 0, 1e-5, True, False),
    ('three vae tx16 silu (2,1100,128)', 2, 1100, 128, 0, 1e-6, True, False),
    ('three vae tx16 (2,1100,128)', 2, 1100, 128, 0, 1e-6, False, False),
    ('three vae tx32 silu (2,1100,256)', 2, 1100, 256, 0, 1e-6, True, False),
    ('three vae tx32 (2,1100,256)', 2, 1100, 256, 0, 1e-6, False, False),
    ('three vae tx64 silu (1,2304,512)', 1, 2304, 512, 0, 1e-6, True, False),
    ('three vae tx64 (1,2304,512)', 1, 2304, 512, 0, 1e-6, False, False),
]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', GN_CASES, ids=[c[0] for c in GN_CASES])
def test_groupnorm_families(lib, dtype, case):
    path, B, HW, C1, C2, eps, silu, forced = case
    C, G = C1 + C2, 32
    gamma, beta = _affine(C)
    one_launch = path.startswith(ONE)
    failures = []
    for fam in (f for f in H.families(dtype) if not (path == ODD and f in ('offset128', 'offset256'))):
        x = H.make(fam, B * HW, C, G, dtype, 1, DEV)
        ref = H.groupnorm_ref(x, B, HW, G, gamma, beta, eps, silu)
        x16 = x.to(dtype)
        x1, x2 = x16[:, :C1].contiguous(), (x16[:, C1:].contiguous() if C2 else None)
        prev = _gn_tune(lib, 0 if forced else -1)
        try:
            out = _gn(x1, x2, B, HW, G, gamma, beta, eps, silu)
            if one_launch:
                _gn_tune(lib, 0)
                three = _gn(x1, x2, B, HW, G, gamma, beta, eps, silu)
        finally:
            _gn_tune(lib, prev)
        try:
            WORST.add(path, fam, dtype, H.check_groups(path, fam, out, ref, B, HW, G, dtype))
        except AssertionError as e:
            failures.append(str(e))
        if one_launch:
            p3 = path.replace(ONE, 'three forced at')
            try:
                WORST.add(p3, fam, dtype, H.check_groups(p3, fam, three, ref, B, HW, G, dtype))
                H.check_groups(path + ' against the three launches', fam, out, three, B, HW, G, dtype, scale_ref=ref)
            except AssertionError as e:
                failures.append(str(e))
    _raise_all(failures)


PAIR_CASES = [('pair one launch (3,256,640)', 3, 256, 640, 0), ('pair one launch (3,64,1280+1280)', 3, 64, 1280, 1280),
              ('pair three (2,1100,320)', 2, 1100, 320, 0), ('pair three (2,1024,1280+640)', 2, 1024, 1280, 640)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_groupnorm_pair_families(lib, dtype, case):
    """mve_groupnorm_silu_pair: the input is the unrounded family split into (hi, lo8); the reference is float64 on hi + lo"""
    from mvedit_amd import ops
    path, B, HW, C1, C2 = case
    C, G, eps = C1 + C2, 32, 1e-5
    gamma, beta = _affine(C)
    failures = []
    for fam in H.families(dtype, pair=True):
        x = H.make(fam, B * HW, C, G, None, 2, DEV)
        h1, l1 = ops.split_pair(x[:, :C1].contiguous(), dtype)
        h2, l2 = ops.split_pair(x[:, C1:].contiguous(), dtype) if C2 else (None, None)
        val = torch.cat([h1.double() + ops.lo8_to_float(l1).double()] + ([h2.double() + ops.lo8_to_float(l2).double()] if C2 else []), 1)
        ref = H.groupnorm_ref(val, B, HW, G, gamma, beta, eps, True)
        out = _gn(h1, h2, B, HW, G, gamma, beta, eps, True, l1, l2)
        try:
            WORST.add(path, fam, dtype, H.check_groups(path, fam, out, ref, B, HW, G, dtype))
        except AssertionError as e:
            failures.append(str(e))
    _raise_all(failures)


@pytest.mark.parametrize('HW,C1,C2,word,pair', [(256, 640, 0, -1, False), (1100, 320, 0, 0, False), (1100, 640, 320, 0, False),
                                                (256, 640, 0, -1, True), (1100, 320, 0, -1, True)])
def test_groupnorm_batch_invariance_on_offset128(lib, HW, C1, C2, word, pair):
    """test_groupnorm_batch_invariance_and_paths' claim on a group mean of 128 standard deviations: an image alone equals the same image inside a
    batch, bitwise, on the one-launch kernel and on the three launches, plain and as a stream pair"""
    from mvedit_amd import ops
    dtype, B, G = torch.float16, 3, 32
    C = C1 + C2
    gamma, beta = _affine(C)
    x = H.make('offset128', B * HW, C, G, None if pair else dtype, 3, DEV)
    h1, l1 = ops.split_pair(x[:, :C1].contiguous(), dtype)
    h2, l2 = ops.split_pair(x[:, C1:].contiguous(), dtype) if C2 else (None, None)
    if not pair:
        l1 = l2 = None
    prev = _gn_tune(lib, word)
    try:
        full = _gn(h1, h2, B, HW, G, gamma, beta, 1e-5, True, l1, l2)
        for b in range(B):
            sl = slice(b * HW, (b + 1) * HW)
            c = lambda t: None if t is None else t[sl].contiguous()
            one = _gn(c(h1), c(h2), 1, HW, G, gamma, beta, 1e-5, True, c(l1), c(l2))
            assert torch.equal(one, full[sl]), f'image {b} alone differs from image {b} of the {B}-image launch'
    finally:
        _gn_tune(lib, prev)


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('M,C', [(70, 320), (33, 640), (9, 1280), (5, 2048)])
def test_layernorm_families(lib, dtype, M, C):
    from mvedit_amd import ops
    gamma, beta = _affine(C)
    path, failures = f'layernorm ({M},{C})', []
    for fam in H.families(dtype):
        x = H.make_rows(fam, M, C, dtype, 4, DEV)
        out = ops.layernorm(x.to(dtype), gamma, beta)
        try:
            WORST.add(path, fam, dtype, H.check_rows(path, fam, out, H.layernorm_ref(x, gamma, beta, 1e-5), dtype))
        except AssertionError as e:
            failures.append(str(e))
    _raise_all(failures)


@pytest.mark.parametrize('dtype', DTYPES)
def test_layernorm_pair_families(lib, dtype):
    from mvedit_amd import ops, _lib
    M, C = 70, 320
    gamma, beta = _affine(C)
    path, failures = f'layernorm pair ({M},{C})', []
    for fam in H.families(dtype, pair=True):
        hi, lo = ops.split_pair(H.make_rows(fam, M, C, None, 5, DEV), dtype)
        out = torch.empty(M, C, dtype=dtype, device=DEV)
        _lib.call('mve_layernorm_pair', ops.dt(hi), _lib.ptr(hi), C, _lib.ptr(out), C, M, C, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, _lib.ptr(lo),
                  _lib.stream_ptr(hi.device))
        ref = H.layernorm_ref(hi.double() + ops.lo8_to_float(lo).double(), gamma, beta, 1e-5)
        try:
            WORST.add(path, fam, dtype, H.check_rows(path, fam, out, ref, dtype))
        except AssertionError as e:
            failures.append(str(e))
    _raise_all(failures)


@pytest.mark.parametrize('dtype', DTYPES)
def test_gemm_layernorm_epilogue_families(lib, dtype):
    """ops.gemm_ln at (512, 320, 320): the residual pair carries the family, the GEMM term is small.  The LayerNorm reads the row as a consumer reads
    it back, so its reference is float64 LayerNorm of the launch's own output pair hi + lo; the pair itself stays within the pair format's error of
    the float64 sum: that second assertion is what sees an error of the residual add -- the LayerNorm check alone, fed the launch's own pair, would
    not.  Fusion on and off give the same bits (as test_gemm_ln.py requires)."""
    from mvedit_amd import ops, _lib
    fuse = _lib.raw('mve_gemm_ln_fuse_tune')
    M, N, K = 512, 320, 320
    a, w = rnd((M, K), dtype, 1).to(DEV), rnd((N, K), dtype, 2, 0.05 * K ** -0.5).to(DEV)
    bias = rnd((N,), torch.float32, 3, 0.05).to(DEV)
    gamma, beta = _affine(N)
    failures = []
    for fam in H.families(dtype, pair=True):
        rh, rl = ops.split_pair(H.make_rows(fam, M, N, None, 6, DEV), dtype)
        old = fuse(-1)
        try:
            fuse(1)
            (hi1, lo1), ln1 = ops.gemm_ln(a, w, bias, gamma, beta, residual=rh, residual_lo=rl)
            fuse(0)
            (hi0, lo0), ln0 = ops.gemm_ln(a, w, bias, gamma, beta, residual=rh, residual_lo=rl)
        finally:
            fuse(old)
        try:
            assert torch.equal(hi1, hi0) and torch.equal(lo1, lo0) and torch.equal(ln1, ln0), f'gemm_ln / {fam}: fusion on and off differ'
            val = hi1.double() + ops.lo8_to_float(lo1).double()
            x64 = a.double() @ w.double().t() + bias.double() + rh.double() + ops.lo8_to_float(rl).double()
            e = float((val - x64).abs().max() / x64.abs().max())
            assert e < _pair_tol(dtype), f'gemm_ln / {fam}: |hi + lo - float64| / max = {e:.2e}'
            WORST.add('gemm_ln epilogue (512,320,320)', fam, dtype,
                      H.check_rows('gemm_ln epilogue', fam, ln1, H.layernorm_ref(val, gamma, beta, 1e-5), dtype))
        except AssertionError as e:
            failures.append(str(e))
    _raise_all(failures)


# ---- row softmax ------------------------------------------------------------------------------------------------------------------------------------
def _softmax_rows(N):
    """fp32 logits [7, N]: wide (+-3e4, with a cluster of near-maximal ones), all equal, maximum in the last element, all near -1e4 (nothing survives
    unless the maximum is subtracted), and the suite's benign rows as the anchor"""
    g = torch.Generator().manual_seed(N)
    s = torch.randn(7, N, generator=g) * 6
    s[0] = (torch.rand(N, generator=g) * 2 - 1) * 3e4
    s[0, :: max(1, N // 5)] = 3e4 - torch.arange(len(s[0, :: max(1, N // 5)])).float() * 0.7
    s[1] = (torch.rand(N, generator=g) * 2 - 1) * 3e4
    s[2] = 7.5
    s[3, N - 1] = 40.0
    s[4] = -1e4 + torch.randn(N, generator=g) * 2
    return s


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N', [4, 1028, 4096, 5000])
def test_softmax_rows_hard_logits(lib, dtype, N):
    from mvedit_amd import _lib, ops
    s = _softmax_rows(N)
    M, lds, ldp = s.shape[0], N + 4, N + 8
    S = torch.full((M, lds), 1e30, device=DEV)              # padding that would win every maximum if it were read
    S[:, :N] = s.to(DEV)
    P = torch.full((M, ldp), 7.0, dtype=dtype, device=DEV)
    _lib.call('mve_softmax_rows', ops.dt(dtype), _lib.ptr(S), lds, M, N, _lib.ptr(P), ldp, _lib.stream_ptr(S.device))
    assert bool((P[:, N:] == 7.0).all()), 'the kernel wrote outside its columns'
    got, ref = P[:, :N].double().cpu(), H.softmax_ref(s)
    names = SOFTMAX_ROWS + ('randn',) * 2
    failures = []
    for r in range(M):
        try:
            WORST.add(f'softmax N={N}', names[r], dtype, H.check_rows(f'softmax N={N}', names[r], got[r:r + 1], ref[r:r + 1], dtype))
            rs = float(got[r].sum())
            assert abs(rs - 1) <= TOL[dtype], f'softmax N={N} / {names[r]} / {dtype}: the row sums to {rs:.6f}'
        except AssertionError as e:
            failures.append(str(e))
    _raise_all(failures)
