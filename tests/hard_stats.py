"""Activation statistics that real checkpoints produce and `randn` does not, float64 references of the reduction ops, and the per-group check.

Shared by test_norm_stress_gpu.py, test_attention_paths_gpu.py and the LayerNorm cases of test_loftr_kernels_gpu.py / test_sam_decoder_kernels_gpu.py.

Input families.  `make(family, rows, C, G, dtype, seed)` returns an fp32 tensor [rows, C] already rounded to `dtype` (dtype None: left unrounded,
to be split with ops.split_pair).  A "group" is the reduction unit: channels [g C/G, (g + 1) C/G) of every row for GroupNorm; for LayerNorm the
row is the unit (`make_rows`).
  benign       randn + 0.5: what the suite used before, the anchor
  offset<R>    every group has std 0.5 and mean +-R 0.5, the sign alternating by group (R = 8, 32, 128, 256: |mean| / std of the group)
  split        half the channels of a group sit at +40, the other half at -40, std 0.5: the channels do not share a mean, the group does
  outlier      one channel per group is 40 x wider than the rest
  constant     in every fourth group all elements are equal (3.0 in groups 0, 8, ..., the 16-bit value nearest 0.1 in groups 4, 12, ...); the rest randn
  tiny         in every fourth group std = 2^-10 around 0, so that eps decides; the rest randn

The bar is the one tests/test_unet_ops.py states once (TOL: 1e-3 fp16, 8e-3 bf16: the output rounding alone costs 4.9e-4 / 3.9e-3 of a value) on
max|got - ref| / max|ref| and on the relative L2 error -- here per (image, group) for GroupNorm and per block of 64 rows for LayerNorm, so that one bad
group cannot hide behind 31 good ones.  In the `constant` and `tiny` families the special groups' reference is (nearly) act(beta): there the kernel and
torch alike amplify a last-bit error of the mean by 1 / sqrt(eps), and those groups are normalised by the tensor-wide max|ref| (rms ref) instead."""
import functools

import torch

OFFSETS = (8, 32, 128, 256)
FAMILIES = ('benign',) + tuple(f'offset{r}' for r in OFFSETS) + ('split', 'outlier', 'constant', 'tiny')
SPECIAL_EVERY = 4            # constant / tiny: groups g % 4 == 0


def families(dtype, pair=False):
    """The families a dtype can carry: bf16 has 8 significant bits, so a plain bf16 tensor holds std-0.5 data around R 0.5 only up to R = 32
    (at R = 128 a std is half a rounding step).  A stream pair (hi + lo8) carries 3 more bits and takes every R."""
    if dtype == torch.bfloat16 and not pair:
        return tuple(f for f in FAMILIES if f not in ('offset128', 'offset256'))
    return FAMILIES


@functools.lru_cache(maxsize=4)
def _noise(U, rows, n, seed, device):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(U, rows, n, generator=g).to(device)


def _units(family, U, rows, n, dtype, seed, device):
    """[U, rows, n] fp32: U reduction units of rows x n elements ("n channels"), unit u following `family`."""
    z = _noise(U, rows, n, seed, str(device))
    u = torch.arange(U, device=z.device)
    if family == 'benign':
        x = z + 0.5
    elif family.startswith('offset'):
        R = float(family[6:])
        sign = (1.0 - 2.0 * (u % 2)).float()[:, None, None]
        x = 0.5 * z + sign * (R * 0.5)
    elif family == 'split':
        half = torch.where(torch.arange(n, device=z.device) < (n + 1) // 2, 40.0, -40.0)
        x = 0.5 * z + half[None, None, :]
    elif family == 'outlier':
        x = z.clone()
        x[u, :, (3 * u + 1) % n] *= 40.0
    elif family in ('constant', 'tiny'):
        x = z.clone()
        sp = u[u % SPECIAL_EVERY == 0]
        if family == 'tiny':
            x[sp] = z[sp] * 2.0 ** -10
        else:
            tenth = float(torch.tensor(0.1).to(dtype or torch.float32))
            x[sp] = torch.where(sp % (2 * SPECIAL_EVERY) == 0, 3.0, tenth).float()[:, None, None]
    else:
        raise ValueError(family)
    return x if dtype is None else x.to(dtype).float()


def make(family, rows, C, G, dtype, seed, device='cpu'):
    """GroupNorm input [rows, C] (rows = B HW): group g is channels [g C/G, (g + 1) C/G) of every row."""
    x = _units(family, G, rows, C // G, dtype, seed, device)
    return x.permute(1, 0, 2).reshape(rows, C).contiguous()


def make_rows(family, M, C, dtype, seed, device='cpu'):
    """LayerNorm input [M, C]: the row is the group."""
    return _units(family, M, 1, C, dtype, seed, device).reshape(M, C).contiguous()


def special_groups(family, G):
    """mask [G] of the groups normalised by the tensor-wide max|ref| (see the module docstring)"""
    m = torch.zeros(G, dtype=torch.bool)
    if family in ('constant', 'tiny'):
        m[::SPECIAL_EVERY] = True
    return m


# ---- float64 references ----------------------------------------------------------------------------------------------------------------------------
def groupnorm_ref(x, B, HW, G, gamma, beta, eps, silu):
    """x [B HW, C] (any float dtype) -> float64 GroupNorm(+SiLU), biased variance over (HW, C / G), eps inside the sqrt"""
    C = x.shape[1]
    x = x.double().reshape(B, HW, G, C // G)
    m = x.mean(dim=(1, 3), keepdim=True)
    v = ((x - m) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((x - m) / torch.sqrt(v + eps)).reshape(B, HW, C) * gamma.double().to(x.device) + beta.double().to(x.device)
    if silu:
        y = y / (1 + torch.exp(-y))
    return y.reshape(B * HW, C)


def layernorm_ref(x, gamma, beta, eps):
    x = x.double()
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * gamma.double().to(x.device) + beta.double().to(x.device)


def softmax_ref(s):
    s = s.double()
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def attention_ref(q, k, v, B, Lq, Lk, heads, d, scale=None):
    """float64 softmax attention; q [B Lq, heads d], k / v [B Lk, heads d] -> [B Lq, heads d]"""
    q = q.double().reshape(B, Lq, heads, d).transpose(1, 2)
    k = k.double().reshape(B, Lk, heads, d).transpose(1, 2)
    v = v.double().reshape(B, Lk, heads, d).transpose(1, 2)
    p = softmax_ref(q @ k.transpose(-1, -2) * (d ** -0.5 if scale is None else scale))
    return (p @ v).transpose(1, 2).reshape(B * Lq, heads * d)


# ---- the check -------------------------------------------------------------------------------------------------------------------------------------
def _tol(dtype):
    from test_unet_ops import TOL
    return TOL[dtype]


def _worst(name, emax, rmax, el2, rl2, tol, where):
    """emax / rmax / el2 / rl2: per-unit max error, max reference, rms error, rms reference (1-D, same length).  -> (worst max ratio, worst L2 ratio)"""
    r_max, r_l2 = emax / rmax.clamp_min(1e-30), el2 / rl2.clamp_min(1e-30)
    w_max, w_l2 = float(r_max.max()), float(r_l2.max())
    if not (w_max <= tol and w_l2 <= tol):        # (a NaN fails too)
        bad = r_max if not w_max <= tol else r_l2
        i = int(torch.nan_to_num(bad, nan=float('inf')).argmax())
        raise AssertionError(f'{name}: {where(i)}: max|err| / max|ref| = {float(r_max[i]):.3e}, rel-L2 = {float(r_l2[i]):.3e}, bar {tol:.0e}; '
                             f'{int(((r_max > tol) | (r_l2 > tol) | (r_max != r_max)).sum())} of {r_max.numel()} units over the bar')
    return w_max, w_l2


def check_groups(path, family, got, ref, B, HW, G, dtype, scale_ref=None):
    """GroupNorm outputs [B HW, C] per (image, group).  `scale_ref`: the tensor whose magnitudes normalise the error (default `ref`; the float64
    reference when two kernel paths are compared with each other).  -> (worst max ratio, worst rel-L2)"""
    C = ref.shape[1]
    got, ref = got.double().to(ref.device), ref.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f'{path} / {family}: shape or non-finite output'
    sref = ref if scale_ref is None else scale_ref.double()
    per = lambda t: t.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B * G, -1)
    err, s = per((got - ref).abs()), per(sref.abs())
    emax, rmax = err.max(1).values, s.max(1).values
    el2, rl2 = (err ** 2).mean(1).sqrt(), (s ** 2).mean(1).sqrt()
    sp = special_groups(family, G).to(ref.device).repeat(B)
    rmax = torch.where(sp, sref.abs().max(), rmax)
    rl2 = torch.where(sp, (sref ** 2).mean().sqrt(), rl2)

    def where(i):
        b, g = divmod(i, G)
        e = (got - ref).abs().reshape(B, HW, G, C // G)[b, :, g]
        r, c = divmod(int(e.argmax()), C // G)
        row, col = b * HW + r, g * (C // G) + c
        return (f'path {path}, family {family}, {dtype}, image {b}, group {g}, worst element [row {r}, channel {col}]: '
                f'got {float(got[row, col]):.6f} ref {float(ref[row, col]):.6f}')
    return _worst('groupnorm', emax, rmax, el2, rl2, _tol(dtype), where)


def check_rows(path, family, got, ref, dtype, block=64, tol=None):
    """row-wise outputs [M, C] (LayerNorm, softmax) per block of `block` rows.  -> (worst max ratio, worst rel-L2)"""
    got, ref = got.double().to(ref.device), ref.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f'{path} / {family}: shape or non-finite output'
    M = ref.shape[0]
    err = (got - ref).abs()
    nb = (M + block - 1) // block
    sl = [slice(i * block, min(M, (i + 1) * block)) for i in range(nb)]
    emax, rmax = torch.stack([err[s].max() for s in sl]), torch.stack([ref[s].abs().max() for s in sl])
    el2, rl2 = torch.stack([(err[s] ** 2).mean().sqrt() for s in sl]), torch.stack([(ref[s] ** 2).mean().sqrt() for s in sl])

    def where(i):
        e = err[sl[i]]
        r, c = divmod(int(e.argmax()), ref.shape[1])
        row = i * block + r
        return (f'path {path}, family {family}, {dtype}, rows {sl[i].start}..{sl[i].stop - 1}, worst element [row {row}, column {c}]: '
                f'got {float(got[row, c]):.6f} ref {float(ref[row, c]):.6f}')
    return _worst('rows', emax, rmax, el2, rl2, _tol(dtype) if tol is None else tol, where)


class Worst:
    """worst ratio per (path, family, dtype), printed once"""

    def __init__(self):
        self.t = {}

    def add(self, path, family, dtype, ratios):
        k = (path, family, str(dtype).replace('torch.', ''))
        self.t[k] = max(self.t.get(k, 0.0), max(ratios))

    def table(self, fams=FAMILIES):
        paths = sorted({(p, d) for p, f, d in self.t if f in fams})
        lines = [f'{"path":46s} {"dtype":8s} ' + ' '.join(f'{f:>9s}' for f in fams)]
        for p, d in paths:
            lines.append(f'{p:46s} {d:8s} ' + ' '.join(f'{self.t[(p, f, d)]:9.1e}' if (p, f, d) in self.t else f'{"-":>9s}' for f in fams))
        return '\n'.join(lines)
