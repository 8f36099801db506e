"""Activation statistics that real checkpoints produce and `randn` does not, float64 references of the reduction ops, and the per-group check.

Shared by test_norm_stress_gpu.py, test_attention_paths_gpu.py and the LayerNorm cases of test_loftr_kernels_gpu.py / test_sam_decoder_kernels_gpu.py.
The attention inputs (families, shapes and float64 references of the causal, relative-position, linear and vision-shape attention kernels) are
described at `attn_qkv` / `attn_case` below and shared by test_attention_stress_gpu.py and test_attention_bar_teeth.py.

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


def _heads(t, B, L, heads, d):
    return t.double().reshape(B, L, heads, d).transpose(1, 2)


def causal_attention_ref(q, k, v, B, L, heads, d, scale=None):
    """float64 causal softmax attention (query i sees keys 0..i); q / k / v [B L, heads d] -> [B L, heads d]"""
    q, k, v = (_heads(t, B, L, heads, d) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) * (d ** -0.5 if scale is None else scale)
    s = s.masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(), float('-inf'))
    return (softmax_ref(s) @ v).transpose(1, 2).reshape(B * L, heads * d)


def relpos_logits(q, k, rel_h, rel_w, gh, gw, scale):
    """q, k [..., L, d] (any float dtype: the arithmetic runs in it), rel_h [2 gh - 1, d], rel_w [2 gw - 1, d] ->
    scale q.k + q.Rh[qh - kh + gh - 1] + q.Rw[qw - kw + gw - 1] with (qh, qw) = (q / gw, q % gw), [..., L, L]"""
    i = torch.arange(gh * gw)
    ih, iw = i // gw, i % gw
    th, tw = q @ rel_h.transpose(0, 1), q @ rel_w.transpose(0, 1)                   # [..., L, 2 gh - 1], [..., L, 2 gw - 1]
    jh = (ih[:, None] - ih[None, :] + gh - 1).expand(q.shape[:-2] + (-1, -1))
    jw = (iw[:, None] - iw[None, :] + gw - 1).expand(q.shape[:-2] + (-1, -1))
    return q @ k.transpose(-1, -2) * scale + th.gather(-1, jh) + tw.gather(-1, jw)


def relpos_attention_ref(q, k, v, rel_h, rel_w, NS, gh, gw, heads, d, scale=None):
    """float64 attention with the decomposed relative-position bias (the statement of tests/sam_rule.py's relpos_attention: the two agree, see
    test_attention_bar_teeth.py); q / k / v [NS gh gw, heads d] -> [NS gh gw, heads d]"""
    L = gh * gw
    q, k, v = (_heads(t, NS, L, heads, d) for t in (q, k, v))
    s = relpos_logits(q, k, rel_h.double(), rel_w.double(), gh, gw, d ** -0.5 if scale is None else scale)
    return (softmax_ref(s) @ v).transpose(1, 2).reshape(NS * L, heads * d)


def linear_attention_ref(q, k, v, B, L, S, heads, D, eps=1e-6):
    """float64 linear attention, phi(x) = x + 1 for x > 0 and exp(x) otherwise (elu + 1); q [B L, heads D], k / v [B S, heads D] ->
    (out [B L, heads D], KV [B heads, D D], Ksum [B heads, D])"""
    phi = lambda t: torch.where(t > 0, t + 1, torch.exp(t.clamp(max=0)))
    Q, K, V = phi(q.double()).reshape(B, L, heads, D), phi(k.double()).reshape(B, S, heads, D), v.double().reshape(B, S, heads, D)
    KV = torch.einsum('nshd,nshv->nhdv', K, V)
    Ksum = K.sum(1)
    Z = 1 / (torch.einsum('nlhd,nhd->nlh', Q, Ksum) + eps)
    out = torch.einsum('nlhd,nhdv,nlh->nlhv', Q, KV, Z).reshape(B * L, heads * D)
    return out, KV.reshape(B * heads, D * D), Ksum.reshape(B * heads, D)


# ---- attention inputs ------------------------------------------------------------------------------------------------------------------------------
# Softmax attention (mve_attention, mve_attention_causal, mve_attention_relpos): one packed [B L, 3 C] buffer of the storage dtype, q | k | v its column
# blocks, made from rnd(..., scale 1.5).  Every change is applied in every batch item and head.
#   randn          the buffer as it is: the anchor
#   spike          one query row x 6 and one key row copied from it: the logit of that pair is far above the row's others, so the running maximum
#                  of an online softmax jumps at that key.  Non-causal: query 5, key L - 3 -- or L - 1 where L - 3 is not in the last, partly
#                  filled tile of `tile` keys (L = 65: key 64).  Causal: the key must be visible, so query L - 2 and key L - 3
#   large+offset   q and k x 2 (sharp rows), V + 2: an error of the denominator shows in every output element
#   negative       q = -(|q| + 2), k = |k| + 2: every logit far below zero; a zero-padded key (logit 0) would win the maximum and the sum
#   sink           causal only: key row 0 x 4, every query shifted by 0.5 sign(k0), V[0] x 40 -- every row puts a large share on key 0, whose value
#                  is 40 x the others'
# Rel-pos tables: rnd(..., scale `tables`) of the storage dtype; 0.1 (q.R of order 1) or 1.0 ('tables x1': q.R of order 10, the bias decides nearly
# every argmax; run with the randn and the negative buffer).
ATTN_FAMILIES = ('randn', 'spike', 'large+offset', 'negative', 'sink', 'tables x1', 'tables x1 neg')
PLAIN_FAMILIES = ('randn', 'spike', 'large+offset')
CAUSAL_FAMILIES = ('randn', 'spike', 'large+offset', 'negative', 'sink')
RELPOS_FAMILIES = ('randn', 'spike', 'large+offset', 'negative', 'tables x1', 'tables x1 neg')
LINATTN_FAMILIES = ('randn', 'keys-12', 'keys-20', 'qkv+8', 'v+32', 'outlier')


def _rnd(shape, dtype, seed, scale):
    from test_unet_ops import rnd
    return rnd(shape, dtype, seed, scale)


def spike_rows(L, causal, tile=64):
    """(query, key) of the spike family"""
    if causal:
        return L - 2, L - 3
    return 5, (L - 3 if (L - 3) // tile == (L - 1) // tile else L - 1)


def attn_qkv(family, B, L, heads, d, dtype, seed, causal=False):
    """packed [B L, 3 heads d] buffer of `dtype` (CPU)"""
    C = heads * d
    x = _rnd((B * L, 3 * C), dtype, seed, 1.5).float().reshape(B, L, 3, C)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    base = {'tables x1': 'randn', 'tables x1 neg': 'negative'}.get(family, family)
    if base == 'spike':
        qi, ki = spike_rows(L, causal)
        q[:, qi] = (q[:, qi] * 6).to(dtype).float()
        k[:, ki] = q[:, qi]
    elif base == 'large+offset':
        q *= 2
        k *= 2
        v += 2
    elif base == 'negative':
        q.copy_(-(q.abs() + 2))
        k.copy_(k.abs() + 2)
    elif base == 'sink':
        assert causal
        k[:, 0] *= 4
        q += 0.5 * torch.sign(k[:, :1])
        v[:, 0] *= 40
    elif base != 'randn':
        raise ValueError(family)
    return x.reshape(B * L, 3 * C).to(dtype)


def relpos_tables(family, gh, gw, d, dtype, seed):
    std = 1.0 if family.startswith('tables x1') else 0.1
    return _rnd((2 * gh - 1, d), dtype, seed, std), _rnd((2 * gw - 1, d), dtype, seed + 1, std)


def linattn_qkv(family, B, L, S, heads, D, dtype, seed):
    """(ql [B L, 3 C], ks [B S, 3 C]) of `dtype` (CPU): q is the first column block of ql, k | v the second and third of ks.  z = randn:
      randn      q = k = v = z
      keys-12    k = 0.5 z - 12: phi(k) = 6e-6
      keys-20    k = 0.5 z - 20: phi(k) = 2e-9, q.Ksum of the order of eps = 1e-6; elu(x) + 1 evaluated in fp32 would be 0 here
      qkv+8      q, k, v = z + 8
      v+32       v = 0.5 z + 32: the output is 32 +- 0.5 / sqrt(S), a ratio of two sums that share every rounding of phi
      outlier    one q / k channel and one v channel of every head x 40"""
    C = heads * D
    ql, ks = _rnd((B * L, 3 * C), dtype, seed, 1.0).float(), _rnd((B * S, 3 * C), dtype, seed + 1, 1.0).float()
    q, k, v = ql[:, :C], ks[:, C:2 * C], ks[:, 2 * C:]
    if family in ('keys-12', 'keys-20'):
        k.copy_(0.5 * k - float(family[5:]))
    elif family == 'qkv+8':
        q += 8
        k += 8
        v += 8
    elif family == 'v+32':
        v.copy_(0.5 * v + 32)
    elif family == 'outlier':
        h = torch.arange(heads)
        q[:, h * D + (3 * h + 1) % D] *= 40
        k[:, h * D + (3 * h + 1) % D] *= 40
        v[:, h * D + (5 * h + 2) % D] *= 40
    elif family != 'randn':
        raise ValueError(family)
    return ql.to(dtype), ks.to(dtype)


# The cases of test_attention_stress_gpu.py and test_attention_bar_teeth.py.  B (or NS) = 2 and heads = 2: the head and item offsets are exercised.
ATTN_B, ATTN_HEADS = 2, 2
CAUSAL_L = (17, 77, 128)                                               # d = 64
RELPOS_SHAPES = ((6, 10, 64), (10, 6, 80), (5, 13, 64), (1, 70, 80), (14, 14, 64))      # (gh, gw, d)
LINATTN_SHAPES = ((70, 300, 32), (25, 25, 16), (99, 99, 32))           # (L, S, D)
PLAIN_SHAPES = ((65, 64), (257, 80))                                   # (L, d) of mve_attention


@functools.lru_cache(maxsize=None)
def attn_case(kind, shape, family, dtype):
    """The inputs and the float64 reference of one case, computed once per process and shared (treat as read-only).
      'plain'   shape (L, d)        -> (qkv, ref)
      'causal'  shape L             -> (qkv, ref)
      'relpos'  shape (gh, gw, d)   -> (qkv, rel_h, rel_w, ref)
      'linear'  shape (L, S, D)     -> (ql, ks, ref, KV, Ksum)"""
    B, H = ATTN_B, ATTN_HEADS
    if kind == 'linear':
        L, S, D = shape
        C = H * D
        ql, ks = linattn_qkv(family, B, L, S, H, D, dtype, 11 + S)
        return (ql, ks) + linear_attention_ref(ql[:, :C], ks[:, C:2 * C], ks[:, 2 * C:], B, L, S, H, D)
    if kind == 'relpos':
        gh, gw, d = shape
        L, C = gh * gw, H * d
        qkv = attn_qkv(family, B, L, H, d, dtype, 21 + L)
        rel_h, rel_w = relpos_tables(family, gh, gw, d, dtype, 31 + L)
        return qkv, rel_h, rel_w, relpos_attention_ref(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], rel_h, rel_w, B, gh, gw, H, d)
    L, d = (shape, 64) if kind == 'causal' else shape
    C = H * d
    qkv = attn_qkv(family, B, L, H, d, dtype, 41 + L, causal=kind == 'causal')
    f = causal_attention_ref if kind == 'causal' else (lambda q, k, v, B, L, H, d: attention_ref(q, k, v, B, L, L, H, d))
    return qkv, f(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, L, H, d)


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
        w = [max(9, len(f)) for f in fams]
        lines = [f'{"path":46s} {"dtype":8s} ' + ' '.join(f'{f:>{n}s}' for f, n in zip(fams, w))]
        for p, d in paths:
            lines.append(f'{p:46s} {d:8s} ' + ' '.join(f'{self.t[(p, f, d)]:{n}.1e}' if (p, f, d) in self.t else f'{"-":>{n}s}' for f, n in zip(fams, w)))
        return '\n'.join(lines)
