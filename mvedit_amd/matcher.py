"""The LoFTR feature matcher on the native executor, and its primitives.

`LoFTREngine` is the reference's `LoFTR(config=default_cfg)` (loftr/loftr.py; `init_matcher`, lib/apis/adapter3d.py:411-415): it takes the `batch`
dict of `lib/core/utils/pose_estimation.py` and fills in the keys the callers read.  Behind it: `mve_loftr_create / _plan / _forward_coarse /
_forward_fine` (plans in csrc/builder_loftr.h) with ONE host read per forward, the match count.  The functions below it are typed wrappers over
section 2f of include/mvedit_amd.h (csrc/loftr.hip) and the two host-side preparations -- the sinusoidal position table and the BatchNorm fold.

    stem_rows / leaky_relu / pos_add        the backbone's operand rows, the FPN heads' activation, the position add
    linear_attention                        LinearAttention.forward without masks (mve_linattn_kv + mve_linattn_apply)
    dual_softmax / select_matches           CoarseMatching's conf_matrix and get_coarse_match (match_type 'dual_softmax', no masks)
    unfold_windows / fine_match             FinePreprocess' window gather and FineMatching

Tensors are PyTorch-ROCm tensors used as storage.  No op here has a torch fallback: importing `mvedit_amd._lib` raises when the library is missing,
and an input or configuration the native plan does not cover is refused (NotImplementedError / ValueError) before anything is launched.
"""
import copy
import ctypes
import math

import torch

from . import _lib
from .module_surface import EngineHandle

_DT = {torch.float16: 1, torch.bfloat16: 2}
WINDOW = 5          # the fine window the kernels are written for (FINE_WINDOW_SIZE)
MAX_GRID = 256      # PositionEncodingSine's max_shape


def _s(t):
    return _lib.stream_ptr(t.device)


def _chk16(*ts):
    for t in ts:
        if not (t.is_cuda and t.dtype in _DT and t.stride(-1) == 1):
            raise ValueError(f'expected a 16-bit device tensor with a dense last axis, got {t.dtype} {tuple(t.shape)} on {t.device}')


def _chk32(*ts):
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f'expected a contiguous float32 device tensor, got {t.dtype} {tuple(t.shape)} on {t.device}')


# ---- host-side preparation (float64, one rounding) -----------------------------------------------------------------------------------------------

def position_table(d_model, h, w, temp_bug_fix=True):
    """PositionEncodingSine's table for an h x w grid as float64 [h*w, d_model] (token-major, the layout pos_add takes).
    temp_bug_fix=False keeps the released checkpoints' form, Python's precedence included: `-log(1e4) / d_model // 2` is
    `(-log(1e4) / d_model) // 2`, a floor division of a small negative number, i.e. -1."""
    if d_model % 4:
        raise ValueError(f'd_model {d_model} must be a multiple of 4')
    if not (1 <= h <= MAX_GRID and 1 <= w <= MAX_GRID):
        raise ValueError(f'a {h} x {w} grid exceeds the {MAX_GRID} x {MAX_GRID} position table')
    k = torch.arange(0, d_model // 2, 2, dtype=torch.float64)
    rate = -math.log(10000.0) / (d_model // 2) if temp_bug_fix else (-math.log(10000.0) / d_model) // 2
    div = torch.exp(k * rate)[None, None, :]                                       # [1, 1, d_model/4]
    y = torch.arange(1, h + 1, dtype=torch.float64)[:, None, None].expand(h, w, 1)
    x = torch.arange(1, w + 1, dtype=torch.float64)[None, :, None].expand(h, w, 1)
    pe = torch.empty(h, w, d_model, dtype=torch.float64)
    pe[..., 0::4] = torch.sin(x * div)
    pe[..., 1::4] = torch.cos(x * div)
    pe[..., 2::4] = torch.sin(y * div)
    pe[..., 3::4] = torch.cos(y * div)
    return pe.reshape(h * w, d_model)


def fold_batchnorm(weight, gamma, beta, mean, var, eps=1e-5):
    """Eval-mode BatchNorm2d folded into the bias-free convolution in front of it, in float64: -> (weight', bias') with
    conv(x, weight') + bias' == bn(conv(x, weight)).  The caller rounds once."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return weight.double() * s.view(-1, *([1] * (weight.dim() - 1))), beta.double() - mean.double() * s


# ---- backbone helpers -------------------------------------------------------------------------------------------------------------------------------

def stem_rows(pixels):
    """pixels [B,1,H,W] -> [B*(H/2)*(W/2), 56]: the 7 x 7 / 2, padding 3 windows in (ky, kx) order, columns 49..55 zero."""
    _chk16(pixels)
    if pixels.dim() != 4 or pixels.shape[1] != 1 or not pixels.is_contiguous():
        raise ValueError(f'pixels must be a contiguous [B, 1, H, W] tensor, got {tuple(pixels.shape)}')
    B, _, H, W = pixels.shape
    rows = torch.empty(B * (H // 2) * (W // 2), 56, dtype=pixels.dtype, device=pixels.device)
    with torch.cuda.device(pixels.device):
        _lib.call('mve_loftr_stem_rows', _DT[pixels.dtype], _lib.ptr(pixels), B, H, W, _lib.ptr(rows), 56, _s(pixels))
    return rows


def leaky_relu(x, slope=0.01, out=None):
    _chk16(x)
    if not x.is_contiguous():
        raise ValueError('leaky_relu takes a contiguous tensor')
    out = torch.empty_like(x) if out is None else out
    with torch.cuda.device(x.device):
        _lib.call('mve_loftr_leaky_relu', _DT[x.dtype], _lib.ptr(x), _lib.ptr(out), x.numel(), float(slope), _s(x))
    return out


def pos_add(x, table):
    """x [B, HW, C] (16-bit) + table [HW, C] (float32 on the device) -> [B, HW, C], one rounding."""
    _chk16(x)
    _chk32(table)
    B, HW, C = x.shape
    if tuple(table.shape) != (HW, C) or not x.is_contiguous():
        raise ValueError(f'table {tuple(table.shape)} does not fit contiguous tokens {tuple(x.shape)}')
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.call('mve_loftr_pos_add', _DT[x.dtype], _lib.ptr(x), _lib.ptr(table), _lib.ptr(y), B, HW, C, _s(x))
    return y


# ---- linear attention ---------------------------------------------------------------------------------------------------------------------------------

def linear_attention(q, k, v, heads, eps=1e-6, return_kv=False):
    """q [B, L, heads*D], k / v [B, S, heads*D] (row-strided views are fine) -> [B, L, heads*D]; D = 32 or 16.
    out = phi(q) . (phi(k)^T v) / (phi(q) . sum_s phi(k) + eps), phi = elu + 1, fp32 accumulation in a fixed order."""
    _chk16(q, k, v)
    B, L, C = q.shape
    S = k.shape[1]
    if k.shape != v.shape or k.shape[0] != B or k.shape[2] != C or C % heads:
        raise ValueError(f'shapes q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} do not fit {heads} heads')
    D = C // heads
    if D not in (32, 16):
        raise NotImplementedError(f'linear attention is written for head dims 32 and 16, not {D}')
    for t, n in ((q, L), (k, S), (v, S)):
        if t.stride(0) != n * t.stride(1):
            raise ValueError('q / k / v must be dense over (batch, token): stride(0) == tokens * stride(1)')
    kv = torch.empty(B * heads, D * D + D, dtype=torch.float32, device=q.device)
    nbytes = _lib.raw('mve_linattn_workspace_bytes')(B, S, heads, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes else None
    out = torch.empty(B, L, C, dtype=q.dtype, device=q.device)
    with torch.cuda.device(q.device):
        _lib.call('mve_linattn_kv', _DT[q.dtype], _lib.ptr(k), k.stride(1), _lib.ptr(v), v.stride(1), B, S, heads, D, _lib.ptr(kv), _lib.ptr(ws), nbytes, _s(q))
        _lib.call('mve_linattn_apply', _DT[q.dtype], _lib.ptr(q), q.stride(1), _lib.ptr(kv), _lib.ptr(out), C, B, L, heads, D, float(eps), _s(q))
    return (out, kv) if return_kv else out


# ---- coarse matching ----------------------------------------------------------------------------------------------------------------------------------

def dual_softmax(sim, S=None):
    """sim float32 [N, L, ld] (columns [S, ld) are padding and never read; S defaults to ld) -> conf float32 [N, L, S] =
    softmax over L * softmax over S."""
    _chk32(sim)
    N, L, ld = sim.shape
    S = ld if S is None else int(S)
    rs = torch.empty(N * L, 2, dtype=torch.float32, device=sim.device)
    cs = torch.empty(N * S, 2, dtype=torch.float32, device=sim.device)
    conf = torch.empty(N, L, S, dtype=torch.float32, device=sim.device)
    with torch.cuda.device(sim.device):
        _lib.call('mve_dsmax_stats', _lib.ptr(sim), N, L, S, ld, _lib.ptr(rs), _lib.ptr(cs), _s(sim))
        _lib.call('mve_dsmax_conf', _lib.ptr(sim), N, L, S, ld, _lib.ptr(rs), _lib.ptr(cs), _lib.ptr(conf), _s(sim))
    return conf


def select_matches(conf, hw0, hw1, thr=0.2, border=2, scale=8.0):
    """get_coarse_match on conf float32 [N, H0*W0, H1*W1]: -> dict(b_ids, i_ids, j_ids (int64 [M]), mconf (float32 [M]), mkpts0_c, mkpts1_c
    (float32 [M, 2], (x, y) * scale)), in ascending (b, i) order.  Reads the match count M back: the one host read of a forward."""
    _chk32(conf)
    (H0, W0), (H1, W1) = hw0, hw1
    N, L, S = conf.shape
    if (L, S) != (H0 * W0, H1 * W1):
        raise ValueError(f'conf {tuple(conf.shape)} does not fit grids {tuple(hw0)} and {tuple(hw1)}')
    dev, cap = conf.device, N * L
    ids = torch.empty(3, cap, dtype=torch.int64, device=dev)
    mconf = torch.empty(cap, dtype=torch.float32, device=dev)
    mk = torch.empty(2, cap, 2, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = _lib.raw('mve_dsmax_select_workspace_bytes')(N, L, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.call('mve_dsmax_select', _lib.ptr(conf), N, H0, W0, H1, W1, float(thr), int(border), float(scale), _lib.ptr(ids[0]), _lib.ptr(ids[1]), _lib.ptr(ids[2]),
                  _lib.ptr(mconf), _lib.ptr(mk[0]), _lib.ptr(mk[1]), _lib.ptr(count), _lib.ptr(ws), nbytes, _s(conf))
    M = int(count.item())
    return dict(b_ids=ids[0, :M], i_ids=ids[1, :M], j_ids=ids[2, :M], mconf=mconf[:M], mkpts0_c=mk[0, :M], mkpts1_c=mk[1, :M])


# ---- fine stage ---------------------------------------------------------------------------------------------------------------------------------------

def unfold_windows(feat, b_ids, ids):
    """feat [N, Hf, Wf, C] NHWC, b_ids / ids int64 [M] (coarse cell ids on the Hf/4 x Wf/4 grid) -> [M, 25, C]: the 5 x 5 windows (stride 4,
    padding 2, zero outside) around the matched cells."""
    _chk16(feat)
    N, Hf, Wf, C = feat.shape
    M = int(b_ids.shape[0])
    if not (feat.is_contiguous() and b_ids.dtype == ids.dtype == torch.int64 and b_ids.is_cuda and ids.is_cuda and ids.shape[0] == M):
        raise ValueError('unfold_windows takes a contiguous NHWC map and int64 device ids of one length')
    rows = torch.empty(M, WINDOW * WINDOW, C, dtype=feat.dtype, device=feat.device)
    if M == 0:
        return rows
    b_ids, ids = b_ids.contiguous(), ids.contiguous()
    with torch.cuda.device(feat.device):
        _lib.call('mve_loftr_unfold', _DT[feat.dtype], _lib.ptr(feat), N, Hf, Wf, C, _lib.ptr(b_ids), _lib.ptr(ids), M, _lib.ptr(rows), _s(feat))
    return rows


def fine_match(feat0, feat1, mkpts1_c, radius):
    """feat0 / feat1 [M, 25, C], mkpts1_c float32 [M, 2] -> (expec_f float32 [M, 3], mkpts1_f float32 [M, 2]);
    radius = (window // 2) * (image height / fine map height)."""
    _chk16(feat0, feat1)
    M, WW, C = feat0.shape
    if WW != WINDOW * WINDOW or feat1.shape != feat0.shape or not (feat0.is_contiguous() and feat1.is_contiguous()):
        raise ValueError(f'fine_match takes two contiguous [M, 25, C] tensors, got {tuple(feat0.shape)} and {tuple(feat1.shape)}')
    expec = torch.empty(M, 3, dtype=torch.float32, device=feat0.device)
    if M == 0:
        return expec, mkpts1_c
    mkpts1_c = mkpts1_c.contiguous()
    _chk32(mkpts1_c)
    mk1 = torch.empty(M, 2, dtype=torch.float32, device=feat0.device)
    with torch.cuda.device(feat0.device):
        _lib.call('mve_loftr_fine_match', _DT[feat0.dtype], _lib.ptr(feat0), _lib.ptr(feat1), M, C, _lib.ptr(mkpts1_c), float(radius), _lib.ptr(expec), _lib.ptr(mk1), _s(feat0))
    return expec, mk1


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------------------

DEFAULT_CONFIG = dict(
    backbone_type='ResNetFPN', resolution=(8, 2), fine_window_size=5, fine_concat_coarse_feat=True,
    resnetfpn=dict(initial_dim=128, block_dims=[128, 196, 256]),
    coarse=dict(d_model=256, d_ffn=256, nhead=8, layer_names=['self', 'cross'] * 4, attention='linear', temp_bug_fix=False),
    match_coarse=dict(thr=0.2, border_rm=2, match_type='dual_softmax', dsmax_temperature=0.1),
    fine=dict(d_model=128, d_ffn=128, nhead=8, layer_names=['self', 'cross'], attention='linear'))
COARSE_TAPS = ('stem', 'layer1', 'layer2', 'layer3', 'fpn_c', 'pos') + tuple(f'c{k}' for k in range(8))
FINE_TAPS = ('unfold', 'merged', 'fine')
_BLOCK_DIMS, _PADDED = (128, 196, 256), (128, 200, 256)      # the 196-wide stage runs as 200 channels, the last 4 zero


def check_config(config):
    """-> the config as a plain nested dict (keys lower-case, as `lower_config` gives them); NotImplementedError for what the native plan is not."""
    def plain(c):
        return {str(k).lower(): plain(v) for k, v in c.items()} if hasattr(c, 'items') else c
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    for k, v in plain(config or {}).items():
        if isinstance(v, dict) and isinstance(cfg.get(k), dict):
            cfg[k].update(v)
        else:
            cfg[k] = v
    no = NotImplementedError
    if cfg['backbone_type'] != 'ResNetFPN' or tuple(cfg['resolution']) != (8, 2):
        raise no(f"backbone {cfg['backbone_type']} at resolution {tuple(cfg['resolution'])}: the native plan is ResNetFPN_8_2")
    if cfg['fine_window_size'] != WINDOW:
        raise no(f"fine_window_size {cfg['fine_window_size']}: the fine kernels are written for a window of {WINDOW}")
    if not cfg['fine_concat_coarse_feat']:
        raise no('fine_concat_coarse_feat=False: the native fine stage merges the coarse feature')
    if cfg['match_coarse']['match_type'] != 'dual_softmax':
        raise no(f"match_type {cfg['match_coarse']['match_type']!r}: the native matcher is dual_softmax")
    if abs(cfg['match_coarse']['dsmax_temperature'] - 0.1) > 1e-12:
        raise no(f"dsmax_temperature {cfg['match_coarse']['dsmax_temperature']}: the similarity scale of the native plan is 1 / (C * 0.1)")
    if cfg['resnetfpn']['initial_dim'] != 128 or tuple(cfg['resnetfpn']['block_dims']) != _BLOCK_DIMS:
        raise no(f"ResNetFPN {cfg['resnetfpn']}: the native plan is 1 -> 128 -> [128, 196, 256]")
    for part, d_model, names, hd in (('coarse', 256, ['self', 'cross'] * 4, 32), ('fine', 128, ['self', 'cross'], 16)):
        c = cfg[part]
        if c['attention'] != 'linear':
            raise no(f"{part}.attention {c['attention']!r}: the native transformer is linear attention")
        if c['d_model'] % c['nhead'] or c['d_model'] // c['nhead'] != hd:
            raise no(f"{part}: d_model {c['d_model']} / nhead {c['nhead']}: the native head dim is {hd}")
        if c['d_model'] != d_model or list(c['layer_names']) != names:
            raise no(f"{part}: d_model {c['d_model']} with layers {list(c['layer_names'])}: the native plan is {d_model} wide over {names}")
    return cfg


def key_table():
    """engine-side logical name -> the reference's state-dict key (after the `matcher.` prefix is stripped), every key of LoFTR(default_cfg) exactly
    once.  A logical name that starts with '_' is accepted and dropped (`num_batches_tracked`)."""
    t = {}

    def bn(logical, key):
        for k in ('weight', 'bias', 'running_mean', 'running_var'):
            t[f'{logical}.{k}'] = f'{key}.{k}'
        t[f'_{logical}.num_batches_tracked'] = f'{key}.num_batches_tracked'

    t['stem.conv'] = 'backbone.conv1.weight'
    bn('stem.bn', 'backbone.bn1')
    for li in (1, 2, 3):
        for b in (0, 1):
            for i in (1, 2):
                t[f'l{li}.b{b}.c{i}.conv'] = f'backbone.layer{li}.{b}.conv{i}.weight'
                bn(f'l{li}.b{b}.c{i}.bn', f'backbone.layer{li}.{b}.bn{i}')
            if b == 0 and li > 1:
                t[f'l{li}.b{b}.ds.conv'] = f'backbone.layer{li}.{b}.downsample.0.weight'
                bn(f'l{li}.b{b}.ds.bn', f'backbone.layer{li}.{b}.downsample.1')
    for n in (3, 2, 1):
        t[f'l{n}oc.conv'] = f'backbone.layer{n}_outconv.weight'
    for n in (2, 1):
        t[f'l{n}oc2.0.conv'] = f'backbone.layer{n}_outconv2.0.weight'
        bn(f'l{n}oc2.0.bn', f'backbone.layer{n}_outconv2.1')
        t[f'l{n}oc2.3.conv'] = f'backbone.layer{n}_outconv2.3.weight'
    for tag, mod, n in (('c', 'loftr_coarse', 8), ('f', 'loftr_fine', 2)):
        for k in range(n):
            for m in ('q_proj', 'k_proj', 'v_proj', 'merge'):
                t[f'{tag}{k}.{m}'] = f'{mod}.layers.{k}.{m}.weight'
            t[f'{tag}{k}.mlp0'] = f'{mod}.layers.{k}.mlp.0.weight'
            t[f'{tag}{k}.mlp2'] = f'{mod}.layers.{k}.mlp.2.weight'
            for m in ('norm1', 'norm2'):
                t[f'{tag}{k}.{m}.weight'] = f'{mod}.layers.{k}.{m}.weight'
                t[f'{tag}{k}.{m}.bias'] = f'{mod}.layers.{k}.{m}.bias'
    for logical, key in (('dp', 'down_proj'), ('mf', 'merge_feat')):
        t[f'{logical}.weight'] = f'fine_preprocess.{key}.weight'
        t[f'{logical}.bias'] = f'fine_preprocess.{key}.bias'
    return t


def match_state_dict(state_dict):
    """-> {logical name: tensor} with every key of `state_dict` consumed exactly once (a `matcher.` prefix stripped, as the reference's own
    `load_state_dict` override does); a missing or unused key is named in a KeyError."""
    sd = {(k[len('matcher.'):] if k.startswith('matcher.') else k): v for k, v in state_dict.items()}
    if len(sd) != len(state_dict):
        raise KeyError('state dict holds a key both with and without the matcher. prefix')
    out, used = {}, set()
    for logical, key in key_table().items():
        if key not in sd:
            raise KeyError(f'LoFTR parameter {key} is missing from the state dict')
        used.add(key)
        if not logical.startswith('_'):
            out[logical] = sd[key]
    unused = [k for k in sd if k not in used]
    if unused:
        raise KeyError(f'state dict key {unused[0]} is not a parameter of LoFTR(default_cfg) ({len(unused)} unused)')
    return out


def _pad_to(w, out_ch=None, in_ch=None):
    if in_ch is not None and w.shape[1] < in_ch:
        w = torch.cat([w, w.new_zeros(w.shape[0], in_ch - w.shape[1], *w.shape[2:])], 1)
    if out_ch is not None and w.shape[0] < out_ch:
        w = torch.cat([w, w.new_zeros(out_ch - w.shape[0], *w.shape[1:])], 0)
    return w


def pack_slots(params):
    """{logical name: tensor} -> {engine slot: float64 tensor of the slot's size}: BatchNorm folded in float64, 196 -> 200 channels, conv K order."""
    from .normal_model import conv_k_order
    g = lambda n: params[n].detach().double()
    pad = lambda c: 200 if c == 196 else c
    s = {}

    def conv_bn(slot, logical, bn=True):
        w = g(logical + '.conv')
        b = None
        if bn:
            w, b = fold_batchnorm(w, g(logical + '.bn.weight'), g(logical + '.bn.bias'), g(logical + '.bn.running_mean'), g(logical + '.bn.running_var'))
        O, I = pad(w.shape[0]), pad(w.shape[1])
        w = _pad_to(w, O, I)
        if w.shape[2] == 3:
            s[slot + '.w'] = conv_k_order(w)
        elif w.shape[2] == 7:
            s[slot + '.w'] = torch.nn.functional.pad(w.reshape(O, 49), (0, 7))
        else:
            s[slot + '.w'] = w.reshape(O, I)
        if b is not None:
            s[slot + '.b'] = _pad_to(b[:, None], O)[:, 0]

    conv_bn('stem', 'stem')
    for li in (1, 2, 3):
        for b in (0, 1):
            for i in (1, 2):
                conv_bn(f'l{li}.b{b}.c{i}', f'l{li}.b{b}.c{i}')
            if b == 0 and li > 1:
                conv_bn(f'l{li}.b{b}.ds', f'l{li}.b{b}.ds')
    for n in (3, 2, 1):
        conv_bn(f'l{n}oc', f'l{n}oc', bn=False)
    for n in (2, 1):
        conv_bn(f'l{n}oc2.0', f'l{n}oc2.0')
        conv_bn(f'l{n}oc2.3', f'l{n}oc2.3', bn=False)
    for tag, n in (('c', 8), ('f', 2)):
        for k in range(n):
            p = f'{tag}{k}'
            s[p + '.q.w'], s[p + '.merge.w'] = g(p + '.q_proj'), g(p + '.merge')
            s[p + '.kv.w'] = torch.cat([g(p + '.k_proj'), g(p + '.v_proj')], 0)
            s[p + '.mlp0.w'], s[p + '.mlp2.w'] = g(p + '.mlp0'), g(p + '.mlp2')
            for i in (1, 2):
                s[f'{p}.n{i}.g'], s[f'{p}.n{i}.b'] = g(f'{p}.norm{i}.weight'), g(f'{p}.norm{i}.bias')
    for p in ('dp', 'mf'):
        s[p + '.w'], s[p + '.b'] = g(p + '.weight'), g(p + '.bias')
    return s


class LoFTREngine(EngineHandle):
    """`LoFTR(config=default_cfg)` (either `temp_bug_fix`) on the native executor: `engine(batch)` updates the reference's batch dict in place."""

    def __init__(self, config=None, dtype=torch.float16, device='cuda'):
        if dtype not in _DT:
            raise NotImplementedError(f'LoFTREngine in {dtype}: the engine is fp16 or bf16')
        self.cfg = check_config(config)
        self.config = self.cfg
        self.dtype, self.device = dtype, torch.device(device)
        self.thr, self.border = float(self.cfg['match_coarse']['thr']), int(self.cfg['match_coarse']['border_rm'])
        self._h = ctypes.c_void_p()
        _lib.call('mve_loftr_create', ctypes.byref(self._h), _DT[dtype])
        self._ws, self._pos = None, {}
        self.training = False

    @classmethod
    def from_module(cls, m, dtype=None, device=None):
        """From a loaded reference `LoFTR`: its config, state dict, dtype and device (a module on the CPU gives a plan-only engine)."""
        p = next(iter(m.parameters()))
        dtype = dtype or (p.dtype if p.dtype in _DT else torch.float16)
        device = torch.device(device) if device is not None else p.device
        eng = cls(getattr(m, 'config', None), dtype=dtype, device=device)
        if device.type != 'cpu':
            eng.load_state_dict(m.state_dict())
        return eng

    def load_state_dict(self, state_dict, strict=True):
        if not strict:
            raise NotImplementedError('LoFTREngine.load_state_dict(strict=False): every key is consumed exactly once')
        slots = pack_slots(match_state_dict(state_dict))
        with torch.cuda.device(self.device):
            s = _lib.stream_ptr(self.device)
            keep = []
            for name, t in slots.items():
                if name.endswith('.w'):                                 # a 16-bit slot: ONE rounding, float64 -> engine dtype (its fp32 image is exact)
                    t = t.to(self.dtype)
                t = t.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
                keep.append(t)
                shape = (ctypes.c_longlong * 1)(t.numel())
                _lib.call('mve_unet_load_param', self._h, name.encode(), _lib.ptr(t), 0, 1, shape, s)
            torch.cuda.current_stream(self.device).synchronize()
        missing, first = self._missing_params()
        if missing:
            raise KeyError(f'{missing} LoFTR slots were not filled (first: {first})')
        return self

    # ---- the nn.Module sliver the runner touches (`init_matcher().requires_grad_(False).to(device)`) ----------------------------------------------
    def train(self, mode=True):
        if mode:
            raise NotImplementedError('LoFTREngine.train(): the engine is inference only')
        return self

    # ---- planning -------------------------------------------------------------------------------------------------------------------------------
    def plan(self, N, H, W, phase=1):
        ws, n_ops, flops = ctypes.c_size_t(), ctypes.c_int(), (ctypes.c_double * 5)()
        _lib.call('mve_loftr_plan', self._h, int(phase), int(N), int(H), int(W), ctypes.byref(ws), ctypes.byref(n_ops), flops)
        return self._plan_result(ws, n_ops, flops)

    def op_table(self):
        return [row[1:] for row in self._op_rows()]

    # ---- forward ----------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def check_images(image0, image1):
        for name, im in (('image0', image0), ('image1', image1)):
            if not torch.is_tensor(im) or im.dim() != 4 or im.shape[1] != 1 or im.shape[0] == 0 or not im.is_floating_point():
                raise ValueError(f'{name}: {tuple(im.shape) if torch.is_tensor(im) else type(im).__name__} is not a floating-point [N, 1, H, W] tensor')
        if image0.shape != image1.shape:
            raise ValueError(f'image0 {tuple(image0.shape)} and image1 {tuple(image1.shape)} differ: the native plan runs the pair as one batch')
        N, _, H, W = image0.shape
        if H % 8 or W % 8:
            raise ValueError(f'H = {H} and W = {W} must be multiples of 8 (the coarse grid is 1/8)')
        if H // 8 > MAX_GRID or W // 8 > MAX_GRID:
            raise ValueError(f'a {H // 8} x {W // 8} coarse grid exceeds the {MAX_GRID} x {MAX_GRID} position table')
        return N, H, W

    def _table(self, hc, wc):
        if (hc, wc) not in self._pos:
            self._pos[(hc, wc)] = position_table(256, hc, wc, bool(self.cfg['coarse']['temp_bug_fix'])).to(device=self.device, dtype=torch.float32).contiguous()
        return self._pos[(hc, wc)]

    def run(self, image0, image1, coarse_matches=None, output_features=False, profile=False, thr=None):
        """-> the dict of keys the reference's forward adds to `batch`; with output_features=True -> (dict, taps).  `coarse_matches=(b_ids, i_ids,
        j_ids)` forces the fine stage onto the given matches (mkpts*_c, m_bids follow them; mconf is read from conf_matrix)."""
        N, H, W = self.check_images(image0, image1)
        dev, dt = self.device, self.dtype
        Hc, Wc, H2, W2 = H // 8, W // 8, H // 2, W // 2
        L, Sp, cap = Hc * Wc, (Hc * Wc + 7) // 8 * 8, N * Hc * Wc
        images = torch.cat([image0, image1], 0).to(device=dev, dtype=dt).contiguous()
        ms = []
        with torch.cuda.device(dev):
            table = self._table(Hc, Wc)
            info = self.plan(N, H, W, 1)
            ws = self._workspace(info['workspace_bytes'])
            f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
            io = [torch.empty(2 * N, H2, W2, 128, dtype=dt, device=dev), torch.empty(2 * N, L, 256, dtype=dt, device=dev), torch.empty(N, L, Sp, **f32),
                  torch.empty(N, L, L, **f32), torch.empty(cap, **i64), torch.empty(cap, **i64), torch.empty(cap, **i64), torch.empty(cap, **f32),
                  torch.empty(cap, 2, **f32), torch.empty(cap, 2, **f32), torch.zeros(4, dtype=torch.int32, device=dev), None, None]
            taps = None
            if output_features:
                shapes = [(2 * N, H2, W2, 128), (2 * N, H2, W2, 128), (2 * N, H // 4, W // 4, 200), (2 * N, Hc, Wc, 256), (2 * N, Hc, Wc, 256)] + [(2 * N, L, 256)] * 9
                taps = [torch.empty(s, dtype=dt, device=dev) for s in shapes]
            ptr = lambda ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
            op_ms = (ctypes.c_float * info['n_ops'])() if profile else None
            _lib.call('mve_loftr_forward_coarse', self._h, _lib.ptr(images), _lib.ptr(table), N, H, W, float(self.thr if thr is None else thr), self.border, ptr(io),
                      ptr(taps) if taps else None, _lib.ptr(ws), ws.numel(), op_ms, _lib.stream_ptr(dev))
            if profile:
                ms.append((self.op_table(), list(op_ms)))
            conf = io[3]
            if coarse_matches is None:
                M = int(io[10][0].item())                               # the one host read of a forward: every fine output is shaped [M, ...]
                b_ids, i_ids, j_ids, mconf, mk0, mk1 = io[4][:M], io[5][:M], io[6][:M], io[7][:M], io[8][:M], io[9][:M]
            else:
                b_ids, i_ids, j_ids = (torch.as_tensor(t).to(device=dev, dtype=torch.int64).contiguous() for t in coarse_matches)
                M = int(b_ids.shape[0])
                if not (i_ids.shape == j_ids.shape == b_ids.shape == (M,)) or M > cap:
                    raise ValueError(f'coarse_matches: three id vectors of one length <= N * L = {cap} are needed')
                if M and (int(b_ids.min()) < 0 or int(b_ids.max()) >= N or int(torch.minimum(i_ids.min(), j_ids.min())) < 0 or int(torch.maximum(i_ids.max(), j_ids.max())) >= L):
                    raise ValueError('coarse_matches: an id lies outside its range')
                mconf = conf[b_ids, i_ids, j_ids]
                mk0 = (torch.stack([i_ids % Wc, i_ids // Wc], 1) * 8).float()
                mk1 = (torch.stack([j_ids % Wc, j_ids // Wc], 1) * 8).float()
                io[4], io[5], io[6], io[9] = b_ids, i_ids, j_ids, mk1.contiguous()
            out = dict(bs=N, hw0_i=images.shape[2:], hw1_i=images.shape[2:], hw0_c=torch.Size((Hc, Wc)), hw1_c=torch.Size((Hc, Wc)), hw0_f=torch.Size((H2, W2)),
                       hw1_f=torch.Size((H2, W2)), W=WINDOW, conf_matrix=conf, b_ids=b_ids, i_ids=i_ids, j_ids=j_ids, m_bids=b_ids, mconf=mconf, mkpts0_c=mk0,
                       mkpts1_c=mk1, gt_mask=mconf == 0)
            ftaps = None
            if M == 0:                                                  # FineMatching's corner case: the fine key points ARE the (empty) coarse ones
                out.update(expec_f=torch.empty(0, 3, **f32), mkpts0_f=mk0, mkpts1_f=mk1)
            else:
                info = self.plan(N, H, W, 2)
                ws = self._workspace(info['workspace_bytes'])
                io[11], io[12] = torch.empty(M, 3, **f32), torch.empty(M, 2, **f32)
                if output_features:
                    ftaps = [torch.empty(2 * M, 25, 128, dtype=dt, device=dev) for _ in FINE_TAPS]
                op_ms = (ctypes.c_float * info['n_ops'])() if profile else None
                _lib.call('mve_loftr_forward_fine', self._h, N, H, W, M, ptr(io), ptr(ftaps) if ftaps else None, _lib.ptr(ws), ws.numel(), op_ms, _lib.stream_ptr(dev))
                if profile:
                    ms.append((self.op_table(), list(op_ms)))
                out.update(expec_f=io[11], mkpts0_f=mk0, mkpts1_f=io[12])
        res = out
        if output_features:
            feats = {n: (t if t.dim() == 3 else t.permute(0, 3, 1, 2)) for n, t in zip(COARSE_TAPS, taps)}
            feats.update(fpn_f=io[0].permute(0, 3, 1, 2), feat_c=io[1], sim_matrix=io[2][..., :L])
            if ftaps:
                feats.update({n: t for n, t in zip(FINE_TAPS, ftaps)})
            res = (out, feats)
        if profile:
            res = (res if isinstance(res, tuple) else (res,)) + (ms,)
        return res

    def forward(self, batch):
        if 'mask0' in batch or 'mask1' in batch:
            raise NotImplementedError('LoFTREngine: mask0 / mask1 (padded training batches) are not part of the native plan')
        if 'scale0' in batch or 'scale1' in batch:
            raise NotImplementedError('LoFTREngine: scale0 / scale1 (resized evaluation pairs) are not part of the native plan')
        batch.update(self.run(batch['image0'], batch['image1']))
        return None

    __call__ = forward
