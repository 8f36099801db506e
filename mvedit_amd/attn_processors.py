"""The diffusers attention-processor surface of the UNet / ControlNet engines: `attn_processors`, `set_attn_processor`, and the translation of
an installed table into the executor's attention options.  Pure Python, no native handle: the engines mix `AttnProcessorTable` in and supply
the two hooks (`_attn_names`, `_attn_push`); tests drive the same class with a recorder in place of the native calls.

The reference installs and mutates processor objects on whatever stands behind `pipe.unet` / `pipe.controlnet`:

    lib/models/architecture/joint_attn.py:40-54          apply_/remove_cross_image_attn_proc -> CrossImageAttnProcWrapper(base_attn_proc)
    lib/models/architecture/ip_adapter/ip_adapter.py:85-110, :61-62, :170-173
                                                         IPAttnProcessor on every attn2, AttnProcessor on every attn1, CNAttnProcessor on the
                                                         ControlNets; the weights are loaded INTO those objects afterwards through
                                                         ModuleList(unet.attn_processors.values()).load_state_dict (integer keys, table order),
                                                         and `.scale` is mutated later
    lib/pipelines/zero123plus.py:88-99, :187-190         ReferenceOnlyAttnProc(chained_proc, enabled=<attn1>, name=...)
    lib/models/architecture/diffusers.py:533-538         ReferenceAttnProc, likewise

None of these classes can be imported here (they live in the reference and in diffusers), so they are recognised by class name and attributes.
The kernels behind them exist already (builder_unet.h: the IP branch, reference attention 'w' / 'r' / 'm', the cross-image pairing, the context
tail of ControlNets); the table only decides which of them a forward uses.  There is no fallback: a processor or an arrangement the executor
cannot express raises NotImplementedError naming the layer and the class.
"""
from collections import OrderedDict

import torch

PLAIN_NAMES = ('AttnProcessor', 'AttnProcessor2_0', 'XFormersAttnProcessor')
IP_NAMES = ('IPAttnProcessor', 'IPAttnProcessor2_0')
CN_NAMES = ('CNAttnProcessor', 'CNAttnProcessor2_0')
CROSS_IMAGE_NAMES = ('CrossImageAttnProcWrapper',)
REFERENCE_NAMES = ('ReferenceOnlyAttnProc', 'ReferenceAttnProc')


def attn_processor_names(cfg):
    """The keys of `UNet2DConditionModel(**cfg).attn_processors` for an engine topology dict (mvedit_amd.unet.SD15_CONFIG ...), in order.

    diffusers 0.27.2 fills that dict by walking `named_children()` recursively, i.e. in module REGISTRATION order: `down_blocks`, then
    `up_blocks`, then `mid_block` (unet_2d_condition.py registers them in that order in __init__), inside a block `attentions.<j>`, inside a
    Transformer2DModel `transformer_blocks.<k>`, inside a BasicTransformerBlock `attn1` before `attn2`.  Up block i mirrors down level
    n - 1 - i and has layers_per_block + 1 attentions.  (A ControlNetModel has no `up_blocks`: controlnet_attn_processor_names.)

    ORDER UNPINNED: diffusers is not importable here, so this order is restated from its source and not checked against the library.  It
    matters: the reference loads the IP-Adapter weights with integer keys in this order (ip_adapter.py:61-62).  The published
    ip-adapter-plus_sd15 key layout (odd indices 1..31, 1280-wide rows at 31 = mid_block) agrees with it for SD-1.5; a wrong order would
    fail loudly there with a shape mismatch."""
    return _names(cfg, True)


def controlnet_attn_processor_names(cfg):
    """`ControlNetModel.attn_processors` keys: the UNet's without `up_blocks` (same order; unpinned like attn_processor_names)."""
    return _names(cfg, False)


def _names(cfg, up):
    n = len(cfg['block_out_channels'])
    L, attn, tl = cfg['layers_per_block'], cfg['down_attn'], cfg['transformer_layers']
    out = []

    def block(prefix, n_attn, depth):
        for j in range(n_attn):
            for k in range(depth):
                for a in ('attn1', 'attn2'):
                    out.append(f'{prefix}.attentions.{j}.transformer_blocks.{k}.{a}.processor')
    for i in range(n):
        if attn[i]:
            block(f'down_blocks.{i}', L, tl[i])
    if up:
        for i in range(n):
            if attn[n - 1 - i]:
                block(f'up_blocks.{i}', L + 1, tl[n - 1 - i])
    block('mid_block', 1, tl[n - 1])
    return out


class EngineAttnProcessor(torch.nn.Module):
    """What `attn_processors` holds before anything is set: the engine's plain attention.  A parameter-free nn.Module, so that
    `torch.nn.ModuleList(engine.attn_processors.values())` works (ip_adapter.py:61)."""


class Resolved:
    """A translated table: what the executor needs to know."""
    __slots__ = ('ip_tokens', 'ip_scale', 'ip_weights', 'reference', 'cn_tokens')

    def __init__(self):
        self.ip_tokens, self.ip_scale, self.ip_weights, self.reference, self.cn_tokens = 0, 1.0, [], False, 0


def _cls(p):
    return type(p).__name__


def _leaf(name, proc):
    """Peel the wrappers the reference nests -- CrossImageAttnProcWrapper outermost (joint_attn.py:43 wraps whatever is installed, at the
    start of a pipeline call), then at most one Reference*AttnProc (installed once around the processor of a fresh module) -- and return
    (leaf processor, the reference processor or None)."""
    ref, seen_ref = None, False
    p = proc
    for _ in range(8):
        c = _cls(p)
        if c in CROSS_IMAGE_NAMES and hasattr(p, 'base_attn_proc'):
            if seen_ref:
                raise NotImplementedError(f'{name}: {c} inside {_cls(ref)} -- the reference nests them the other way round '
                                          f'(joint_attn.py:43), this order is not implemented')
            p = p.base_attn_proc
        elif c in REFERENCE_NAMES and all(hasattr(p, a) for a in ('chained_proc', 'enabled', 'name')):
            if seen_ref:
                raise NotImplementedError(f'{name}: {c} nested in {_cls(ref)} is not implemented')
            ref, seen_ref = p, True
            p = p.chained_proc
        else:
            return p, ref
    raise NotImplementedError(f'{name}: attention processors nested more than 8 deep ({_cls(proc)})')


def _ident(t):
    """Host-side identity of a weight: storage address, in-place version, dtype, device.  No device access."""
    try:
        v = t._version
    except RuntimeError:          # inference tensors keep no version counter: an in-place update is invisible, so never call them unchanged
        v = None
    return (t.data_ptr(), v, t.dtype, t.device, tuple(t.shape))


class AttnProcessorTable:
    """Mixin: the processor table of one engine.

    Hooks of the host class:
        _attn_names()            -> list of processor names (attn_processor_names / controlnet_attn_processor_names of its config)
        _attn_push(name, tensor) -> hand one to_k_ip / to_v_ip weight to the executor under its state-dict name `<processor name>.to_k_ip.weight`
        _attn_is_controlnet      -> True on ControlNet engines (CNAttnProcessor allowed, IP / reference processors are not)

    `_attn_source`: a torch module (the diffusers model an engine was built from, mvedit_amd.dropin) whose own `attn_processors` /
    `set_attn_processor` are then the single source of truth -- the engine's delegate to them and every forward translates the module's
    current table, so code that talks to the module (lib/apis/adapter3d.py:325-336 `unload_ip_adapter`) reaches the engine.

    Until `set_attn_processor` is called (and without a source module) the table does not govern: `attn_processors` returns the defaults and
    the engine's keyword-driven behaviour (`set_ip_adapter`, `mode` / `ref_dict`) is what it was."""
    _attn_table = None
    _attn_explicit = False
    _attn_source = None
    _attn_pushed = None
    _attn_is_controlnet = False

    # ------------------------------------------------------------------ the diffusers surface
    def _attn_own_table(self):
        if self._attn_table is None:
            self._attn_table = OrderedDict((n, EngineAttnProcessor()) for n in self._attn_names())
        return self._attn_table

    @property
    def attn_processors(self):
        """Ordered {name: processor object}; the very objects that were passed to set_attn_processor."""
        if self._attn_source is not None:
            return self._attn_source.attn_processors
        return dict(self._attn_own_table())

    def set_attn_processor(self, processor):
        """diffusers' `set_attn_processor`: one object for every layer, or a dict with exactly the table's keys.  Stored by identity."""
        if self._attn_source is not None:
            return self._attn_source.set_attn_processor(processor)
        table = self._attn_own_table()
        if isinstance(processor, dict):
            if len(processor) != len(table):
                raise ValueError(f'A dict of processors was passed, but the number of processors {len(processor)} does not match the number of '
                                 f'attention layers: {len(table)}. Please make sure to pass {len(table)} processor classes.')
            unknown = [k for k in processor if k not in table]
            if unknown:
                raise ValueError(f'A dict of processors was passed, but {unknown[0]!r} is not the name of an attention layer '
                                 f'({len(unknown)} unknown keys; the names are those of `attn_processors`).')
            new = OrderedDict((n, processor[n]) for n in table)
        else:
            new = OrderedDict((n, processor) for n in table)
        self._attn_check(new)                      # a table the executor cannot express is refused before it is installed
        self._attn_table = new
        self._attn_explicit = True

    def set_use_memory_efficient_attention_xformers(self, valid, attention_op=None):
        """diffusers ModelMixin surface (lib/apis/adapter3d.py:309-313): the engine has one attention kernel, nothing to switch."""

    # ------------------------------------------------------------------ translation
    @property
    def _attn_governs(self):
        return self._attn_explicit or self._attn_source is not None

    def _attn_check(self, table):
        """Structure of a table -> [(name, leaf, reference processor)] or NotImplementedError naming the layer and the class."""
        rows = []
        n_ip = n_attn2 = n_cn = n_ref_on = 0
        for name, proc in table.items():
            leaf, ref = _leaf(name, proc)
            c = _cls(leaf)
            is_attn2 = name.endswith('attn2.processor')
            n_attn2 += is_attn2
            if c in IP_NAMES and all(hasattr(leaf, a) for a in ('to_k_ip', 'to_v_ip', 'scale', 'num_tokens')):
                if self._attn_is_controlnet:
                    raise NotImplementedError(f'{name}: {c} on a ControlNet engine is not implemented (the reference installs CNAttnProcessor there)')
                if not is_attn2:
                    raise NotImplementedError(f'{name}: {c} on a self-attention layer is not implemented (ip_adapter.py:98-103 installs it on attn2 only)')
                n_ip += 1
            elif c in CN_NAMES and hasattr(leaf, 'num_tokens'):
                if not self._attn_is_controlnet:
                    raise NotImplementedError(f'{name}: {c} is a ControlNet processor; on a UNet engine it is not implemented')
                n_cn += 1
            elif c in PLAIN_NAMES or isinstance(leaf, EngineAttnProcessor):
                pass
            else:
                raise NotImplementedError(f'{name}: attention processor {c} is not implemented by the engine')
            if ref is not None:
                if self._attn_is_controlnet:
                    raise NotImplementedError(f'{name}: {_cls(ref)} on a ControlNet engine is not implemented')
                n_ref_on += bool(ref.enabled)
            rows.append((name, leaf, ref))
        if n_ip and n_ip != n_attn2:
            missing, leaf = next((n, leaf) for n, leaf, _ in rows if n.endswith('attn2.processor') and _cls(leaf) not in IP_NAMES)
            raise NotImplementedError(f'{missing}: {_cls(leaf)} here while {n_ip} other cross-attention layers carry an '
                                      f'IP-Adapter processor -- the executor runs the image branch on every cross-attention or on none')
        if n_cn and n_cn != len(rows):
            missing, leaf = next((n, leaf) for n, leaf, _ in rows if _cls(leaf) not in CN_NAMES)
            raise NotImplementedError(f'{missing}: {_cls(leaf)} here while {n_cn} other layers carry a CNAttnProcessor -- the '
                                      f'executor drops the context tail on every layer or on none')
        if n_ref_on:
            for name, _, ref in rows:
                want = name.endswith('attn1.processor')
                have = ref is not None and bool(ref.enabled)
                if want != have:
                    what = f'{_cls(ref)}(enabled={bool(ref.enabled)})' if ref is not None else 'no reference processor'
                    raise NotImplementedError(f'{name}: {what} -- the executor stores / reads reference tokens on exactly the self-attention '
                                              f'layers (enabled on every attn1, on no attn2)')
        return rows

    def _attn_resolve(self):
        """Translate the current table (lazily, at every forward: the reference mutates the installed objects) and push the IP weights
        whose identity changed since the last push.  Host metadata only when nothing changed: no copy, no synchronisation."""
        table = self._attn_source.attn_processors if self._attn_source is not None else self._attn_own_table()
        if self._attn_source is not None and set(table) != set(self._attn_names()):       # (its ORDER is its own: weights are pushed by name)
            raise ValueError(f'the source module has {len(table)} attention processors, the engine {len(self._attn_names())}, under other '
                             f'names: they do not describe the same network')
        rows = self._attn_check(table)
        r = Resolved()
        first_ip = first_cn = None
        for name, leaf, ref in rows:
            c = _cls(leaf)
            if c in IP_NAMES:
                tok, sc = int(leaf.num_tokens), float(leaf.scale)
                if first_ip is None:
                    first_ip, r.ip_tokens, r.ip_scale = name, tok, sc
                elif tok != r.ip_tokens:
                    raise ValueError(f'{first_ip} has num_tokens={r.ip_tokens} but {name} has num_tokens={tok}: the executor takes one value for all layers')
                elif sc != r.ip_scale:
                    raise ValueError(f'{first_ip} has scale={r.ip_scale} but {name} has scale={sc}: the executor takes one value for all layers')
                r.ip_weights.append((name + '.to_k_ip.weight', leaf.to_k_ip.weight))
                r.ip_weights.append((name + '.to_v_ip.weight', leaf.to_v_ip.weight))
            elif c in CN_NAMES:
                tok = int(leaf.num_tokens)
                if first_cn is None:
                    first_cn, r.cn_tokens = name, tok
                elif tok != r.cn_tokens:
                    raise ValueError(f'{first_cn} has num_tokens={r.cn_tokens} but {name} has num_tokens={tok}: the executor takes one value for all layers')
            if ref is not None and ref.enabled:
                r.reference = True
        if r.ip_tokens < 0 or r.cn_tokens < 0:
            raise ValueError(f'num_tokens must not be negative ({first_ip or first_cn})')
        if r.ip_weights:
            if self._attn_pushed is None:
                self._attn_pushed = {}
            for pname, w in r.ip_weights:
                ident = _ident(w)
                if ident[1] is None or self._attn_pushed.get(pname) != ident:
                    self._attn_push(pname, w)
                    self._attn_pushed[pname] = ident
        return r
