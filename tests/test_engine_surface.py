"""The diffusers module surface of the engines that `mvedit_amd.dropin` puts on the reference's pipelines: the attention-processor table
(mvedit_amd/attn_processors.py), `parameters()` and its like, the shared table of an engine built from a torch module, the Zero123++ swap at
`prepare()`.  Host logic only, no GPU: the table is driven on a handle-free recorder, and -- with the reference tree present -- by the
reference's OWN code (joint_attn.py, ip_adapter.py, zero123plus.py), loaded from its files or cut out of them with `ast`, never copied."""
import ast
import importlib.util
import json
import os
import sys
import types

import pytest
import torch

import attn_standins as S
from mvedit_amd.attn_processors import AttnProcessorTable, EngineAttnProcessor, attn_processor_names, controlnet_attn_processor_names
from oracle import unet_oracle as U

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF, 'lib', 'models', 'architecture', 'joint_attn.py')), reason='reference tree not present')


class Recorder(AttnProcessorTable):
    """The table on an object without a native handle: pushes are recorded."""

    def __init__(self, cfg=U.SMALL, controlnet=False):
        self.cfg, self._attn_is_controlnet, self.pushed = cfg, controlnet, []
        self.config = types.SimpleNamespace(cross_attention_dim=cfg['cross_attention_dim'], block_out_channels=cfg['block_out_channels'])

    def _attn_names(self):
        return (controlnet_attn_processor_names if self._attn_is_controlnet else attn_processor_names)(self.cfg)

    def _attn_push(self, name, tensor):
        self.pushed.append((name, tensor))


# ------------------------------------------------------------------------------------------------------------------------ 1. names
def test_processor_names_follow_registration_order(lib):
    from mvedit_amd.unet import SD15_CONFIG, SDXL_CONFIG, UNet2DConditionEngine
    n15 = attn_processor_names(SD15_CONFIG)
    assert len(n15) == 32 and len(set(n15)) == 32
    assert n15[0] == 'down_blocks.0.attentions.0.transformer_blocks.0.attn1.processor'
    assert n15[1] == 'down_blocks.0.attentions.0.transformer_blocks.0.attn2.processor'
    assert all(n.startswith('down_blocks.') for n in n15[:12]) and all(n.startswith('up_blocks.') for n in n15[12:30])
    assert n15[30:] == [f'mid_block.attentions.0.transformer_blocks.0.attn{k}.processor' for k in (1, 2)]
    assert n15[12].startswith('up_blocks.1.') and n15[29].startswith('up_blocks.3.attentions.2.')     # up block 0 has no attention in SD-1.5
    nxl = attn_processor_names(SDXL_CONFIG)
    count = lambda p: sum(n.startswith(p) and n.endswith('attn1.processor') for n in nxl)
    assert len(nxl) == 140 and (count('down_blocks.'), count('up_blocks.'), count('mid_block.')) == (24, 36, 10)
    assert nxl[-1] == 'mid_block.attentions.0.transformer_blocks.9.attn2.processor'
    assert controlnet_attn_processor_names(SD15_CONFIG) == n15[:12] + n15[30:]
    # twice the executor's transformer-layer count: every transformer block plans one self- and one cross-attention
    for cfg in (SD15_CONFIG, SDXL_CONFIG, U.SMALL, U.TINY):
        eng = UNet2DConditionEngine(cfg, torch.float16, device='cpu')
        eng.plan(2, 16, 16, 77)
        assert sum(c == 'attention' for _, c, _, _ in eng.op_table()) == len(attn_processor_names(cfg)) == len(eng.attn_processors)
        assert list(eng.attn_processors) == attn_processor_names(cfg)


# ------------------------------------------------------------------------------------------------------------------------ 2. table semantics
def test_defaults_identity_and_key_mismatch():
    r = Recorder()
    names = attn_processor_names(U.SMALL)
    d = r.attn_processors
    assert list(d) == names and all(isinstance(v, EngineAttnProcessor) for v in d.values())
    assert len(list(torch.nn.ModuleList(d.values()).parameters())) == 0 and not r._attn_governs
    table = S.ip_table(U.SMALL, names)
    r.set_attn_processor(table)
    assert r._attn_governs and list(r.attn_processors) == names
    assert all(r.attn_processors[n] is table[n] for n in names)                   # the very objects
    one = S.AttnProcessor2_0()
    r.set_attn_processor(one)
    assert all(v is one for v in r.attn_processors.values())
    with pytest.raises(ValueError, match='number of processors 19 does not match the number of attention layers: 20'):
        r.set_attn_processor({n: one for n in names[1:]})
    with pytest.raises(ValueError, match="'bogus.processor' is not the name of an attention layer"):
        r.set_attn_processor({**{n: one for n in names[1:]}, 'bogus.processor': one})
    assert all(v is one for v in r.attn_processors.values())                      # a refused table leaves the old one


def test_translation_and_wrapper_transparency():
    names = attn_processor_names(U.SMALL)
    r = Recorder()
    r.set_attn_processor(S.ip_table(U.SMALL, names, num_tokens=16, scale=0.6))
    t = r._attn_resolve()
    assert (t.ip_tokens, t.ip_scale, t.reference, t.cn_tokens) == (16, 0.6, False, 0)
    # CrossImageAttnProcWrapper is transparent, around IP and around Reference(IP / plain) -- the nestings the reference can produce
    r2 = Recorder()
    r2.set_attn_processor(S.ip_table(U.SMALL, names, 16, 0.6, wrap=S.CrossImageAttnProcWrapper))
    t2 = r2._attn_resolve()
    assert (t2.ip_tokens, t2.ip_scale, t2.reference) == (16, 0.6, False)
    assert [n for n, _ in r2.pushed] == [n for n, _ in r.pushed] and len(r.pushed) == len(names)
    ref = lambda n, p: S.ReferenceOnlyAttnProc(p, enabled=n.endswith('attn1.processor'), name=n)
    r3 = Recorder()
    base = S.ip_table(U.SMALL, names, 4, 1.0)
    r3.set_attn_processor({n: S.CrossImageAttnProcWrapper(ref(n, base[n])) for n in names})
    t3 = r3._attn_resolve()
    assert (t3.ip_tokens, t3.reference) == (4, True)
    r4 = Recorder()
    r4.set_attn_processor({n: ref(n, S.AttnProcessor2_0()) for n in names})
    t4 = r4._attn_resolve()
    assert (t4.ip_tokens, t4.reference) == (0, True) and r4.pushed == []
    cn = Recorder(controlnet=True)
    cn.set_attn_processor(S.CNAttnProcessor())
    assert cn._attn_resolve().cn_tokens == 4
    cn.set_attn_processor(S.CNAttnProcessor(num_tokens=16))
    assert cn._attn_resolve().cn_tokens == 16
    cn.set_attn_processor(S.AttnProcessor2_0())
    assert cn._attn_resolve().cn_tokens == 0


def test_refusals_name_the_layer():
    names = attn_processor_names(U.SMALL)
    attn2 = [n for n in names if n.endswith('attn2.processor')]
    plain = S.AttnProcessor2_0
    r = Recorder()
    with pytest.raises(NotImplementedError, match=r'down_blocks\.0\.attentions\.0\.transformer_blocks\.0\.attn1\.processor: attention processor LoRAAttnProcessor'):
        r.set_attn_processor(S.LoRAAttnProcessor())
    half = S.ip_table(U.SMALL, names)
    for n in attn2[len(attn2) // 2:]:
        half[n] = plain()
    with pytest.raises(NotImplementedError, match=attn2[len(attn2) // 2].replace('.', r'\.') + ': AttnProcessor2_0'):
        r.set_attn_processor(half)
    on_attn1 = S.ip_table(U.SMALL, names)
    on_attn1[names[0]] = S.IPAttnProcessor(320, 768)
    with pytest.raises(NotImplementedError, match=names[0].replace('.', r'\.') + ': IPAttnProcessor on a self-attention'):
        r.set_attn_processor(on_attn1)
    with pytest.raises(NotImplementedError, match='CNAttnProcessor is a ControlNet processor'):
        r.set_attn_processor(S.CNAttnProcessor())
    # a reference processor enabled on attn2 / missing on an attn1
    with pytest.raises(NotImplementedError, match=names[1].replace('.', r'\.') + r': ReferenceOnlyAttnProc\(enabled=True\)'):
        r.set_attn_processor({n: S.ReferenceOnlyAttnProc(plain(), enabled=True, name=n) for n in names})
    some = {n: S.ReferenceOnlyAttnProc(plain(), enabled=n.endswith('attn1.processor'), name=n) for n in names}
    some[names[2]] = plain()
    with pytest.raises(NotImplementedError, match=names[2].replace('.', r'\.') + ': no reference processor'):
        r.set_attn_processor(some)
    # wrappers nested the other way round
    with pytest.raises(NotImplementedError, match='CrossImageAttnProcWrapper inside ReferenceOnlyAttnProc'):
        r.set_attn_processor({n: S.ReferenceOnlyAttnProc(S.CrossImageAttnProcWrapper(plain()), enabled=n.endswith('attn1.processor'), name=n) for n in names})
    assert not r._attn_governs                                                   # nothing was installed
    cn = Recorder(controlnet=True)
    with pytest.raises(NotImplementedError, match='IPAttnProcessor on a ControlNet engine'):
        cn.set_attn_processor(S.ip_table(U.SMALL, controlnet_attn_processor_names(U.SMALL)))
    mixed = {n: S.CNAttnProcessor() for n in controlnet_attn_processor_names(U.SMALL)}
    mixed[controlnet_attn_processor_names(U.SMALL)[3]] = plain()
    with pytest.raises(NotImplementedError, match='transformer_blocks.0.attn2.processor: AttnProcessor2_0 here while 7 other layers carry a CNAttnProcessor'):
        cn.set_attn_processor(mixed)
    # values that must agree across layers: at the forward (the reference mutates them after installing), naming both layers
    table = S.ip_table(U.SMALL, names, 16, 0.6)
    r.set_attn_processor(table)
    table[attn2[3]].scale = 0.5
    with pytest.raises(ValueError, match=f'{attn2[0]} has scale=0.6 but {attn2[3]} has scale=0.5'.replace('.', r'\.')):
        r._attn_resolve()
    table[attn2[3]].scale, table[attn2[2]].num_tokens = 0.6, 4
    with pytest.raises(ValueError, match=f'{attn2[0]} has num_tokens=16 but {attn2[2]} has num_tokens=4'.replace('.', r'\.')):
        r._attn_resolve()


def test_lazy_translation_and_weight_pushes():
    names = attn_processor_names(U.SMALL)
    attn2 = [n for n in names if n.endswith('attn2.processor')]
    table = S.ip_table(U.SMALL, names, 16, 1.0)
    r = Recorder()
    r.set_attn_processor(table)
    assert r.pushed == []                                                        # nothing happens before a forward
    assert r._attn_resolve().ip_scale == 1.0
    want = [f'{n}.{kv}.weight' for n in attn2 for kv in ('to_k_ip', 'to_v_ip')]
    assert [n for n, _ in r.pushed] == want
    assert all(t is table[n.rsplit('.', 2)[0]].get_submodule(n.split('.')[-2]).weight for n, t in r.pushed)
    for p in table.values():                                                     # IPAdapter.set_scale
        if isinstance(p, S.IPAttnProcessor):
            p.scale = 0.3
    assert r._attn_resolve().ip_scale == 0.3 and len(r.pushed) == len(want)     # a second forward pushes nothing
    # load_state_dict into the installed objects (ip_adapter.py:61-62): every weight's version moves -> exactly one re-push per weight
    ck = S.ip_checkpoint({k: v * 2 for k, v in U.make_ip_state_dict(U.SMALL).items()}, names)
    torch.nn.ModuleList(r.attn_processors.values()).load_state_dict(ck)
    del r.pushed[:]
    r._attn_resolve()
    assert [n for n, _ in r.pushed] == want
    r._attn_resolve()
    assert len(r.pushed) == len(want)
    with torch.no_grad():
        table[attn2[1]].to_v_ip.weight.mul_(0.5)                                 # one weight edited in place
    r._attn_resolve()
    assert [n for n, _ in r.pushed[len(want):]] == [f'{attn2[1]}.to_v_ip.weight']
    table[attn2[0]].to_k_ip.weight = torch.nn.Parameter(table[attn2[0]].to_k_ip.weight.detach().clone())      # replaced (.to(dtype))
    r._attn_resolve()
    assert [n for n, _ in r.pushed[len(want) + 1:]] == [f'{attn2[0]}.to_k_ip.weight']


def test_module_surface_of_every_swapped_engine(lib):
    from mvedit_amd.controlnet import ControlNetEngine, MultiControlNetEngine
    from mvedit_amd.image_enhancer import SRVGGNetCompactEngine
    from mvedit_amd.segmentor import TracerUniversalB7Engine
    from mvedit_amd.unet import UNet2DConditionEngine
    from mvedit_amd.vae import AutoencoderKLEngine
    cn = ControlNetEngine(U.TINY, torch.bfloat16, device='cpu')
    engines = [UNet2DConditionEngine(U.TINY, torch.float16, device='cpu'), cn, MultiControlNetEngine([cn]), AutoencoderKLEngine(None, torch.float16, 'cpu'),
               SRVGGNetCompactEngine(num_feat=16, num_conv=2, dtype=torch.bfloat16, device='cpu'), TracerUniversalB7Engine(torch_dtype='float16', device='cpu')]
    for e in engines:
        p = next(e.parameters())
        assert torch.is_tensor(p) and p.dtype == e.dtype and p.device == e.device, type(e).__name__
    for e in engines[:3]:
        assert e.set_use_memory_efficient_attention_xformers(True) is None
    multi = MultiControlNetEngine([ControlNetEngine(U.TINY, torch.float16, device='cpu') for _ in range(2)])
    proc = S.CNAttnProcessor()
    multi.set_attn_processor(proc)
    assert all(v is proc for net in multi.nets for v in net.attn_processors.values()) and all(net._attn_governs for net in multi.nets)


def test_a_governing_table_decides_about_the_kwargs(lib):
    """Once set, the table governs: reference kwargs without a reference processor and an IP processor on a short context are ValueErrors,
    raised before anything native runs (a CPU-device engine cannot launch)."""
    from mvedit_amd.unet import UNet2DConditionEngine
    eng = UNet2DConditionEngine(U.TINY, torch.float16, device='cpu')
    names = attn_processor_names(U.TINY)
    eng.set_attn_processor(S.AttnProcessor2_0())
    with pytest.raises(ValueError, match="mode='w'"):
        eng._set_attention(dict(mode='w', ref_dict={}), 2, 16, 16, 77)
    pushed = []
    eng._attn_push = lambda name, t: pushed.append(name)
    eng.set_attn_processor(S.ip_table(U.TINY, names, 16))
    with pytest.raises(ValueError, match='take the last 16 rows of encoder_hidden_states, which has 16'):
        eng._set_attention(None, 2, 16, 16, 16)
    assert len(pushed) == len(names)


def test_context_tail_is_a_plan_option(lib):
    """mve_unet_set_context_tail (plan-time only, no GPU): one more op (the strided gather of the text rows), fewer cross-attention flops, plans of
    either setting cached side by side; n >= ctx_len and the combination with ip tokens are refused at plan time; other executors refuse it."""
    from mvedit_amd.controlnet import ControlNetEngine
    from mvedit_amd.unet import UNet2DConditionEngine
    from mvedit_amd.vae import AutoencoderKLEngine
    tail = lib.raw('mve_unet_set_context_tail')
    cn = ControlNetEngine(U.SMALL, torch.float16, device='cpu')
    a = cn.plan(2, 16, 16, 93)
    assert tail(cn._h, 4) == 0 and tail(cn._h, -1) == 4
    b = cn.plan(2, 16, 16, 93)
    assert b['n_ops'] == a['n_ops'] + 1 and [lab for *_, lab in cn.op_table() if 'tail' in lab] == ['ctx rows without the tail']
    assert 0 < b['flops']['attention'] < a['flops']['attention'] and b['flops']['conv3x3'] == a['flops']['conv3x3']
    ref = cn.plan(2, 16, 16, 89)                      # the dense 89-row context of the comparison: same work without the gather
    assert tail(cn._h, 0) == 4
    dense = cn.plan(2, 16, 16, 89)
    assert b['flops'] == dense['flops'] and b['n_ops'] == dense['n_ops'] + 1 and ref['n_ops'] == dense['n_ops'] + 1
    assert cn.plan(2, 16, 16, 93) == a
    for n in (93, 200):
        tail(cn._h, n)
        with pytest.raises(lib.MveError, match=f'cannot ignore the last {n} rows of a context of 93 rows'):
            cn.plan(2, 16, 16, 93)
    tail(cn._h, 0)
    unet = UNet2DConditionEngine(U.SMALL, torch.float16, device='cpu')
    tail(unet._h, 4)
    lib.call('mve_unet_set_attention', unet._h, 16, 1.0, 0, 0, 0, 0, None, 0)
    with pytest.raises(lib.MveError, match='not combined with ip tokens'):
        unet.plan(2, 16, 16, 93)
    with pytest.raises(lib.MveError):
        lib.call('mve_unet_set_context_tail', AutoencoderKLEngine(None, torch.float16, 'cpu').decoder._h, 1)


# ------------------------------------------------------------------------------------------------------------------------ 3. the reference's own code
def _load(rel, name):
    sys.dont_write_bytecode = True           # never write __pycache__ into the reference tree
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cut(rel, wanted, ns):
    """Execute the named top-level classes / the named methods of a class (`Class.method`) of a reference file in `ns`."""
    tree = ast.parse(open(os.path.join(REF, rel)).read())
    for node in tree.body:
        if isinstance(node, ast.ClassDef):
            if node.name in wanted:
                exec(compile(ast.Module([node], []), rel, 'exec'), ns)
            for fn in node.body:
                if isinstance(fn, ast.FunctionDef) and f'{node.name}.{fn.name}' in wanted:
                    exec(compile(ast.Module([fn], []), rel, 'exec'), ns)
    return ns


@needs_ref
def test_reference_cross_image_wrapper_round_trip():
    ja = _load('lib/models/architecture/joint_attn.py', 'ref_joint_attn')
    r = Recorder()
    names = attn_processor_names(U.SMALL)
    table = S.ip_table(U.SMALL, names, 16, 0.7)
    r.set_attn_processor(table)
    ja.apply_cross_image_attn_proc(r)
    assert all(type(v).__name__ == 'CrossImageAttnProcWrapper' and v.base_attn_proc is table[n] for n, v in r.attn_processors.items())
    t = r._attn_resolve()
    assert (t.ip_tokens, t.ip_scale) == (16, 0.7)
    ja.remove_cross_image_attn_proc(r)
    assert all(r.attn_processors[n] is table[n] for n in names)
    fresh = Recorder()                                                            # on the defaults, as MVEdit3DPipeline.__call__ meets them
    before = fresh.attn_processors
    ja.apply_cross_image_attn_proc(fresh)
    assert fresh._attn_resolve().ip_tokens == 0
    ja.remove_cross_image_attn_proc(fresh)
    assert all(fresh.attn_processors[n] is before[n] for n in names)


@needs_ref
def test_reference_ip_adapter_installs_loads_and_scales():
    ap = _load('lib/models/architecture/ip_adapter/attention_processor.py', 'ref_ip_attention_processor')

    class MultiControlNetModel:              # diffusers name, stubbed: the engines are not instances of it
        pass
    ns = dict(torch=torch, MultiControlNetModel=MultiControlNetModel, IPAttnProcessor=ap.IPAttnProcessor2_0, AttnProcessor=ap.AttnProcessor2_0,
              CNAttnProcessor=ap.CNAttnProcessor2_0)
    _cut('lib/models/architecture/ip_adapter/ip_adapter.py', {'IPAdapter.set_ip_adapter', 'IPAdapter.set_scale'}, ns)
    unet, cn = Recorder(), Recorder(controlnet=True)
    multi = types.SimpleNamespace(nets=[cn], set_attn_processor=lambda p: [n.set_attn_processor(p) for n in [cn]])
    me = types.SimpleNamespace(pipe=types.SimpleNamespace(unet=unet, controlnet=multi), num_tokens=16, device='cpu', dtype=torch.float32)
    ns['set_ip_adapter'](me)
    names = attn_processor_names(U.SMALL)
    assert [type(v).__name__ for v in unet.attn_processors.values()] == ['AttnProcessor2_0', 'IPAttnProcessor2_0'] * (len(names) // 2)
    assert cn._attn_resolve().cn_tokens == 4                                     # CNAttnProcessor() keeps its default under the 16-token adapter
    ip_sd = U.make_ip_state_dict(U.SMALL)
    ip_layers = torch.nn.ModuleList(unet.attn_processors.values())              # ip_adapter.py:61-62
    ip_layers.load_state_dict(S.ip_checkpoint(ip_sd, names))
    t = unet._attn_resolve()
    assert (t.ip_tokens, t.ip_scale) == (16, 1.0) and len(unet.pushed) == len(names)
    for pname, w in unet.pushed:                                                 # the table order put every weight on its own layer
        assert torch.equal(w.detach(), ip_sd[pname]), pname
    ns['set_scale'](me, 0.45)
    assert unet._attn_resolve().ip_scale == 0.45 and len(unet.pushed) == len(names)


@needs_ref
def test_reference_zero123_wrappers_construct_on_the_table():
    import typing
    ns = dict(torch=torch, Any=typing.Any, Optional=typing.Optional, Attention=object, UNet2DConditionModel=object, DDPMScheduler=object,
              EulerAncestralDiscreteScheduler=object, AttnProcessor=S.AttnProcessor2_0, AttnProcessor2_0=S.AttnProcessor2_0,
              XFormersAttnProcessor=S.AttnProcessor2_0, is_xformers_available=lambda: False, diffusers=types.SimpleNamespace(ControlNetModel=object))
    _cut('lib/pipelines/zero123plus.py', {'ReferenceOnlyAttnProc', 'RefOnlyNoisedUNet', 'DepthControlUNet'}, ns)
    unet, cn = Recorder(), Recorder(controlnet=True)
    wrapped = ns['RefOnlyNoisedUNet'](unet, None, None)
    names = attn_processor_names(U.SMALL)
    procs = unet.attn_processors
    assert all(type(procs[n]).__name__ == 'ReferenceOnlyAttnProc' and procs[n].enabled == n.endswith('attn1.processor') and procs[n].name == n for n in names)
    t = unet._attn_resolve()
    assert t.reference and t.ip_tokens == 0
    assert wrapped.unet is unet and wrapped.config is unet.config               # the wrapper's __getattr__ falls through to the engine
    depth = ns['DepthControlUNet'](wrapped, cn, 0.8)
    assert depth.controlnet is cn and cn._attn_governs and cn._attn_resolve().cn_tokens == 0


# ------------------------------------------------------------------------------------------------------------------------ 4. drop-in wiring
class TableModule(torch.nn.Module):
    """A loaded diffusers model as far as the drop-in reads it: parameters, a reported device, its own processor table."""

    def __init__(self, names=(), device='cpu'):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))
        self.reported = torch.device(device)
        self.table = {n: S.AttnProcessor2_0() for n in names}

    def parameters(self, recurse=True):
        for p in super().parameters(recurse):
            yield types.SimpleNamespace(device=self.reported, dtype=p.dtype)

    @property
    def attn_processors(self):
        return dict(self.table)

    def set_attn_processor(self, processor):
        self.table = dict(processor) if isinstance(processor, dict) else {n: processor for n in self.table}


ZERO123_SKELETON = '''
import torch
class RefOnlyNoisedUNet(torch.nn.Module):
    def __init__(self, unet, train_sched, val_sched):
        super().__init__()
        self.unet = unet
class DepthControlUNet(torch.nn.Module):
    def __init__(self, unet, controlnet=None, conditioning_scale=1.0):
        super().__init__()
        self.unet, self.controlnet = unet, controlnet
class Zero123PlusPipeline:
    def __init__(self, vae=None, text_encoder=None, tokenizer=None, unet=None, scheduler=None, vision_encoder=None, feature_extractor_clip=None,
                 feature_extractor_vae=None, ramping_coefficients=None, safety_checker=None):
        self.vae, self.unet, self.scheduler = vae, unet, scheduler
    def prepare(self):
        if not isinstance(self.unet, (RefOnlyNoisedUNet, DepthControlUNet)):
            self.unet = RefOnlyNoisedUNet(self.unet, None, self.scheduler).eval()
    def add_controlnet(self, controlnet=None, conditioning_scale=1.0):
        self.prepare()
        self.unet = DepthControlUNet(self.unet, controlnet, conditioning_scale)
'''


@pytest.fixture()
def skeleton(tmp_path, monkeypatch):
    from test_dropin import SKELETON
    files = dict(SKELETON)
    files['lib/pipelines/zero123plus.py'] = ZERO123_SKELETON
    for rel, src in files.items():
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(src)
    monkeypatch.syspath_prepend(str(tmp_path))
    for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
        monkeypatch.delitem(sys.modules, k)
    from mvedit_amd import dropin
    yield dropin
    dropin.uninstall()
    for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
        sys.modules.pop(k, None)


def test_engine_and_source_module_share_one_table(lib, skeleton, monkeypatch):
    dropin = skeleton
    from mvedit_amd.controlnet import ControlNetEngine, MultiControlNetEngine
    from mvedit_amd.unet import UNet2DConditionEngine
    monkeypatch.setitem(dropin.MAKERS, 'unet', lambda m: UNet2DConditionEngine(U.TINY, torch.float16, device='cpu'))
    monkeypatch.setitem(dropin.MAKERS, 'controlnet', lambda m: MultiControlNetEngine([ControlNetEngine(U.TINY, torch.float16, device='cpu') for _ in m.nets]))
    names = attn_processor_names(U.TINY)
    module = TableModule(names, 'cuda:0')
    eng = dropin.engine_for('unet', module)
    assert eng._attn_governs and list(eng.attn_processors) == names
    assert all(eng.attn_processors[n] is module.table[n] for n in names)
    table = S.ip_table(U.TINY, names, 16, 0.5)
    module.set_attn_processor(table)                                            # the runner talks to the module ...
    assert all(eng.attn_processors[n] is table[n] for n in names)
    pushed = []
    eng._attn_push = lambda name, t: pushed.append(name)
    t = eng._attn_resolve()
    assert (t.ip_tokens, t.ip_scale) == (16, 0.5) and len(pushed) == len(names)
    plain = S.AttnProcessor2_0()
    eng.set_attn_processor(plain)                                               # ... and the pipeline to the engine
    assert all(v is plain for v in module.table.values()) and eng._attn_resolve().ip_tokens == 0
    module.set_attn_processor(S.LoRAAttnProcessor())                            # what the module holds is translated at the forward: refused there
    with pytest.raises(NotImplementedError, match='LoRAAttnProcessor'):
        eng._attn_resolve()
    cn_names = controlnet_attn_processor_names(U.TINY)
    cmod = TableModule((), 'cuda:0')
    cmod.nets = torch.nn.ModuleList([TableModule(cn_names, 'cuda:0'), TableModule(cn_names, 'cuda:0')])
    multi = dropin.engine_for('controlnet', cmod)
    cmod.nets[1].set_attn_processor(S.CNAttnProcessor())                        # unload_ip_adapter / set_ip_adapter reach each net through its module
    assert [n._attn_resolve().cn_tokens for n in multi.nets] == [0, 4]
    multi.set_attn_processor(S.CNAttnProcessor(num_tokens=16))
    assert [type(p).__name__ for m in cmod.nets for p in m.table.values()] == ['CNAttnProcessor'] * (2 * len(cn_names))
    # engines are built from weights on the accelerator only
    with pytest.raises(RuntimeError, match='parameters are on the CPU'):
        dropin.make_unet(TableModule(names, 'cpu'))


class FakeEngine:
    def __init__(self, kind, src):
        self.kind, self.src = kind, src


def test_zero123_is_swapped_at_prepare_on_the_accelerator(lib, skeleton, monkeypatch):
    dropin = skeleton
    built = []

    def maker(kind):
        def make(m):
            built.append(kind)
            return FakeEngine(kind, m)
        return make
    monkeypatch.setattr(dropin, 'MAKERS', {k: maker(k) for k in dropin.SWAPPED_ATTRS})
    dropin.install()
    from lib.pipelines import Zero123PlusPipeline
    unet, vae, cnet = TableModule(), TableModule(), TableModule()
    pipe = Zero123PlusPipeline(vae=vae, unet=unet, scheduler='sch')
    assert pipe.unet is unet and pipe.vae is vae and built == []               # from_pretrained builds on the CPU: nothing is swapped at __init__
    pipe.prepare()
    assert type(pipe.unet).__name__ == 'RefOnlyNoisedUNet' and pipe.unet.unet is unet and pipe.vae is vae and built == []      # still on the CPU
    for m in (unet, vae):
        m.reported = torch.device('cuda:0')                                     # pipe.to(device)
    pipe.prepare()
    wrapper = pipe.unet
    assert isinstance(wrapper.unet, FakeEngine) and wrapper.unet.src is unet and wrapper._modules['unet'] is unet
    assert isinstance(pipe.vae, FakeEngine) and sorted(built) == ['unet', 'vae']
    eng = wrapper.unet
    pipe.prepare()                                                              # idempotent
    assert pipe.unet is wrapper and wrapper.unet is eng and sorted(built) == ['unet', 'vae']
    # the normal pipeline: a shallow copy that adds a ControlNet loaded on the CPU, moved later (lib/apis/adapter3d.py:392-396)
    from copy import copy
    pipe2 = copy(pipe)
    pipe2.unet, pipe2.vae = unet, vae
    pipe2.add_controlnet(cnet)
    depth = pipe2.unet
    assert type(depth).__name__ == 'DepthControlUNet' and depth.controlnet is cnet and depth.unet.unet is eng     # the engine cached on the module
    cnet.reported = torch.device('cuda:0')
    pipe2.prepare()
    assert isinstance(depth.controlnet, FakeEngine) and depth.controlnet.src is cnet and depth._modules['controlnet'] is cnet
    assert sorted(built) == ['controlnet', 'unet', 'vae']
    dropin.uninstall()
    assert wrapper.unet is unet and depth.controlnet is cnet and depth.unet.unet is unet and pipe.vae is vae and pipe2.vae is vae
    assert 'unet' not in wrapper.__dict__ and 'controlnet' not in depth.__dict__
    p3 = Zero123PlusPipeline(vae=vae, unet=unet)
    p3.prepare()
    assert p3.unet.unet is unet                                                 # the class is the reference's again


# ------------------------------------------------------------------------------------------------------------------------ 5. surface coverage
NAMES = os.path.join(HERE, 'golden', 'dropin_surface_names.json')


def _generator():
    spec = importlib.util.spec_from_file_location('make_dropin_surface_names', os.path.join(HERE, 'golden', 'make_dropin_surface_names.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_name_the_reference_reads_exists_on_the_engines(lib):
    from mvedit_amd.controlnet import ControlNetEngine, MultiControlNetEngine
    from mvedit_amd.image_enhancer import SRVGGNetCompactEngine
    from mvedit_amd.mesh_ops import MeshRenderer
    from mvedit_amd.segmentor import TracerUniversalB7Engine
    from mvedit_amd.unet import UNet2DConditionEngine
    from mvedit_amd.vae import AutoencoderKLEngine
    cn = ControlNetEngine(U.TINY, torch.float16, device='cpu')
    stand_ins = dict(unet=[UNet2DConditionEngine(U.TINY, torch.float16, device='cpu')], controlnet=[MultiControlNetEngine([cn])],
                     vae=[AutoencoderKLEngine(None, torch.float16, 'cpu')], image_enhancer=[SRVGGNetCompactEngine(num_feat=16, num_conv=2, device='cpu')],
                     segmentation=[TracerUniversalB7Engine(torch_dtype='float16', device='cpu')], mesh_renderer=[MeshRenderer()])
    listed = json.load(open(NAMES))
    assert set(stand_ins) == {k for k in listed if not k.startswith('_')}
    assert {'attn_processors', 'set_attn_processor', 'dtype', 'config'} <= set(listed['unet']['names']) and 'parameters' in listed['image_enhancer']['names']
    for member, entry in listed.items():
        if member.startswith('_'):
            continue
        assert all(isinstance(r, str) and r for r in entry['excluded'].values())
        for name in entry['names']:
            if name not in entry['excluded']:
                assert all(hasattr(e, name) for e in stand_ins[member]), f'{member}.{name}'
    # the single-net engine carries what IPAdapter.set_ip_adapter calls on it too
    assert hasattr(cn, 'set_attn_processor')


@needs_ref
def test_the_committed_name_list_is_what_the_generator_reads():
    assert _generator().surface_names(REF) == json.load(open(NAMES))
