"""`mvedit_amd.nvdiffrast.torch` without a GPU: the public surface (nvdiffrast's names, parameter names and defaults), the refusals, the call
shapes the reference's base_mesh_renderer.py uses (tests/golden/nvdiffrast_ref_calls.json, read out of the reference tree with `ast`:
`python tests/test_nvdr_facade_cpu.py <reference tree>` rewrites it), the drop-in seeding, and the argument checks of the new C entry points."""
import ast
import ctypes
import inspect
import json
import os
import sys

import pytest
import torch

CALLS_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nvdiffrast_ref_calls.json')
RENDERER = 'lib/models/decoders/mesh_renderer/base_mesh_renderer.py'
E = inspect.Parameter.empty
SIGNATURES = {
    'RasterizeCudaContext': [('device', None)],
    'RasterizeGLContext': [('output_db', True), ('mode', 'automatic'), ('device', None)],
    'rasterize': [('glctx', E), ('pos', E), ('tri', E), ('resolution', E), ('ranges', None), ('grad_db', True)],
    'interpolate': [('attr', E), ('rast', E), ('tri', E), ('rast_db', None), ('diff_attrs', None)],
    'texture': [('tex', E), ('uv', E), ('uv_da', None), ('mip_level_bias', None), ('mip', None), ('filter_mode', 'auto'), ('boundary_mode', 'wrap'),
                ('max_mip_level', None)],
    'antialias': [('color', E), ('rast', E), ('pos', E), ('tri', E), ('topology_hash', None), ('pos_gradient_boost', 1.0)],
    'antialias_construct_topology_hash': [('tri', E)],
    'get_log_level': [],
    'set_log_level': [('level', E)],
}


def test_public_names_and_signatures(lib):
    import copy
    import mvedit_amd.nvdiffrast.torch as dr
    for name, want in SIGNATURES.items():
        params = list(inspect.signature(getattr(dr, name)).parameters.values())
        assert [(p.name, p.default) for p in params] == want, name
        assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in params), name
    assert set(SIGNATURES) <= set(dr.__all__)
    # contexts: plain objects the reference copies along with its renderer (lib/apis/adapter3d.py:1237)
    for ctx in (dr.RasterizeCudaContext(), dr.RasterizeCudaContext(device='cuda:0'), dr.RasterizeGLContext(), dr.RasterizeGLContext(output_db=False)):
        c = copy.deepcopy(ctx)
        assert type(c) is type(ctx) and vars(c) == vars(ctx)
    old = dr.get_log_level()
    dr.set_log_level(2)
    assert dr.get_log_level() == 2
    dr.set_log_level(old)


def test_everything_not_built_raises_not_implemented(lib):
    """Each refusal names the argument and happens before any launch (CPU tensors here: a launch would fail differently)."""
    import mvedit_amd.nvdiffrast.torch as dr
    ctx = dr.RasterizeCudaContext()
    pos, tri = torch.zeros(1, 3, 4), torch.zeros(1, 3, dtype=torch.int32)
    rast, color = torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 3)
    tex, uv, uv_da = torch.zeros(1, 8, 8, 3), torch.zeros(1, 4, 4, 2), torch.zeros(1, 4, 4, 4)
    cases = [
        ('ranges', lambda: dr.rasterize(ctx, pos, tri, (4, 4), ranges=torch.zeros(1, 2, dtype=torch.int32))),
        ('pos', lambda: dr.rasterize(ctx, pos[0], tri, (4, 4))),                                   # 2-D pos: range mode
        ('CPU', lambda: dr.rasterize(ctx, pos, tri, (4, 4))),
        ('attr', lambda: dr.interpolate(torch.zeros(3, 2), rast, tri)),                            # 2-D attr: range mode
        ('CPU', lambda: dr.interpolate(torch.zeros(1, 3, 2), rast, tri)),
        ('mip_level_bias', lambda: dr.texture(tex, uv, uv_da, mip_level_bias=torch.zeros(1, 4, 4))),
        ('mip=', lambda: dr.texture(tex, uv, uv_da, mip=[tex])),
        ('boundary_mode', lambda: dr.texture(tex, uv, boundary_mode='clamp')),
        ('boundary_mode', lambda: dr.texture(tex, uv, boundary_mode='zero')),
        ('boundary_mode', lambda: dr.texture(torch.zeros(1, 6, 8, 8, 3), torch.zeros(1, 4, 4, 3), boundary_mode='cube')),
        ('cube', lambda: dr.texture(torch.zeros(1, 6, 8, 8, 3), torch.zeros(1, 4, 4, 3))),
        ('filter_mode', lambda: dr.texture(tex, uv, filter_mode='nearest')),
        ('filter_mode', lambda: dr.texture(tex, uv, uv_da, filter_mode='linear-mipmap-nearest')),
        ('CPU', lambda: dr.texture(tex, uv)),
        ('CPU', lambda: dr.texture(tex, uv, uv_da)),
        ('pos', lambda: dr.antialias(color, rast, pos[0], tri)),
        ('CPU', lambda: dr.antialias(color, rast, pos, tri)),
        ('CPU', lambda: dr.antialias_construct_topology_hash(tri)),
    ]
    for word, call in cases:
        with pytest.raises(NotImplementedError, match=word):
            call()
    assert not hasattr(dr, 'texture_construct_mip')             # goes with mip=, which is refused


# ------------------------------------------------------------------------------------------------ the reference's call shapes
def _reference_calls(ref):
    """Every `dr.<name>(...)` call of the reference's base_mesh_renderer.py: name, line, number of positional arguments, keyword names."""
    tree = ast.parse(open(os.path.join(ref, RENDERER)).read())
    calls = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name) and node.func.value.id == 'dr':
            calls.append(dict(name=node.func.attr, line=node.lineno, positional=len(node.args), keywords=[k.arg for k in node.keywords]))
    imports = [a.name + (' as ' + a.asname if a.asname else '') for n in tree.body if isinstance(n, ast.Import) for a in n.names if 'nvdiffrast' in a.name]
    return dict(file=RENDERER, imports=imports, calls=sorted(calls, key=lambda c: (c['line'], c['name'])))


def test_every_call_shape_of_the_reference_binds(lib):
    import mvedit_amd.nvdiffrast.torch as dr
    r = json.load(open(CALLS_GOLD))
    assert r['imports'] == ['nvdiffrast.torch as dr']
    assert len(r['calls']) >= 30 and {c['name'] for c in r['calls']} >= {'RasterizeCudaContext', 'RasterizeGLContext', 'rasterize', 'interpolate',
                                                                        'texture', 'antialias'}
    for c in r['calls']:
        fn = getattr(dr, c['name'], None)
        assert fn is not None, c
        inspect.signature(fn).bind(*([None] * c['positional']), **{k: None for k in c['keywords']})        # raises TypeError on a mismatch


# ------------------------------------------------------------------------------------------------ drop-in
SKELETON = {
    'lib/__init__.py': '', 'lib/models/__init__.py': '', 'lib/models/decoders/__init__.py': '', 'lib/models/decoders/mesh_renderer/__init__.py': '',
    'lib/models/decoders/mesh_renderer/base_mesh_renderer.py': (
        'import nvdiffrast.torch as dr\n\n\nclass MeshRenderer:\n    def __init__(self, opengl=False):\n'
        '        self.glctx = dr.RasterizeGLContext() if opengl else dr.RasterizeCudaContext()\n'),
}


@pytest.fixture()
def skeleton(tmp_path, monkeypatch):
    for rel, src in SKELETON.items():
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(src)
    monkeypatch.syspath_prepend(str(tmp_path))
    for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.') or k == 'nvdiffrast' or k.startswith('nvdiffrast.')]:
        monkeypatch.delitem(sys.modules, k)
    from mvedit_amd import dropin
    yield dropin
    dropin.uninstall()
    for k in [k for k in sys.modules if k == 'lib' or k.startswith('lib.')]:
        sys.modules.pop(k, None)


def test_install_seeds_nvdiffrast(lib, skeleton):
    dropin = skeleton
    import mvedit_amd.nvdiffrast
    import mvedit_amd.nvdiffrast.torch as facade
    with pytest.raises(ImportError):
        import nvdiffrast.torch  # noqa: F401
    dropin.install()
    import nvdiffrast.torch as dr
    assert dr is facade and sys.modules['nvdiffrast'] is mvedit_amd.nvdiffrast
    import lib.models.decoders.mesh_renderer.base_mesh_renderer as B
    assert B.dr is facade
    assert isinstance(B.MeshRenderer().glctx, facade.RasterizeCudaContext) and isinstance(B.MeshRenderer(opengl=True).glctx, facade.RasterizeGLContext)
    dropin.uninstall()
    assert 'nvdiffrast' not in sys.modules and 'nvdiffrast.torch' not in sys.modules


def test_late_install_rebinds_dr(lib, skeleton, monkeypatch):
    """base_mesh_renderer imported before install() (over some other `nvdiffrast`): `dr` is rebound, and restored by uninstall()."""
    dropin = skeleton
    import mvedit_amd.nvdiffrast.torch as facade
    pkg, other = type(sys)('nvdiffrast'), type(sys)('nvdiffrast.torch')
    pkg.__path__, pkg.torch = [], other
    other.RasterizeCudaContext = lambda *a, **k: 'cuda-only'
    monkeypatch.setitem(sys.modules, 'nvdiffrast', pkg)
    monkeypatch.setitem(sys.modules, 'nvdiffrast.torch', other)
    import lib.models.decoders.mesh_renderer.base_mesh_renderer as B
    assert B.dr is other and B.MeshRenderer().glctx == 'cuda-only'
    dropin.install()
    assert B.dr is facade and isinstance(B.MeshRenderer().glctx, facade.RasterizeCudaContext)
    dropin.uninstall()
    assert B.dr is other and sys.modules['nvdiffrast.torch'] is other and sys.modules['nvdiffrast'] is pkg


# ------------------------------------------------------------------------------------------------ C entry points
def test_new_entry_points_reject_bad_arguments(lib):
    """MVE_ERR_ARG (-1) with a message, before any launch; empty problems are MVE_OK without one."""
    p = ctypes.c_void_p(64)            # a non-null address that is never dereferenced: every case fails its check first
    tg, ida, rdb = lib.raw('mve_texture_grad_uv'), lib.raw('mve_interpolate_da_backward'), lib.raw('mve_rasterize_db_backward')
    assert tg(None, None, 1, 8, 8, 3, 0, None, None, None, 0, 4, 4, None, None, None) == 0                       # n == 0
    assert tg(None, p, 1, 8, 8, 3, 3, p, p, p, 1, 4, 4, p, p, None) == -1 and 'null' in lib.last_error()          # no texture
    assert tg(p, p, 1, 8, 8, 3, 3, p, p, p, 1, 4, 4, None, None, None) == -1                                      # no output at all
    assert tg(p, p, 3, 8, 8, 3, 3, p, p, p, 2, 4, 4, p, p, None) == -1 and 'texture shape' in lib.last_error()    # 3 textures, 2 images
    assert tg(p, p, 1, 8, 8, 0, 3, p, p, p, 1, 4, 4, p, p, None) == -1                                            # no channels
    assert tg(p, None, 1, 8, 8, 3, 0, p, None, p, 1, 4, 4, p, p, None) == -1 and 'needs uv_da' in lib.last_error()
    assert tg(p, None, 1, 8, 8, 3, 3, p, p, p, 1, 4, 4, p, p, None) == -1 and 'level stack' in lib.last_error()   # mip mode without mips
    assert tg(p, p, 1, 12, 12, 3, 3, p, p, p, 1, 4, 4, p, p, None) == -1 and 'odd extent' in lib.last_error()     # 12 -> 6 -> 3 -> odd
    assert tg(p, p, 1, 8, 8, 3, 31, p, p, p, 1, 4, 4, p, p, None) == -1
    assert ida(None, 1, 3, 2, None, None, 0, 16, None, 1, None, None, None, None) == 0                            # B == 0
    assert ida(None, 1, 3, 2, p, p, 1, 16, p, 1, p, p, p, None) == -1 and 'null' in lib.last_error()
    assert ida(p, 1, 3, 2, p, p, 1, 16, p, 1, p, None, None, None) == -1                                          # no output at all
    assert ida(p, 3, 3, 2, p, p, 2, 16, p, 1, p, p, p, None) == -1 and 'attribute batch' in lib.last_error()
    assert rdb(None, 0, 3, None, 1, None, 4, 4, None, None, None, None) == 0                                      # B == 0
    assert rdb(None, 1, 3, p, 1, p, 4, 4, p, p, p, None) == -1 and 'null' in lib.last_error()
    assert rdb(p, 1, 3, p, 1, p, 4, 4, p, None, None, None) == -1                                                 # no output at all
    assert rdb(p, 1, 0, p, 1, p, 4, 4, p, p, p, None) == -1 and 'bad mesh' in lib.last_error()


if __name__ == '__main__':
    with open(CALLS_GOLD, 'w') as f:
        json.dump(_reference_calls(sys.argv[1]), f, indent=1)
        f.write('\n')
    print('wrote', CALLS_GOLD)
