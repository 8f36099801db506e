"""Writes tests/golden/dropin_surface_names.json: the attribute NAMES the reference reads off the six pipeline members that
`mvedit_amd.dropin` replaces with engines (unet, controlnet, vae, image_enhancer, segmentation, mesh_renderer).

The reference's sources are read with `ast` only -- nothing of them is executed or copied; the file holds names, and for the names that belong to
the training stack or to code paths the drop-in does not serve, the reason they are excluded from the surface test
(tests/test_engine_surface.py::test_every_name_the_reference_reads_exists_on_the_engines).

Sources: lib/pipelines/*.py, lib/apis/adapter3d.py, lib/models/architecture/ip_adapter/ip_adapter.py, lib/models/architecture/joint_attn.py and the
RefOnly* / DepthControl* classes of lib/models/architecture/diffusers.py.  Recorded: every attribute read on `self.<member>`, `pipe.<member>` or
`self.pipe.<member>`, and on a local name bound by a one-step alias such as `unet = self.pipe.unet`.

    python tests/golden/make_dropin_surface_names.py <reference tree>
"""
import ast
import glob
import json
import os
import sys

MEMBERS = ('unet', 'controlnet', 'vae', 'image_enhancer', 'segmentation', 'mesh_renderer')
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dropin_surface_names.json')
CLASS_FILTER = {'lib/models/architecture/diffusers.py': ('RefOnly', 'DepthControl')}

# names the engines deliberately do not carry: {member: {name: reason}}.  Written to the file whether or not the scan meets them: some are read in
# parts of the reference the scan leaves out on purpose (NOT_SCANNED), and the file is where a reader looks for the boundary of the surface.
NOT_SCANNED = {
    'lib/core/*_gui.py': 'training / GUI stack: drives the torch modules directly, never through a pipeline the drop-in serves',
    'lib/models/architecture/diffusers.py (other classes)': 'mmgen training wrappers around diffusers models (enable_gradient_checkpointing, LoRA)',
}
EXCLUDED = {
    'unet': {
        'modules': 'accelerate offload-hook walk of lib/pipelines/zero123.py, a pipeline lib.pipelines does not export; guarded by hasattr(_hf_hook)',
        'enable_gradient_checkpointing': 'training stack: the engines are inference-only',
        'train': 'training stack: the engines are inference-only',
        'requires_grad_': 'training stack: the engines are inference-only',
        'controlnet': 'attribute of the DepthControlUNet wrapper, which stays a torch module around the engine (dropin.swap_zero123)',
    },
    'vae': {
        'encoder': 'training stack (lib/core/*_gui.py, fine-tuning hooks): submodule access to the torch AutoencoderKL',
        'decoder': 'training stack (lib/core/*_gui.py, fine-tuning hooks): submodule access to the torch AutoencoderKL',
    },
    'controlnet': {}, 'image_enhancer': {}, 'segmentation': {},
    'mesh_renderer': {},
}


def _member_of(node):
    """`self.<m>`, `pipe.<m>`, `self.pipe.<m>` -> m."""
    if not isinstance(node, ast.Attribute) or node.attr not in MEMBERS:
        return None
    v = node.value
    if isinstance(v, ast.Name) and v.id in ('self', 'pipe'):
        return node.attr
    if isinstance(v, ast.Attribute) and v.attr == 'pipe' and isinstance(v.value, ast.Name) and v.value.id == 'self':
        return node.attr
    return None


def _scan(scope, found):
    aliases = {}
    for node in ast.walk(scope):          # one-step aliases of this function / class body
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            m = _member_of(node.value)
            if m:
                aliases[node.targets[0].id] = m
    for node in ast.walk(scope):
        if not isinstance(node, ast.Attribute):
            continue
        m = _member_of(node.value)
        if m is None and isinstance(node.value, ast.Name):
            m = aliases.get(node.value.id)
        if m is not None:
            found[m].add(node.attr)


def surface_names(ref):
    files = sorted(glob.glob(os.path.join(ref, 'lib', 'pipelines', '*.py')))
    files += [os.path.join(ref, p) for p in ('lib/apis/adapter3d.py', 'lib/models/architecture/ip_adapter/ip_adapter.py',
                                             'lib/models/architecture/joint_attn.py', 'lib/models/architecture/diffusers.py')]
    found = {m: set() for m in MEMBERS}
    for path in files:
        rel = os.path.relpath(path, ref).replace(os.sep, '/')
        tree = ast.parse(open(path).read())
        scopes = [tree]
        if rel in CLASS_FILTER:
            scopes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name.startswith(CLASS_FILTER[rel])]
        for scope in scopes:
            funcs = [n for n in ast.walk(scope) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]
            for fn in funcs or [scope]:
                _scan(fn, found)
    out = {}
    for m in MEMBERS:
        ex = dict(EXCLUDED.get(m, {}))
        out[m] = dict(names=sorted(found[m]), excluded=ex)
    out['_not_scanned'] = dict(NOT_SCANNED)
    return out


if __name__ == '__main__':
    with open(OUT, 'w') as f:
        json.dump(surface_names(sys.argv[1]), f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', OUT)
