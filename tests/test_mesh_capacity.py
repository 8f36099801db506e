"""Capacity (host-read-free) form of the mesh optimisation iteration, the parts that need no GPU.

  * include/mvedit_amd.h declares every `_n` entry point of the mesh half (tests/test_abi.py then checks the arity of their call sites by
    itself), each with the exact call's arguments plus the capacities / device counts;
  * `DMTet.__call__(capacity=...)` rejects non-positive capacities before anything is launched;
  * the bounds arithmetic the kernels share (mvedit_amd/csrc/mesh_capacity_core.h: the totals, the all-or-nothing live counts, the overflow
    flag, the clamp of a device count, which rows are written and which padded) is walked by a stand-alone host program built with the
    address and undefined-behaviour sanitizers (tests/mesh_capacity_core_host.cpp, run as a program of its own) and compared with the
    restatement of the rules below.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = dict(mve_dmtet_extract_n=16, mve_dmtet_backward_n=9, mve_mesh_normals_forward_n=9, mve_mesh_normals_backward_n=11,
                        mve_mesh_reg_forward_n=10, mve_mesh_reg_backward_n=12, mve_edge_opposites_n=7)


def test_header_declares_the_mesh_capacity_entry_points(lib):
    for name, nargs in NEW_ENTRY_POINTS.items():
        assert name in lib.PROTOS, name
        assert len(lib.PROTOS[name][1]) == nargs, (name, len(lib.PROTOS[name][1]))
        assert any(t.replace(' ', '') == 'constint32_t*' and a == 'd_live' for t, a in lib.PROTOS[name][1]) or name == 'mve_dmtet_extract_n', name
    # each takes the exact call's arguments plus the device live counts
    for exact, n in (('mve_mesh_normals_forward', 'mve_mesh_normals_forward_n'), ('mve_mesh_normals_backward', 'mve_mesh_normals_backward_n'),
                     ('mve_mesh_reg_forward', 'mve_mesh_reg_forward_n'), ('mve_mesh_reg_backward', 'mve_mesh_reg_backward_n'),
                     ('mve_edge_opposites', 'mve_edge_opposites_n'), ('mve_dmtet_backward', 'mve_dmtet_backward_n')):
        assert len(lib.PROTOS[n][1]) == len(lib.PROTOS[exact][1]) + 1, n
    # the extraction publishes its three device words
    names = [a for _, a in lib.PROTOS['mve_dmtet_extract_n'][1]]
    assert {'v_cap', 'f_cap', 'd_counts', 'd_live', 'd_overflow'} <= set(names)


def test_capacity_argument_errors_come_before_any_launch(lib, monkeypatch):
    from mvedit_amd import mesh_ops

    def no_launch(name, *a):
        raise AssertionError(f'{name} was launched')
    monkeypatch.setattr(lib, 'call', no_launch)
    dm = mesh_ops.DMTet('cpu')
    pos, sdf, tets = torch.zeros(4, 3), torch.ones(4), torch.tensor([[0, 1, 2, 3]])
    for bad in ((0, 8), (8, 0), (-1, 8), (8, -4096), (0, 0)):
        with pytest.raises(ValueError, match='capacity'):
            dm(pos, sdf, tets, capacity=bad)
    assert dm.counts is None and dm.live is None and dm.overflow is None


# --------------------------------------------------------------------------------------------------------------------------------
# the rules, restated (mesh_capacity_core.h says them in words)
def resolve_rule(nv, nf, v_cap, f_cap):
    """-> (counts, live, overflow): the totals always; the live counts all or nothing"""
    overflow = int(nv > v_cap or nf > f_cap)
    return (nv, nf), ((0, 0) if overflow else (nv, nf)), overflow


def clamp_rule(count, capacity):
    return min(max(count, 0), max(capacity, 0))


def _cases():
    rng = np.random.default_rng(23)
    cases = []
    for nv, nf in ((0, 0), (1, 1), (3, 1), (4, 2), (12, 20), (255, 506), (256, 508), (257, 510), (1000, 1996)):
        caps_v = {1, max(nv - 1, 1), max(nv, 1), nv + 1, nv // 2 + 1, 2 * nv + 3}       # below, at and above the total; capacity 1
        caps_f = {1, max(nf - 1, 1), max(nf, 1), nf + 1, nf // 2 + 1, 2 * nf + 3}
        for v_cap in sorted(caps_v):
            for f_cap in sorted(caps_f):
                gv, gf = (int(g) for g in rng.choice([-2 ** 31, -7, -1, 0, 1, v_cap - 1, v_cap, v_cap + 1, 2 ** 31 - 1], 2))
                cases.append((nv, nf, v_cap, f_cap, gv, gf))
    return cases


def test_bounds_arithmetic_host_walk_under_sanitizers(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = tmp_path / 'mesh_capacity_core_host'
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(ROOT, 'tests', 'mesh_capacity_core_host.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    cases = _cases()
    text = [str(len(cases))] + [' '.join(map(str, c)) for c in cases]
    # the program is run directly, as its own process, in the inherited environment; a library someone preloads must not make the
    # sanitizer refuse to start it
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:verify_asan_link_order=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([str(exe)], input='\n'.join(text) + '\n', capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    lines = run.stdout.strip().splitlines()
    assert len(lines) == len(cases) + 9
    seen = dict(overflow_v=0, overflow_f=0, exact_fit=0, empty=0, roomy=0)
    for (nv, nf, v_cap, f_cap, gv, gf), line in zip(cases, lines):
        got = [int(v) for v in line.split()]
        counts, live, overflow = resolve_rule(nv, nf, v_cap, f_cap)
        want = [*counts, *live, overflow,
                live[0], live[1],                                    # rows written: exactly the live ones
                v_cap - live[0], f_cap - live[1],                    # rows padded: every other row of the buffers
                0,                                                   # nothing left stale
                -(-live[0] // 256),                                  # 256-row blocks that hold live rows
                clamp_rule(gv, v_cap), clamp_rule(gf, f_cap)]
        assert got == want, ((nv, nf, v_cap, f_cap, gv, gf), got, want)
        assert (live == (0, 0)) if overflow else (live == counts)    # the empty mesh, never a truncated one
        seen['overflow_v'] += int(nv > v_cap)
        seen['overflow_f'] += int(nf > f_cap and nv <= v_cap)
        seen['exact_fit'] += int(nv == v_cap and nf == f_cap)
        seen['empty'] += int(nv == 0)
        seen['roomy'] += int(nv < v_cap and nf < f_cap)
    assert all(v > 0 for v in seen.values()), seen
    probes = [-2 ** 31, -5, 0, 1, 6, 7, 8, 2 ** 31 - 1]
    for c, line in zip(probes, lines[len(cases):]):
        assert [int(v) for v in line.split()] == [clamp_rule(c, 7), 0, clamp_rule(c, 1), 0], c
    assert lines[-1] == '7 0 0 0 1 2'


def test_padding_values_are_the_ones_the_exact_kernels_give():
    """The header states vn = face_normals = (0, 0, 0) for padded rows: what the host build of the exact arithmetic gives for the padded
    face (0, 0, 0) and for a vertex no face touches."""
    from oracle import devcore as D
    verts = np.array([[0.1, 0.2, 0.3], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [5.0, 5.0, 5.0]], np.float32)
    faces = np.array([[1, 2, 0], [0, 0, 0]], np.int32)
    h = D.mesh_normals(verts, faces, None, np.zeros((2, 3), np.float32))
    assert (h['face_normals'][1] == 0).all() and (h['vn'][3] == 0).all() and np.abs(h['face_normals'][0]).max() > 0.5
