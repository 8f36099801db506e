"""Capacity (host-read-free) form of the NeRF training iteration, the parts that need no GPU.

  * `VolumeRenderer.forward(capacity=...)` rejects bad arguments before anything is launched, and include/mvedit_amd.h declares every
    `_n` entry point (tests/test_abi.py then checks the arity of their call sites by itself);
  * the bounds arithmetic the kernels share (mvedit_amd/csrc/capacity_core.h: which rays fit a capacity, the live count after the march,
    the cull re-index of a ray that did not fit) is walked by a stand-alone host program built with the address and undefined-behaviour
    sanitizers (tests/capacity_core_host.cpp, run as a program of its own) and compared with the restatement of the rules below.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = dict(mve_march_rays_train_clamp=8, mve_cull_samples_n=17, mve_hashgrid_mlp_decode_n=21, mve_hashgrid_mlp_backward_n=28,
                        mve_recon_loss_forward_n=8, mve_recon_loss_backward_n=12, mve_adam_step_n=12, mve_adam_advance_n=3)


def test_header_declares_the_capacity_entry_points(lib):
    for name, nargs in NEW_ENTRY_POINTS.items():
        assert name in lib.PROTOS, name
        assert len(lib.PROTOS[name][1]) == nargs, (name, len(lib.PROTOS[name][1]))
    # each takes the exact call's arguments plus the device count (and, for Adam, the device step and skip flag instead of the host step)
    for exact, n, extra in (('mve_cull_samples', 'mve_cull_samples_n', 1), ('mve_hashgrid_mlp_decode', 'mve_hashgrid_mlp_decode_n', 1),
                            ('mve_hashgrid_mlp_backward', 'mve_hashgrid_mlp_backward_n', 1), ('mve_recon_loss_forward', 'mve_recon_loss_forward_n', 1),
                            ('mve_recon_loss_backward', 'mve_recon_loss_backward_n', 1), ('mve_adam_step', 'mve_adam_step_n', 1)):
        assert len(lib.PROTOS[n][1]) == len(lib.PROTOS[exact][1]) + extra, n
        assert any(t.replace(' ', '') == 'constint32_t*' for t, _ in lib.PROTOS[n][1]), n


def test_forward_capacity_argument_errors_come_before_any_launch(lib, monkeypatch):
    from mvedit_amd import nerf
    from oracle import nerf_oracle as NO
    p = NO.make_nerf_params(12, 320, seed=7, table_scale=0.1)
    dec = nerf.INGPDecoderParams(p['table'], p['w1'], p['b1'], p['w2'], p['b2'], 12, 320, device='cpu')
    vr = nerf.VolumeRenderer(dec)

    def no_launch(name, *a):
        raise AssertionError(f'{name} was launched')
    monkeypatch.setattr(lib, 'call', no_launch)
    o, d, bits = torch.zeros(4, 3), torch.ones(4, 3), torch.zeros(64 ** 3 // 8, dtype=torch.uint8)
    vr.training = False
    with pytest.raises(ValueError, match='training'):
        vr.forward(o, d, bits, 64, capacity=1000)
    vr.training = True
    for bad in (0, -1, -4096):
        with pytest.raises(ValueError, match='capacity'):
            vr.forward(o, d, bits, 64, capacity=bad)
    # the optimiser state is either host-counted or device-counted, never both
    with pytest.raises(ValueError, match='device'):
        dec.adam_step({}, dict(step=torch.zeros(1, dtype=torch.int32)))


# --------------------------------------------------------------------------------------------------------------------------------
# the rules, restated (capacity_core.h says them in words)
def clamp_rule(cnt, capacity):
    """-> (marched total, live count, overflow): the live count is the end of the longest prefix of whole rays that fit"""
    ends = np.cumsum(np.asarray(cnt, np.int64))
    total = int(ends[-1]) if len(ends) else 0
    fit = ends[ends <= capacity]
    return total, (int(fit.max()) if len(fit) else 0), int(total > capacity)


def cull_rule(cnt, live, keep):
    """-> (kept, [(offset, count)]): rays inside the live rows are re-indexed through the prefix counts, any other ray keeps nothing"""
    cnt = np.asarray(cnt, np.int64)
    ends = np.cumsum(cnt)
    offs = ends - cnt
    pref = np.concatenate([[0], np.cumsum(np.asarray(keep[:live], np.int64))])
    kept = int(pref[live])
    rays = [(int(pref[o]), int(pref[e] - pref[o])) if e <= live else (kept, 0) for o, e in zip(offs, ends)]
    return kept, rays


def _cases():
    rng = np.random.default_rng(11)
    cases = []
    for N in (0, 1, 2, 7, 64, 300):
        for trial in range(6):
            cnt = rng.integers(0, 9, N)
            cnt[rng.random(N) < 0.3] = 0                                   # rays that meet nothing
            if trial == 5:
                cnt[:] = 0
            total = int(cnt.sum())
            caps = {0, 1, max(total - 1, 0), total, total + 1, total // 2, 2 * total + 3}      # below, at and above the total; 0 and 1
            if N:
                ends = np.cumsum(cnt)
                caps |= {int(ends[N // 2]), max(int(ends[N // 2]) - 1, 0)}  # exactly at / one short of a ray end
            for cap in sorted(caps):
                keep = (rng.random(cap) < 0.6).astype(np.int64)
                cases.append((cnt, cap, keep))
    return cases


def test_bounds_arithmetic_host_walk_under_sanitizers(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = tmp_path / 'capacity_core_host'
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(ROOT, 'tests', 'capacity_core_host.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    cases = _cases()
    text = [str(len(cases))]
    for cnt, cap, keep in cases:
        text.append(f'{len(cnt)} {cap}')
        text.append(' '.join(map(str, cnt)))
        text.append(' '.join(map(str, keep)))
    # the environment is the inherited one; a library someone preloads must not make the sanitizer refuse to start this program
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:verify_asan_link_order=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([str(exe)], input='\n'.join(text) + '\n', capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    lines = run.stdout.strip().splitlines()
    assert len(lines) == len(cases) + 9
    seen_overflow = seen_partial = 0
    for (cnt, cap, keep), line in zip(cases, lines):
        got = [int(v) for v in line.split()]
        total, count, overflow = clamp_rule(cnt, cap)
        kept, rays = cull_rule(cnt, count, keep)
        deciders = 1 if len(cnt) else 0                                    # exactly one ray writes the count
        assert got[:6] == [total, count, deciders, overflow, count, kept], (list(cnt), cap, got[:6])
        assert got[6:] == [v for r in rays for v in r], (list(cnt), cap)
        assert count <= cap and count <= total and (count == total) == (overflow == 0)
        assert all(0 <= o and o + c <= kept <= count for o, c in rays)     # the re-indexed table stays inside the kept rows
        seen_overflow += overflow
        seen_partial += int(overflow and 0 < count)
    assert seen_overflow > 20 and seen_partial > 10                        # the walk met overflows, also ones that keep some whole rays
    probes = [-2 ** 31, -5, 0, 1, 6, 7, 8, 2 ** 31 - 1]
    for c, line in zip(probes, lines[len(cases):]):
        assert [int(v) for v in line.split()] == [min(max(c, 0), 7), 0, min(max(c, 0), 1)], c
    assert lines[-1] == '7'
