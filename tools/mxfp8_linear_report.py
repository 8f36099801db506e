"""The linear shapes of the SDXL transformer at BASELINE config 5's size (B = 2, 96 x 96 latent: 4608 rows at the 640-wide level, 1152 at the
1280-wide one) on the existing fp16 `ops.gemm` and on the MXFP8 block-scaled path (`mxfp8.gemm` alone, and quantise + GEMM as a layer would run
it: the weight is packed once, the activations on every call), with the rel-L2 of both against float64 on N(0, 1) data.  Nothing is asserted and
there is no target: the table is where the number gets written down.  One process, HIP events around `--reps` calls after a warm-up, three
alternating windows per path, the median reported.  The timed calls go straight to the C entry points with prepared arguments and
preallocated outputs (what an engine would do), so that a 10-microsecond kernel is not timed as its Python wrapper.

    python tools/mxfp8_linear_report.py [--out profiles/mxfp8_linear.txt] [--reps 40]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvedit_amd import _lib, mxfp8, ops  # noqa: E402
from tools.microbench import timeit  # noqa: E402


def shapes():
    out = []
    for C, rows in ((640, 4608), (1280, 1152)):
        out += [(f'{C}: to_q / to_k / to_v / to_out', rows, C, C, rows // 2),
                (f'{C}: context to_k / to_v', 2 * 77, C, 2048, 77),
                (f'{C}: ff in (GEGLU halves)', rows, 8 * C, C, rows // 2),
                (f'{C}: ff out', rows, C, 4 * C, rows // 2)]
    out.append(('4608 x 1280 x 1280', 4608, 1280, 1280, 2304))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mxfp8_linear.txt'))
    ap.add_argument('--reps', type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mxfp8_linear_report needs the GPU: nothing is measured without one')
    dev, g = 'cuda', torch.Generator().manual_seed(0)
    lines = [f'# tools/mxfp8_linear_report.py on {torch.cuda.get_device_name(0)}: fp16 ops.gemm vs MXFP8 (v_mfma_scale_f32_16x16x128_f8f6f4), '
             f'median of 3 windows of {args.reps} calls, ms; TF = 2 M N K / time; rel-L2 against float64 on N(0, 1) data (weights N(0, 1 / K))',
             f'{"layer":34s} {"M":>5s} {"N":>6s} {"K":>5s} | {"fp16 ms":>8s} {"TF":>5s} | {"mx gemm":>8s} {"TF":>5s} | {"quant+gemm":>10s} {"TF":>5s} {"vs fp16":>7s} |'
             f' {"relL2 fp16":>10s} {"relL2 mxfp8":>11s}']
    print('\n'.join(lines), flush=True)
    for name, M, N, K, rpi in shapes():
        a = torch.randn(M, K, generator=g).to(dev).half()
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dev).half()
        bias = torch.randn(N, generator=g).to(dev)
        lin = mxfp8.MXFP8Linear(w, bias)
        aq, ae = mxfp8.quantize(a)
        want = a.double() @ w.double().T + bias.double()
        rel = [float((y.double() - want).norm() / want.norm()) for y in (ops.gemm(a, w, bias=bias, rows_per_image=rpi), lin(a))]
        out = torch.empty(M, N, dtype=torch.float16, device=dev)
        nws = _lib.raw('mve_gemm_workspace_bytes')(M, N, K, rpi)
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
        st, P = _lib.stream_ptr(dev), _lib.ptr
        g16, gq, gm = _lib.raw('mve_gemm'), _lib.raw('mve_mxfp8_quantize'), _lib.raw('mve_mxfp8_gemm')
        a16 = (1, P(a), K, P(w), K, P(out), N, M, N, K, P(bias), None, 0, 0, None, 0, 0, 1.0, P(ws) if nws else None, nws, rpi, st)
        aqz = (1, P(a), K, M, K, P(aq), P(ae), st)
        amx = (P(aq), P(ae), P(lin.wq), P(lin.we), M, N, K, 1, P(out), N, P(bias), None, 0, st)

        def both():
            gq(*aqz)
            gm(*amx)
        paths = [lambda: g16(*a16), lambda: gm(*amx), both]
        assert g16(*a16) == 0 and gq(*aqz) == 0 and gm(*amx) == 0, _lib.last_error()
        assert torch.equal(out, lin(a))
        ts = [[], [], []]
        for _ in range(3):
            for i, f in enumerate(paths):
                ts[i].append(timeit(f, 5, args.reps) * 1e3)
        t = [sorted(x)[1] for x in ts]
        tf = [2.0 * M * N * K / x / 1e9 for x in t]
        line = (f'{name:34s} {M:5d} {N:6d} {K:5d} | {t[0]:8.4f} {tf[0]:5.0f} | {t[1]:8.4f} {tf[1]:5.0f} | {t[2]:10.4f} {tf[2]:5.0f} {t[0] / t[2]:6.2f}x |'
                f' {rel[0]:10.3e} {rel[1]:11.3e}')
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
