"""engine.leverages against the route that exists without it, event-timed.
    python3 tools/leverage_time.py [--rounds R] [--degrees 40 96]
Per degree N (min_degree 2, P = (N + 1)^2 - 4) a default block of accelerations, cols = 3 NormalEquations.default_block_points(P, 3), a
random upper triangular Ui [P, P] and a random X [P, cols]:
  fused    engine.leverages(Ui, X): Z = Ui^T X is never stored
  staged   engine.gemm_ex(Ui, X, Z, transa=True, flags=GEMM_A_LOWER) into a Z buffer of the size of X, then engine.column_dots(Z, Z)
The two routes alternate inside one process on one device, warm-up 2 rounds, then R rounds (default 15); per route the median and the
minimum, TFLOP/s counted as P^2 cols (the triangle) over the median, and the ratio fused / staged of the medians.  Prints one line per
degree and a JSON summary line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import grates_amd as ga  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=15)
    parser.add_argument('--degrees', type=int, nargs='+', default=[40, 96])
    args = parser.parse_args()
    ga.engine.require_gpu()
    summary = []
    for N in args.degrees:
        P = (N + 1) ** 2 - 4
        cols = 3 * ga.lstsq.NormalEquations.default_block_points(P, 3)
        generator = torch.Generator(device='cuda').manual_seed(N)
        Ui = torch.triu(torch.randn((P, P), dtype=torch.float64, device='cuda', generator=generator)) / np.sqrt(P)
        X = torch.randn((P, cols), dtype=torch.float64, device='cuda', generator=generator)
        Z, out = torch.empty_like(X), torch.empty(cols, dtype=torch.float64, device='cuda')

        def fused():
            ga.engine.leverages(Ui, X, out=out)

        def staged():
            ga.engine.gemm_ex(Ui, X, Z, transa=True, flags=ga.engine.GEMM_A_LOWER)
            return ga.engine.column_dots(Z, Z)
        for _ in range(2):
            fused()
            reference = staged()
        torch.cuda.synchronize()
        deviation = float(((out - reference).abs() / reference).max().item())
        times = {'fused': [], 'staged': []}
        for _ in range(args.rounds):
            times['fused'].append(event_ms(fused))
            times['staged'].append(event_ms(staged))
        flop = float(P) * P * cols
        record = {'degree': N, 'parameters': P, 'columns': cols, 'z_buffer_mb': round(8.0 * P * cols / 2 ** 20, 1), 'relative_deviation': deviation}
        for name, values in times.items():
            record[name + '_ms'] = round(float(np.median(values)), 4)
            record[name + '_min_ms'] = round(float(np.min(values)), 4)
            record[name + '_tflops'] = round(flop / np.median(values) * 1e-9, 2)
        record['ratio'] = round(record['fused_ms'] / record['staged_ms'], 4)
        print('d/o {degree}: P {parameters}, {columns} columns: fused {fused_ms} ms (min {fused_min_ms}, {fused_tflops} TFLOP/s), staged {staged_ms} ms '
              '(min {staged_min_ms}, {staged_tflops} TFLOP/s), ratio {ratio}; routes agree to {relative_deviation:.1e}'.format(**record))
        summary.append(record)
    print(json.dumps({'leverage_time': summary}))


if __name__ == '__main__':
    main()
