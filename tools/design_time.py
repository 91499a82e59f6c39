"""Normal equations from accelerations, event-timed.
    python3 tools/design_time.py [--repeats R] [--degrees 60 96] [--points 100000]
At each degree N (min_degree 2), for M scattered positions:
  design   engine.acceleration_design of one default block of points (one shg_acceleration_design call: the solid harmonics kernel and
           the gather kernel), with the bytes it has to move (Y written and read once, At written) over the time
  product  N += At At^T of that block through engine.gemm (the full product, both triangles): flop = 2 (3 Mb) P^2, as a fraction of the
           78.6 TFLOP/s fp64 peak
  whole    NormalEquations.from_accelerations of all M points (blocks of design + three products, then the mirror), with the same
           flop count 2 (3 M) P^2 over the whole time
Warm-up 2 calls, median of R (default 10).  Prints one line per measurement and a JSON summary line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import acceleration_inputs as ai  # noqa: E402
import grates_amd as ga  # noqa: E402

PEAK = 78.6e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([event_ms(fn) for _ in range(repeats)]))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=10)
    parser.add_argument('--degrees', type=int, nargs='+', default=[60, 96])
    parser.add_argument('--points', type=int, default=100_000)
    args = parser.parse_args()
    ga.engine.require_gpu()
    rows = []
    M, nmin = args.points, 2
    for N in args.degrees:
        P = (N + 1) ** 2 - nmin ** 2
        block = min(ga.lstsq.NormalEquations.default_block_points(P, 3), M)
        xyz = ga.engine.to_device(ai.scattered_positions(M, N + M))
        g = torch.from_numpy(np.random.default_rng(N).standard_normal((M, 3)) * 1e-6).to(xyz.device)
        xb = xyz[:block].contiguous()

        ms = median_ms(lambda: ga.engine.acceleration_design(N, xb, ai.GM, ai.R, nmin), args.repeats)
        moved = 8.0 * block * (2 * (N + 2) * (N + 3) + 3 * P)               # Y [packed][2] written and read, At [P][3] written
        rows.append({'degree': N, 'what': 'design', 'points': block, 'ms': ms, 'gbytes_per_s': moved / ms / 1e6, 'points_per_s': block / ms * 1e3})
        print('design  d/o {0:3d} P {1:5d} Mb {2:6d}: {3:9.3f} ms  {4:7.1f} GB/s  {5:.3e} points/s'.format(N, P, block, ms, rows[-1]['gbytes_per_s'],
                                                                                                       rows[-1]['points_per_s']), flush=True)

        At = ga.engine.acceleration_design(N, xb, ai.GM, ai.R, nmin).reshape(P, 3 * block)
        normals = torch.zeros((P, P), dtype=torch.float64, device=xyz.device)
        ms = median_ms(lambda: ga.engine.gemm(At, At, transb=True, beta=1.0, out=normals), args.repeats)
        flop = 2.0 * 3 * block * P * P
        rows.append({'degree': N, 'what': 'product', 'points': block, 'ms': ms, 'tflops': flop / ms / 1e9, 'fraction_of_peak': flop / ms / 1e-3 / PEAK,
                     'upper_only': False})
        print('product d/o {0:3d} P {1:5d} Mb {2:6d}: {3:9.3f} ms  {4:6.2f} TFLOP/s = {5:.3f} of peak (full product)'.format(
            N, P, block, ms, rows[-1]['tflops'], rows[-1]['fraction_of_peak']), flush=True)
        del At, normals

        ms = median_ms(lambda: ga.lstsq.NormalEquations.from_accelerations(xyz, g, nmin, N, ai.GM, ai.R), args.repeats)
        flop = 2.0 * 3 * M * P * P
        rows.append({'degree': N, 'what': 'whole', 'points': M, 'blocks': -(-M // block), 'ms': ms, 'tflops': flop / ms / 1e9,
                     'fraction_of_peak': flop / ms / 1e-3 / PEAK, 'points_per_s': M / ms * 1e3})
        print('whole   d/o {0:3d} P {1:5d} M  {2:6d}: {3:9.3f} ms  {4:6.2f} TFLOP/s = {5:.3f} of peak  {6:.3e} points/s  ({7} blocks)'.format(
            N, P, M, ms, rows[-1]['tflops'], rows[-1]['fraction_of_peak'], rows[-1]['points_per_s'], rows[-1]['blocks']), flush=True)
        del xyz, g, xb
        torch.cuda.empty_cache()
    print(json.dumps({'design': rows}))


if __name__ == '__main__':
    main()
