"""Line-of-sight design matrix of satellite pairs, fused against composed, event-timed.
    python3 tools/los_design_time.py [--repeats R] [--degrees 60 96] [--pairs 100000] [--output profiles/los_design_time.txt]
At each degree N (min_degree 2), for M scattered pairs 220 km apart, on one default block of from_line_of_sight (Mb pairs):
  fused     engine.los_design_checked (one shg_los_design call, without the Python checks: the solid harmonics kernel on both
            satellites and the gather kernel), with the bytes it has to move (Y of both satellites written and read once, At [P][Mb]
            written) over the time
  composed  what the package offered before: engine.acceleration_design at a and at b (At [P][3][Mb] each), then
            e . (At_b - At_a) in torch; its bytes are the fused route's plus the six rows per pair written and read again
  product   N += At At^T of the block through engine.gemm (the full product, both triangles): of the fused At, flop = 2 Mb P^2, and of
            one acceleration design matrix of the same block, flop = 2 (3 Mb) P^2, as fractions of the 78.6 TFLOP/s fp64 peak
  whole     NormalEquations.from_line_of_sight of all M pairs
Warm-up 2 calls, median of R (default 10).  Prints one line per measurement and a JSON summary line, and writes both to --output."""
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
import los_inputs as li  # noqa: E402

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


def composed(N, nmin, a, b):
    """the route of the parent commit: two acceleration design matrices and the projection in torch"""
    d = b - a
    e = d / ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sqrt()[:, None]
    D = ga.engine.acceleration_design(N, b, ai.GM, ai.R, nmin) - ga.engine.acceleration_design(N, a, ai.GM, ai.R, nmin)
    return (e[:, 0] * D[:, 0] + e[:, 1] * D[:, 1]) + e[:, 2] * D[:, 2]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=10)
    parser.add_argument('--degrees', type=int, nargs='+', default=[60, 96])
    parser.add_argument('--pairs', type=int, default=100_000)
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'los_design_time.txt'))
    args = parser.parse_args()
    ga.engine.require_gpu()
    rows, lines = [], []

    def report(line):
        print(line, flush=True)
        lines.append(line)

    def product(At, N, P, block, label, K):
        normals = torch.zeros((P, P), dtype=torch.float64, device=At.device)
        ms = median_ms(lambda: ga.engine.gemm(At, At, transb=True, beta=1.0, out=normals), args.repeats)
        flop = 2.0 * K * block * P * P
        rows.append({'degree': N, 'what': 'product ' + label, 'pairs': block, 'ms': ms, 'tflops': flop / ms / 1e9,
                     'fraction_of_peak': flop / ms / 1e-3 / PEAK})
        report('product  d/o {0:3d} P {1:5d} Mb {2:6d} {3:12s}: {4:9.3f} ms  {5:6.2f} TFLOP/s = {6:.3f} of peak (full product)'.format(
            N, P, block, label, ms, rows[-1]['tflops'], rows[-1]['fraction_of_peak']))

    M, nmin = args.pairs, 2
    for N in args.degrees:
        P = (N + 1) ** 2 - nmin ** 2
        block = min(ga.lstsq.NormalEquations.default_block_points(P, 1), M)
        a_host = ai.scattered_positions(M, N + M)
        a = ga.engine.to_device(a_host)
        b = ga.engine.to_device(a_host + li.SEPARATION * li.unit_vectors(M, N))
        obs = torch.from_numpy(np.random.default_rng(N).standard_normal(M) * 1e-9).to(a.device)
        ab, bb = a[:block].contiguous(), b[:block].contiguous()
        harmonics = 2.0 * 2 * (N + 2) * (N + 3)                          # Y [packed][2] of both satellites, written and read once

        ms = median_ms(lambda: ga.engine.los_design_checked(N, nmin, ab, bb, None, None, ai.GM, ai.R), args.repeats)
        moved = 8.0 * block * (harmonics + P)
        rows.append({'degree': N, 'what': 'fused', 'pairs': block, 'ms': ms, 'gbytes_per_s': moved / ms / 1e6, 'pairs_per_s': block / ms * 1e3})
        report('fused    d/o {0:3d} P {1:5d} Mb {2:6d}: {3:9.3f} ms  {4:7.1f} GB/s  {5:.3e} pairs/s'.format(N, P, block, ms, rows[-1]['gbytes_per_s'],
                                                                                                      rows[-1]['pairs_per_s']))
        fused_ms = ms

        ms = median_ms(lambda: composed(N, nmin, ab, bb), args.repeats)
        moved = 8.0 * block * (harmonics + P + 2 * 6 * P)
        rows.append({'degree': N, 'what': 'composed', 'pairs': block, 'ms': ms, 'gbytes_per_s': moved / ms / 1e6, 'pairs_per_s': block / ms * 1e3,
                     'over_fused': ms / fused_ms})
        report('composed d/o {0:3d} P {1:5d} Mb {2:6d}: {3:9.3f} ms  {4:7.1f} GB/s  {5:.3e} pairs/s  ({6:.2f} x the fused call)'.format(
            N, P, block, ms, rows[-1]['gbytes_per_s'], rows[-1]['pairs_per_s'], ms / fused_ms))

        product(ga.engine.los_design(N, ab, bb, ai.GM, ai.R, nmin), N, P, block, 'line of sight', 1)
        product(ga.engine.acceleration_design(N, ab, ai.GM, ai.R, nmin).reshape(P, 3 * block), N, P, block, 'acceleration', 3)

        ms = median_ms(lambda: ga.lstsq.NormalEquations.from_line_of_sight(a, b, obs, nmin, N, ai.GM, ai.R), args.repeats)
        flop = 2.0 * M * P * P
        rows.append({'degree': N, 'what': 'whole', 'pairs': M, 'blocks': -(-M // block), 'ms': ms, 'tflops': flop / ms / 1e9,
                     'fraction_of_peak': flop / ms / 1e-3 / PEAK, 'pairs_per_s': M / ms * 1e3})
        report('whole    d/o {0:3d} P {1:5d} M  {2:6d}: {3:9.3f} ms  {4:6.2f} TFLOP/s = {5:.3f} of peak  {6:.3e} pairs/s  ({7} blocks)'.format(
            N, P, M, ms, rows[-1]['tflops'], rows[-1]['fraction_of_peak'], rows[-1]['pairs_per_s'], rows[-1]['blocks']))
        del a, b, obs, ab, bb
        torch.cuda.empty_cache()
    report(json.dumps({'los_design': rows}))
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
