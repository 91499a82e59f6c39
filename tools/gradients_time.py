"""Gravitational gradient tensor at points, event-timed.
    python3 tools/gradients_time.py [--repeats R] [--degrees 96 180]
At each degree N: 1 M shared positions x 1, x 4 and x 16 epochs, and 2.6 M positions of their own x 1 epoch (a month of 1 Hz orbit),
through engine.gravitational_gradients_points (one shg_gravitational_gradients_points call: the coefficient combination kernel and the
point kernel).  flop = M_eff (N+3)(N+4)/2 (24 B + 8): twelve FMAs per epoch and (n'', k) plus one recursion step (four flops), the
radial factor and the two trigonometric products per point and (n'', k); M_eff = points (shared) or points x epochs (per epoch, each
with its own recursion).  Fraction = flop / 78.6 TFLOP/s (fp64 vector and matrix peak) / time.
Prints one line per measurement and a JSON summary line."""
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
    parser.add_argument('--degrees', type=int, nargs='+', default=[96, 180])
    args = parser.parse_args()
    ga.engine.require_gpu()
    dev = ga.engine.device()
    rows = []
    for N in args.degrees:
        rng = np.random.default_rng(N)
        anm16 = torch.from_numpy(rng.standard_normal((16, N + 1, N + 1)) * 1e-10).to(dev)
        pairs = (N + 3) * (N + 4) // 2
        cases = (('shared', 1_000_000, 1), ('shared', 1_000_000, 4), ('shared', 1_000_000, 16), ('per_epoch', 2_600_000, 1))
        for layout, M, B in cases:
            xyz = ga.engine.to_device(ai.scattered_positions(M, N + M + B))
            anm = anm16[:B].contiguous()
            if layout == 'per_epoch':
                xyz = xyz.reshape(1, M, 3).expand(B, M, 3).contiguous()

            def run():
                return ga.engine.gravitational_gradients_points(N, xyz, anm, ai.GM, ai.R)
            ms = median_ms(run, args.repeats)
            m_eff = M * (B if layout == 'per_epoch' else 1)
            flop = float(m_eff) * pairs * (24 * (B if layout == 'shared' else 1) + 8)
            row = {'degree': N, 'layout': layout, 'points': M, 'epochs': B, 'ms': ms, 'tflops': flop / ms / 1e9,
                   'fraction_of_peak': flop / ms / 1e-3 / PEAK, 'points_per_s': M * B / ms * 1e3}
            rows.append(row)
            print('gradients d/o {0:3d} {1:9s} M {2:8d} B {3:2d}: {4:9.3f} ms  {5:6.2f} TFLOP/s = {6:.3f} of peak  {7:.3e} point-epochs/s'.format(
                N, layout, M, B, ms, row['tflops'], row['fraction_of_peak'], row['points_per_s']), flush=True)
            del xyz
            torch.cuda.empty_cache()
    print(json.dumps({'gradients': rows}))


if __name__ == '__main__':
    main()
