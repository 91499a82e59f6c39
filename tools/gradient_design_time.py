"""Normal equations from gradients, event-timed.
    python3 tools/gradient_design_time.py [--repeats R] [--degrees 60 96] [--points 100000] [--output profiles/gradient_design_time.txt]
At each degree N (min_degree 2), for M scattered positions with seeded instrument frames, and for the cases K = 6 with frames, K = 4
(xx, yy, zz, xz) with frames and K = 6 without frames:
  design   engine.gradient_design of one default block of points (one shg_gradient_design call: the solid harmonics kernel at degree
           N + 2 and the gather kernel), with the bytes it has to move, 8 (2 * 2 packed(N + 2) + K P + 9) per point (Y written and read
           once, At written, the frame read; the 9 also without frames), over the time
  product  N += At At^T of that block through engine.gemm (the full product): flop = 2 (K Mb) P^2, as a fraction of the 78.6 TFLOP/s
           fp64 peak: the rate the whole is set against
  whole    NormalEquations.from_gradients of all M points, with the flop count 2 (K M) P^2 over the whole time
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
import gradient_design_inputs as gdi  # noqa: E402
import grates_amd as ga  # noqa: E402

PEAK = 78.6e12
CASES = (('K 6 frames', None, True), ('K 4 frames', ('xx', 'yy', 'zz', 'xz'), True), ('K 6 fixed ', None, False))


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
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'gradient_design_time.txt'))
    args = parser.parse_args()
    ga.engine.require_gpu()
    rows, lines = [], []

    def report(line):
        print(line, flush=True)
        lines.append(line)

    M, nmin = args.points, 2
    for N in args.degrees:
        P = (N + 1) ** 2 - nmin ** 2
        xyz = ga.engine.to_device(ai.scattered_positions(M, N + M))
        frames_all = ga.engine.to_device(gdi.frames(M, N))
        for label, components, framed in CASES:
            K = 6 if components is None else len(components)
            block = min(ga.lstsq.NormalEquations.default_block_points(P, K), M)
            frames = frames_all if framed else None
            obs = torch.from_numpy(np.random.default_rng(N).standard_normal((M, K)) * 1e-9).to(xyz.device)
            xb, fb = xyz[:block].contiguous(), (frames[:block].contiguous() if framed else None)

            ms = median_ms(lambda: ga.engine.gradient_design(N, xb, ai.GM, ai.R, nmin, fb, components), args.repeats)
            moved = 8.0 * block * (2 * (N + 3) * (N + 4) + K * P + 9)
            rows.append({'degree': N, 'case': label.strip(), 'what': 'design', 'points': block, 'ms': ms, 'gbytes_per_s': moved / ms / 1e6,
                         'points_per_s': block / ms * 1e3})
            report('design  d/o {0:3d} {1} P {2:5d} Mb {3:6d}: {4:9.3f} ms  {5:7.1f} GB/s  {6:.3e} points/s'.format(
                N, label, P, block, ms, rows[-1]['gbytes_per_s'], rows[-1]['points_per_s']))

            At = ga.engine.gradient_design(N, xb, ai.GM, ai.R, nmin, fb, components).reshape(P, K * block)
            normals = torch.zeros((P, P), dtype=torch.float64, device=xyz.device)
            ms = median_ms(lambda: ga.engine.gemm(At, At, transb=True, beta=1.0, out=normals), args.repeats)
            flop = 2.0 * K * block * P * P
            rows.append({'degree': N, 'case': label.strip(), 'what': 'product', 'points': block, 'ms': ms, 'tflops': flop / ms / 1e9,
                         'fraction_of_peak': flop / ms / 1e-3 / PEAK})
            report('product d/o {0:3d} {1} P {2:5d} Mb {3:6d}: {4:9.3f} ms  {5:6.2f} TFLOP/s = {6:.3f} of peak (full product)'.format(
                N, label, P, block, ms, rows[-1]['tflops'], rows[-1]['fraction_of_peak']))
            del At, normals

            ms = median_ms(lambda: ga.lstsq.NormalEquations.from_gradients(xyz, obs, nmin, N, ai.GM, ai.R, frames=frames, components=components),
                           args.repeats)
            flop = 2.0 * K * M * P * P
            rows.append({'degree': N, 'case': label.strip(), 'what': 'whole', 'points': M, 'blocks': -(-M // block), 'ms': ms,
                         'tflops': flop / ms / 1e9, 'fraction_of_peak': flop / ms / 1e-3 / PEAK, 'points_per_s': M / ms * 1e3})
            report('whole   d/o {0:3d} {1} P {2:5d} M  {3:6d}: {4:9.3f} ms  {5:6.2f} TFLOP/s = {6:.3f} of peak  {7:.3e} points/s  ({8} blocks)'.format(
                N, label, P, M, ms, rows[-1]['tflops'], rows[-1]['fraction_of_peak'], rows[-1]['points_per_s'], rows[-1]['blocks']))
            del obs, xb, fb
            torch.cuda.empty_cache()
        del xyz, frames_all
    report(json.dumps({'gradient_design': rows}))
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
