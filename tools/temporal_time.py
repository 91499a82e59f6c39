"""Normal equations of time-variable parameters, event-timed.
    python3 tools/temporal_time.py [--repeats R] [--degree 40] [--days 30] [--output profiles/temporal_time.txt]
Coefficients of degrees 2 .. N (d/o 40: P = 1677) at daily nodes, `days` + 1 of them, 17 280 time-ordered positions per day (5 s
sampling), linear interpolation between the nodes (W = 2), one process, medians of R runs:
  static     NormalEquations.from_accelerations on the same points: one set of parameters, a code path this work does not alter
  white      TemporalParameters.linear(...).from_accelerations: three products per block against one
  coloured   the same under ColouredNoise of order q = 8, one arc per day
  expand     engine.window_expand alone on one default block of the white call, as a share of that block (the call's time over its
             number of blocks)
Prints one line per measurement and a JSON summary line with the commit and the hashes of the kernel sources."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import acceleration_inputs as ai  # noqa: E402
import grates_amd as ga  # noqa: E402
import source_hashes  # noqa: E402
import whitening_inputs as wi  # noqa: E402

PER_DAY, MIN_DEGREE, ORDER = 17280, 2, 8


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([event_ms(fn) for _ in range(repeats)]))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=7)
    parser.add_argument('--degree', type=int, default=40)
    parser.add_argument('--days', type=int, default=30)
    parser.add_argument('--output', default=None)
    args = parser.parse_args()
    ga.engine.require_gpu()
    ls, N, B = ga.lstsq, args.degree, args.days + 1
    M, P = args.days * PER_DAY, (args.degree + 1) ** 2 - MIN_DEGREE ** 2
    lines = []

    def report(text):
        print(text, flush=True)
        lines.append(text)

    xyz = ga.engine.to_device(ai.scattered_positions(M, N + M))
    g = ga.engine.to_device(np.random.default_rng(N).standard_normal((M, 3)) * 1e-6)
    nodes = 58000.0 + np.arange(B, dtype=np.float64)
    epochs = 58000.0 + (np.arange(M) + 0.5) / PER_DAY
    arcs = np.arange(0, M, PER_DAY)
    white = ls.TemporalParameters.linear(nodes, epochs)
    coloured = ls.TemporalParameters.linear(nodes, epochs, model=ls.ColouredNoise(wi.synthetic_sequence(ls, ORDER, 3601), arcs))
    block_points = ls.TemporalParameters.default_block_points(P, 3, 2)
    blocks = len(ls.temporal_blocks(white.first, 2, block_points))

    static_ms = median_ms(lambda: ls.NormalEquations.from_accelerations(xyz, g, MIN_DEGREE, N, ai.GM, ai.R), args.repeats)
    white_ms = median_ms(lambda: white.from_accelerations(xyz, g, MIN_DEGREE, N, ai.GM, ai.R), args.repeats)
    coloured_ms = median_ms(lambda: coloured.from_accelerations(xyz, g, MIN_DEGREE, N, ai.GM, ai.R), args.repeats)

    T = ga.engine.acceleration_design_checked(N, MIN_DEGREE, xyz[:block_points], None, ai.GM, ai.R).reshape(P * 3, block_points)
    factors = ga.engine.to_device(white.factors[:block_points])
    slot, begin = np.zeros(1, dtype=np.int32), np.array([0, block_points], dtype=np.int32)
    out = torch.empty((2, P * 3, block_points), dtype=torch.float64, device=T.device)
    expand_ms = median_ms(lambda: ga.engine.window_expand(T, factors, slot, begin, 2, out=out), args.repeats, warmup=2)
    moved = 3 * T.numel() * 8                                                               # one read and two writes
    block_ms = white_ms / blocks

    size = 'd/o {0}..{1} (P {2}), {3} nodes, M {4}'.format(MIN_DEGREE, N, P, B, M)
    report('static   {0}: NormalEquations.from_accelerations {1:10.2f} ms'.format(size, static_ms))
    report('white    {0}: TemporalParameters.linear, {1} blocks of {2} points {3:10.2f} ms = {4:.2f} x the static call'.format(
        size, blocks, block_points, white_ms, white_ms / static_ms))
    report('coloured {0}: the same under ColouredNoise(q = {1}), an arc per day {2:10.2f} ms = {3:.2f} x the static call, {4:.2f} x white'.format(
        size, ORDER, coloured_ms, coloured_ms / static_ms, coloured_ms / white_ms))
    report('expand   one block of {0} points, E = W = 2: {1:8.3f} ms ({2:.2f} TB/s over one read and two writes) = {3:.2f} % of the {4:.2f} ms '
           'of a block of the white call'.format(block_points, expand_ms, moved / expand_ms / 1e9, 100.0 * expand_ms / block_ms, block_ms))
    summary = json.dumps({'commit': source_hashes.commit(),
                          'sources': {name: source_hashes.file_hash(name) for name in ('common.h', 'window.hip', 'whiten.hip', 'design.hip', 'blas.hip')},
                          'temporal': {'degree': N, 'parameters': P, 'nodes': B, 'points': M, 'block_points': block_points, 'blocks': blocks,
                                       'static_ms': static_ms, 'white_ms': white_ms, 'coloured_ms': coloured_ms, 'white_over_static': white_ms / static_ms,
                                       'coloured_over_static': coloured_ms / static_ms, 'expand_ms': expand_ms, 'expand_share_of_block': expand_ms / block_ms,
                                       'expand_tb_per_s': moved / expand_ms / 1e9}})
    report(summary)
    if args.output:
        with open(args.output, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
