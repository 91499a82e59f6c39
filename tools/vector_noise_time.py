"""Vector whitening of the design matrix, event-timed.
    python3 tools/vector_noise_time.py [--repeats R] [--degree 96] [--blocks 4]
At degree N (min_degree 2), K = 3, with the default block of points, one arc, for q = 5 and q = 128 (seeded synthetic models):
  vector   engine.whiten_rows_vector of one block with its halo (skip = q): 2 K K (q + 1) flops per output over the time
  scalar   engine.whiten_rows on the same array with the same q, one scalar model per component: 1 / K of the arithmetic
  product  N += At At^T of the whitened block through engine.gemm
  whole    NormalEquations.from_accelerations of `blocks` blocks: white, under the scalar models and under the vector model
vector and scalar alternate call by call inside one loop, after 3 warm calls each; medians of R (default 20).  Prints one line per
measurement and a JSON summary line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import acceleration_inputs as ai  # noqa: E402
import grates_amd as ga  # noqa: E402
import vector_noise_reference as vr  # noqa: E402
import whitening_inputs as wi  # noqa: E402

PEAK = 78.6e12        # fp64 FMA rate of the card, flop/s


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def interleaved_ms(calls, repeats, warmup=3):
    """medians of the calls, timed alternately"""
    for fn in calls:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in calls]
    for _ in range(repeats):
        for i, fn in enumerate(calls):
            times[i].append(event_ms(fn))
    return [float(np.median(t)) for t in times]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--degree', type=int, default=96)
    parser.add_argument('--blocks', type=int, default=4)
    args = parser.parse_args()
    ga.engine.require_gpu()
    N, nmin, K = args.degree, 2, 3
    P = (N + 1) ** 2 - nmin ** 2
    block = ga.lstsq.NormalEquations.default_block_points(P, K)
    M = args.blocks * block
    xyz = ga.engine.to_device(ai.scattered_positions(M, N + M))
    g = torch.from_numpy(np.random.default_rng(N).standard_normal((M, K)) * 1e-6).to(xyz.device)
    summary = {'degree': N, 'block': block, 'P': P, 'points': M}
    print('d/o {0}, block {1} points, P {2}, K {3}'.format(N, block, P, K))
    for q in (5, 128):
        vector = ga.lstsq.VectorNoise(vr.synthetic_sequence(ga.lstsq, K, q, 2990 + q))
        scalar = [wi.synthetic_sequence(ga.lstsq, q, 2980 + q + c) for c in range(K)]
        stage = torch.from_numpy(ga.lstsq.arc_stages(None, M, q)).to(xyz.device)
        xb, sb = xyz[block - q:2 * block].contiguous(), stage[block - q:2 * block]      # the second block with its halo
        At = ga.engine.acceleration_design(N, xb, ai.GM, ai.R, nmin)                     # [P, 3, block + q]
        vt, st = ga.engine.to_device(vector.taps()), ga.engine.to_device(ga.lstsq.whitening_taps(scalar))
        out = torch.empty((P, K, block), dtype=torch.float64, device=xyz.device)
        t_vector, t_scalar = interleaved_ms([lambda: ga.engine.whiten_rows_vector(At, vt, sb, skip=q, out=out),
                                             lambda: ga.engine.whiten_rows(At, st, sb, channels=K, skip=q, out=out)], args.repeats)
        flops = 2.0 * P * K * block * K * (q + 1)
        moved = 8.0 * P * K * (2 * block + q)
        flat = out.reshape(P, K * block)
        normals = torch.zeros((P, P), dtype=torch.float64, device=xyz.device)
        product, = interleaved_ms([lambda: ga.engine.gemm(flat, flat, transb=True, beta=1.0, out=normals)], max(args.repeats // 2, 1))
        print('q {0:3d}: vector {1:8.3f} ms  {2:5.1f} TFLOP/s = {3:.2f} of the fp64 peak, {4:.2f} TB/s | scalar {5:8.3f} ms  {6:5.1f} TFLOP/s, '
              '{7:.2f} TB/s | product {8:8.3f} ms'.format(q, t_vector, flops / t_vector / 1e9, flops / t_vector / 1e-3 / PEAK, moved / t_vector / 1e9,
                                                          t_scalar, flops / K / t_scalar / 1e9, moved / t_scalar / 1e9, product))
        summary['q{0}'.format(q)] = {'vector_ms': t_vector, 'scalar_ms': t_scalar, 'product_ms': product, 'vector_TFLOPs': flops / t_vector / 1e9,
                                     'vector_TBps': moved / t_vector / 1e9}
        build = ga.lstsq.NormalEquations.from_accelerations
        white, coloured, coupled = interleaved_ms([lambda: build(xyz, g, nmin, N, ai.GM, ai.R),
                                                   lambda: build(xyz, g, nmin, N, ai.GM, ai.R, noise_model=scalar),
                                                   lambda: build(xyz, g, nmin, N, ai.GM, ai.R, noise_model=vector)], max(args.repeats // 4, 3), warmup=1)
        print('       whole, {0} points: {1:.1f} ms white, {2:.1f} ms scalar models, {3:.1f} ms vector model'.format(M, white, coloured, coupled))
        summary['q{0}'.format(q)].update(whole_white_ms=white, whole_scalar_ms=coloured, whole_vector_ms=coupled)
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
