"""Whitening of the design matrix inside from_accelerations, event-timed.
    python3 tools/whitening_time.py [--repeats R] [--degree 96] [--blocks 4]
At degree N (min_degree 2) with the default block of points and the AR(5) model of the test fixture, one arc:
  design   engine.acceleration_design of one block with its halo of q points
  whiten   engine.whiten_rows of that block (skip = q): bytes = one read of [P, 3, Mb + q] and one write of [P, 3, Mb], over the time
  product  N += At At^T of the whitened block through engine.gemm
  whole    NormalEquations.from_accelerations of `blocks` blocks, with and without the noise model
Warm-up 2 calls, median of R (default 10).  Prints one line per measurement and a JSON summary line.  Under a kernel trace
(tools/kernel_stats.sh) the per-kernel times of the same calls are what DESIGN.md quotes."""
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
import whitening_inputs as wi  # noqa: E402


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
    parser.add_argument('--degree', type=int, default=96)
    parser.add_argument('--blocks', type=int, default=4)
    args = parser.parse_args()
    ga.engine.require_gpu()
    N, nmin = args.degree, 2
    P = (N + 1) ** 2 - nmin ** 2
    block = ga.lstsq.NormalEquations.default_block_points(P, 3)
    M = args.blocks * block
    model = wi.sequence(wi.fixture(), 'ar5', ga.lstsq)
    taps_host = ga.lstsq.whitening_taps(model)
    q = taps_host.shape[1] - 1
    xyz = ga.engine.to_device(ai.scattered_positions(M, N + M))
    g = torch.from_numpy(np.random.default_rng(N).standard_normal((M, 3)) * 1e-6).to(xyz.device)
    taps = ga.engine.to_device(taps_host)
    stage = torch.from_numpy(ga.lstsq.arc_stages(None, M, q)).to(xyz.device)
    xb, sb = xyz[block - q:2 * block].contiguous(), stage[block - q:2 * block]          # the second block with its halo

    design = median_ms(lambda: ga.engine.acceleration_design(N, xb, ai.GM, ai.R, nmin), args.repeats)
    At = ga.engine.acceleration_design(N, xb, ai.GM, ai.R, nmin)
    out = torch.empty((P, 3, block), dtype=torch.float64, device=xyz.device)
    whiten = median_ms(lambda: ga.engine.whiten_rows(At, taps, sb, skip=q, out=out), args.repeats)
    moved = 8.0 * P * 3 * (2 * block + q)
    flat = out.reshape(P, 3 * block)
    normals = torch.zeros((P, P), dtype=torch.float64, device=xyz.device)
    product = median_ms(lambda: ga.engine.gemm(flat, flat, transb=True, beta=1.0, out=normals), args.repeats)
    build = ga.lstsq.NormalEquations.from_accelerations
    plain = median_ms(lambda: build(xyz, g, nmin, N, ai.GM, ai.R), max(args.repeats // 3, 1), warmup=1)
    whitened = median_ms(lambda: build(xyz, g, nmin, N, ai.GM, ai.R, noise_model=model), max(args.repeats // 3, 1), warmup=1)
    print('d/o {0}, block {1} points (+ {2}), P {3}'.format(N, block, q, P))
    print('design  {0:8.3f} ms'.format(design))
    print('whiten  {0:8.3f} ms   {1:.2f} TB/s of {2:.0f} MB'.format(whiten, moved / whiten / 1e9, moved / 1e6))
    print('product {0:8.3f} ms   {1:.1f} TFLOP/s'.format(product, 2.0 * 3 * block * P * P / product / 1e9))
    print('whole, {0} points: {1:.1f} ms white, {2:.1f} ms with the noise model'.format(M, plain, whitened))
    print(json.dumps({'degree': N, 'block': block, 'q': q, 'design_ms': design, 'whiten_ms': whiten, 'whiten_TBps': moved / whiten / 1e9,
                      'product_ms': product, 'whole_white_ms': plain, 'whole_whitened_ms': whitened, 'points': M}))


if __name__ == '__main__':
    main()
