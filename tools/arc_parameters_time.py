"""Elimination of arc-wise parameters inside from_accelerations, event-timed.
    python3 tools/arc_parameters_time.py [--repeats R] [--degree 96] [--blocks 4] [--arc 600]
At degree N (min_degree 2) with the default block of points, the AR(5) model of the test fixture and arcs of `arc` points:
  segment  engine.segment_products of one whitened block of At with its arc boundaries, u' = 2, 4 and 16: bytes = one read of
           [P, 3, Mb], over the time
  whiten   engine.whiten_rows of the same block (skip = q), which reads and writes it: twice the bytes
  update   N -= D D^T through engine.gemm for 24 and for 256 columns of D: one read and one write of N [P, P]
  whole    NormalEquations.from_accelerations of `blocks` blocks under ColouredNoise alone and under ArcParameters with a bias, a
           drift and one period per axis (u' = 4)
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
    parser.add_argument('--arc', type=int, default=600)
    args = parser.parse_args()
    ga.engine.require_gpu()
    N, nmin = args.degree, 2
    P = (N + 1) ** 2 - nmin ** 2
    block = ga.lstsq.NormalEquations.default_block_points(P, 3)
    M = args.blocks * block
    arcs = list(range(0, M, args.arc))
    model = wi.sequence(wi.fixture(), 'ar5', ga.lstsq)
    taps_host = ga.lstsq.whitening_taps(model)
    q = taps_host.shape[1] - 1
    xyz = ga.engine.to_device(ai.scattered_positions(M, N + M))
    g = torch.from_numpy(np.random.default_rng(N).standard_normal((M, 3)) * 1e-6).to(xyz.device)
    taps = ga.engine.to_device(taps_host)
    stage = torch.from_numpy(ga.lstsq.arc_stages(arcs, M, q)).to(xyz.device)
    xb, sb = xyz[block - q:2 * block].contiguous(), stage[block - q:2 * block]          # the second block with its halo

    At = ga.engine.acceleration_design(N, xb, ai.GM, ai.R, nmin)
    out = torch.empty((P, 3, block), dtype=torch.float64, device=xyz.device)
    whiten = median_ms(lambda: ga.engine.whiten_rows(At, taps, sb, skip=q, out=out), args.repeats)
    bounds = np.append(np.asarray(arcs), M)
    cut = np.clip(bounds[(bounds > block) & (bounds < 2 * block)], block, 2 * block) - block
    seg = torch.from_numpy(np.concatenate(([0], cut, [block])).astype(np.int32)).to(xyz.device)
    read = 8.0 * P * 3 * block
    summary = {'degree': N, 'block': block, 'q': q, 'points': M, 'arc': args.arc, 'segments': int(seg.numel()) - 1, 'whiten_ms': whiten,
               'whiten_TBps': 2 * read / whiten / 1e9}
    print('d/o {0}, block {1} points, P {2}, {3} segments in the block'.format(N, block, P, int(seg.numel()) - 1))
    print('whiten       {0:8.3f} ms   {1:.2f} TB/s of {2:.0f} MB'.format(whiten, 2 * read / whiten / 1e9, 2 * read / 1e6))
    for u in (2, 4, 16):
        Bt = torch.from_numpy(np.random.default_rng(u).standard_normal((u, 3, block))).to(xyz.device)
        S = torch.empty((P, 3, int(seg.numel()) - 1, u), dtype=torch.float64, device=xyz.device)
        segment = median_ms(lambda: ga.engine.segment_products(out, Bt, seg, channels=3, out=S), args.repeats)
        print("segment u'={0:<2d} {1:8.3f} ms   {2:.2f} TB/s of {3:.0f} MB".format(u, segment, read / segment / 1e9, read / 1e6))
        summary['segment_ms_u{0}'.format(u)], summary['segment_TBps_u{0}'.format(u)] = segment, read / segment / 1e9
    flat = out.reshape(P, 3 * block)
    normals = torch.zeros((P, P), dtype=torch.float64, device=xyz.device)
    product = median_ms(lambda: ga.engine.gemm(flat, flat, transb=True, beta=1.0, out=normals), args.repeats)
    print('product      {0:8.3f} ms   {1:.1f} TFLOP/s'.format(product, 2.0 * 3 * block * P * P / product / 1e9))
    for width in (24, 256):                                                              # N -= D D^T: two arcs of u' = 4 per axis, and a full batch
        D = torch.from_numpy(np.random.default_rng(width).standard_normal((P, width))).to(xyz.device)
        update = median_ms(lambda: ga.engine.gemm(D, D, transb=True, alpha=-1.0, beta=1.0, out=normals), args.repeats)
        print('update {0:4d}  {1:8.3f} ms   {2:.2f} TB/s for one read and one write of N'.format(width, update, 16.0 * P * P / update / 1e9))
        summary['update_ms_{0}'.format(width)] = update
    del normals, At, out, flat

    basis = ga.lstsq.arc_basis(arcs, M, degree=1, periods=(1080,))
    coloured = ga.lstsq.ColouredNoise(model, arcs)
    whole = max(args.repeats // 3, 1)
    whitened = median_ms(lambda: coloured.from_accelerations(xyz, g, nmin, N, ai.GM, ai.R), whole, warmup=1)
    for keep in (False, True):
        params = ga.lstsq.ArcParameters(basis, arcs, model, keep=keep)
        reduced = median_ms(lambda: params.from_accelerations(xyz, g, nmin, N, ai.GM, ai.R), whole, warmup=1)
        print('whole, {0} points in {1} arcs: {2:.1f} ms under ColouredNoise, {3:.1f} ms under ArcParameters(keep={4}): {5:+.1f} %'.format(
            M, len(arcs), whitened, reduced, keep, 100.0 * (reduced / whitened - 1.0)))
        summary['whole_reduced_ms_keep{0}'.format(int(keep))] = reduced
    summary.update(product_ms=product, whole_whitened_ms=whitened)
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
