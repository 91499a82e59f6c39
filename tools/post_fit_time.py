"""The post-fit pass and its kernel, event-timed.
    python3 tools/post_fit_time.py [--repeats R] [--degree 96] [--points 4096] [--arcs 7] [--vectors 100]
At degree N (min_degree 2), `points` points in `arcs` arcs of equal length, the AR(5) model of the test fixture, a bias, a drift and one
period per axis (u' = 4) and S = `vectors` Monte-Carlo vectors:
  whole    lstsq.PostFit.of_accelerations against ArcParameters.from_accelerations of the same arguments
  squares  engine.segment_lag_products at lags = 0 on the (1 + S) 3 rows of the pass: bytes = one read of them, over the time; against
           engine.segment_products at u' = 1 on the same block
  lags     engine.segment_lag_products at lags = 5 and 128 on the 3 residual rows: bytes = one read of them, and the pairs per second
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
    parser.add_argument('--points', type=int, default=4096)
    parser.add_argument('--arcs', type=int, default=7)
    parser.add_argument('--vectors', type=int, default=100)
    args = parser.parse_args()
    ga.engine.require_gpu()
    N, nmin, M, S = args.degree, 2, args.points, args.vectors
    P = (N + 1) ** 2 - nmin ** 2
    arcs = [int(a) for a in np.arange(args.arcs) * (M // args.arcs)]
    noise = wi.sequence(wi.fixture(), 'ar5', ga.lstsq)
    xyz = ga.engine.to_device(ai.scattered_positions(M, N + M))
    rng = np.random.default_rng(N)
    g = torch.from_numpy(rng.standard_normal((M, 3)) * 1e-6).to(xyz.device)
    w = torch.from_numpy(rng.uniform(0.25, 4.0, M)).to(xyz.device)
    model = ga.lstsq.ArcParameters(ga.lstsq.arc_basis(arcs, M, degree=1, periods=(1080,)), arcs, noise)
    ne = model.from_accelerations(xyz, g, nmin, N, ai.GM, ai.R, weights=w)
    x = ne.solve(signs=np.where(rng.integers(0, 2, (P, S)) == 1, 1.0, -1.0))
    Z = ne.monte_carlo_vectors
    whole = max(args.repeats // 3, 1)
    normals = median_ms(lambda: model.from_accelerations(xyz, g, nmin, N, ai.GM, ai.R, weights=w), whole, warmup=1)
    post = median_ms(lambda: ga.lstsq.PostFit.of_accelerations(x, xyz, g, nmin, N, ai.GM, ai.R, weights=w, model=model, vectors=Z), whole, warmup=1)
    bare = median_ms(lambda: ga.lstsq.PostFit.of_accelerations(x, xyz, g, nmin, N, ai.GM, ai.R, weights=w, model=model), whole, warmup=1)
    print('d/o {0}, P {1}, {2} points in {3} arcs, S {4}'.format(N, P, M, len(arcs), S))
    print('whole: normals {0:.1f} ms, post-fit pass {1:.1f} ms ({2:.0f} % of the normals), without vectors {3:.1f} ms'.format(
        normals, post, 100.0 * post / normals, bare))
    summary = {'degree': N, 'points': M, 'arcs': len(arcs), 'vectors': S, 'normals_ms': normals, 'post_fit_ms': post, 'post_fit_no_vectors_ms': bare}

    seg = torch.from_numpy(np.append(arcs, M).astype(np.int32)).to(xyz.device)
    rows = torch.from_numpy(rng.standard_normal(((1 + S) * 3, M))).to(xyz.device)
    read = 8.0 * rows.numel()
    out = torch.empty(((1 + S) * 3, len(arcs), 1), dtype=torch.float64, device=xyz.device)
    squares = median_ms(lambda: ga.engine.segment_lag_products(rows, seg, 0, out=out), args.repeats)
    ones = torch.ones((1, 3, M), dtype=torch.float64, device=xyz.device)
    products = median_ms(lambda: ga.engine.segment_products(rows, ones, seg, channels=3, out=out), args.repeats)
    print("squares  lags=0   {0:8.4f} ms   {1:.3f} TB/s of {2:.1f} MB; segment_products u'=1 {3:8.4f} ms   {4:.3f} TB/s".format(
        squares, read / squares / 1e9, read / 1e6, products, read / products / 1e9))
    summary.update(squares_ms=squares, squares_TBps=read / squares / 1e9, products_u1_ms=products, products_u1_TBps=read / products / 1e9)
    residuals = rows[:3].contiguous()
    for lags in (5, 128):
        out = torch.empty((3, len(arcs), lags + 1), dtype=torch.float64, device=xyz.device)
        lagged = median_ms(lambda: ga.engine.segment_lag_products(residuals, seg, lags, out=out), args.repeats)
        pairs = 3.0 * M * (lags + 1)
        print('lags     lags={0:<3d} {1:8.4f} ms   {2:.4f} TB/s of {3:.2f} MB, {4:.1f} G pairs/s'.format(lags, lagged, 24.0 * M / lagged / 1e9, 24.0 * M / 1e6,
                                                                                                      pairs / lagged / 1e6))
        summary['lags{0}_ms'.format(lags)], summary['lags{0}_TBps'.format(lags)] = lagged, 24.0 * M / lagged / 1e9
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
