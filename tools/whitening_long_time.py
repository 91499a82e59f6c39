"""shg_whiten_rows_long against the routes that exist without it, event-timed.
    python3 tools/whitening_long_time.py [--rounds R] [--orders 128 512 2159 4095] [--output profiles/whitening_long_time.txt]
The d/o 96 block of accelerations: P = 9405 parameters, K = 3 components, Mb = 1024 points with a halo of q points in front, so
X [28215, q + 1024] and Y [28215, 1024]; the taps of the covariance function of the tests at order q, every column stationary
(stage = q: a block in the middle of a long arc).  Per order q:
  long     shg_whiten_rows_long on X
  chain    shg_whiten_rows on the same operands (q <= 128 only: the one point where the two kernels meet)
  staged   what exists without the kernel: an explicit banded B [q + 1024, 1024] per channel (built once, not timed) and one
           engine.gemm per channel on the rows of that channel, the full product over the band
  normals  the block's N += At At^T on the whitened block, engine.gemm(Y, Y, transb=True) with Y as [9405, 3072]
The routes alternate inside one process on one device, warm-up 2 rounds, then R rounds (default 9); per route the median and the
minimum, TFLOP/s of the whitening routes counted as 2 rows Mb (q + 128) over the median.  Prints one line per order and a JSON summary
line, and writes both to --output."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import grates_amd as ga  # noqa: E402
from grates_amd import _lib  # noqa: E402

P, K, MB = 9405, 3, 1024


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def covariance(count):
    k = np.arange(count, dtype=np.float64)
    c = 0.5 * 0.9 ** k + 0.5 * np.cos(2.0 * np.pi * k / 50.0) * 0.99 ** k
    c[0] += 0.1
    return c


def entry(name, X, taps, stage, skip, Y):
    _lib.call(name, int(X.shape[0]), K, int(X.shape[1]), ga.engine._ptr(X), int(X.stride(0)), ga.engine._ptr(stage), ga.engine._ptr(taps),
              int(taps.shape[-1]) - 1, skip, ga.engine._ptr(Y), int(Y.stride(0)), ga.engine._stream())


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=9)
    parser.add_argument('--orders', type=int, nargs='+', default=[128, 512, 2159, 4095])
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'whitening_long_time.txt'))
    args = parser.parse_args()
    ga.engine.require_gpu()
    lines, summary = [], []
    for q in args.orders:
        M = q + MB
        generator = torch.Generator(device='cuda').manual_seed(q)
        X = torch.randn((P * K, M), dtype=torch.float64, device='cuda', generator=generator)
        row = ga.lstsq.CovarianceFunction(covariance(q + 1)).taps()
        taps = ga.engine.to_device(np.repeat(row[None], K, axis=0))
        stage = torch.full((M,), q, dtype=torch.int32, device='cuda')
        Y, Z = (torch.empty((P * K, MB), dtype=torch.float64, device='cuda') for _ in range(2))
        N = torch.empty((P, P), dtype=torch.float64, device='cuda')
        lag = (q + torch.arange(MB, device='cuda'))[None, :] - torch.arange(M, device='cuda')[:, None]                  # t - t' of B[t'][t]
        band = torch.where((lag >= 0) & (lag <= q), taps[0, q][lag.clamp(0, q)], torch.zeros((), dtype=torch.float64, device='cuda'))
        B = band[None].repeat(K, 1, 1)
        X3, Z3 = X.view(P, K, M), Z.view(P, K, MB)

        def long_route():
            entry('shg_whiten_rows_long', X, taps, stage, q, Y)

        def chain_route():
            entry('shg_whiten_rows', X, taps, stage, q, Z)

        def staged_route():
            for c in range(K):
                ga.engine.gemm(X3[:, c, :], B[c], out=Z3[:, c, :])

        def normals_route():
            ga.engine.gemm(Y.view(P, K * MB), Y.view(P, K * MB), transb=True, out=N)
        routes = {'long': long_route, 'staged': staged_route, 'normals': normals_route}
        if q <= 128:
            routes['chain'] = chain_route
        record = {'order': q, 'rows': P * K, 'block_points': MB}
        for _ in range(2):
            for name, route in routes.items():
                route()
                if name in ('staged', 'chain'):
                    torch.cuda.synchronize()
                    record[name + '_deviation'] = float(((Y - Z).abs().max() / Y.abs().max()).item())
        times = {name: [] for name in routes}
        for _ in range(args.rounds):
            for name, route in routes.items():
                times[name].append(event_ms(route))
        flop = 2.0 * P * K * MB * (q + 128)
        for name, values in times.items():
            record[name + '_ms'] = round(float(np.median(values)), 4)
            record[name + '_min_ms'] = round(float(np.min(values)), 4)
            if name != 'normals':
                record[name + '_tflops'] = round(flop / np.median(values) * 1e-9, 2)
        record['share_of_normals'] = round(record['long_ms'] / record['normals_ms'], 4)
        line = 'q {order}: long {long_ms} ms (min {long_min_ms}, {long_tflops} TFLOP/s)'.format(**record)
        if 'chain' in routes:
            line += ', chain {chain_ms} ms (min {chain_min_ms}, {chain_tflops} TFLOP/s; differs by {chain_deviation:.1e})'.format(**record)
        line += (', staged {staged_ms} ms (min {staged_min_ms}, {staged_tflops} TFLOP/s; differs by {staged_deviation:.1e}), normals {normals_ms} ms '
                 '(min {normals_min_ms}): the kernel is {share_of_normals} of the product').format(**record)
        print(line, flush=True)
        lines.append(line)
        summary.append(record)
        del X, Y, Z, B, band, lag, N
        torch.cuda.empty_cache()
    lines.append(json.dumps({'whitening_long_time': summary, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0)}))
    print(lines[-1])
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
