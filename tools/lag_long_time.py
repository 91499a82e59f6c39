"""shg_segment_lag_products_long against the routes that exist without it, event-timed.
    python3 tools/lag_long_time.py [--rounds R] [--lags 128 512 2159 4095] [--staged-arcs A] [--output profiles/lag_long_time.txt]
The residuals of a month at 5 s: rows = 3, M = 518 400 columns.  Two segment tables: `month`, 240 arcs of 2160 columns (3 h), and
`single`, the same columns as one arc, where all parallelism comes from the chunks.  Per table and lags:
  long     shg_segment_lag_products_long
  chain    shg_segment_lag_products on the same operands (lags = 128 only: the one point where a route of the parent exists)
  staged   what exists without the kernel, in this tool only (month only): per row and arc the matrix of shifted copies [lags + 1, 2160]
           (stored transposed, zeros behind the arc, built once, not timed), and one engine.gemm of the arc with it.  The matrices of
           all 720 (row, arc) pairs at lags = 4095 are 51 GB, so the route is timed on the first --staged-arcs arcs (default 24) and
           scaled to 240 by the factor printed: an extrapolation along a loop of equal steps, marked as such
The routes alternate inside one process on one device, warm-up 2 rounds, then R rounds (default 9); per route the median and the
minimum.  TFLOP/s of `long` counted as 2 rows M (lags + 1) over the median, and that time against the 78.6 TFLOP/s of the fp64 MFMA.
Prints one line per case and a JSON summary line, and writes both to --output.  No counters are taken here."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import grates_amd as ga  # noqa: E402

ROWS, ARCS, ARC = 3, 240, 2160
M = ARCS * ARC
PEAK_TFLOPS = 78.6


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--rounds', type=int, default=9)
    parser.add_argument('--lags', type=int, nargs='+', default=[128, 512, 2159, 4095])
    parser.add_argument('--staged-arcs', type=int, default=24)
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'lag_long_time.txt'))
    args = parser.parse_args()
    ga.engine.require_gpu()
    X = torch.randn((ROWS, M), dtype=torch.float64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4260))
    tables = {'month': torch.arange(0, M + 1, ARC, dtype=torch.int32, device='cuda'), 'single': torch.tensor([0, M], dtype=torch.int32, device='cuda')}
    lines, summary = [], []
    for table, seg in tables.items():
        nseg = int(seg.numel()) - 1
        for lags in args.lags:
            S = torch.empty((ROWS, nseg, lags + 1), dtype=torch.float64, device='cuda')
            routes = {'long': lambda: ga.engine.segment_lag_products_long(X, seg, lags, out=S)}
            record = {'table': table, 'lags': lags, 'rows': ROWS, 'columns': M, 'segments': nseg}
            if lags <= 128:
                C = torch.empty_like(S)
                routes['chain'] = lambda: ga.engine.segment_lag_products(X, seg, lags, out=C)
            if table == 'month':
                staged_arcs = min(args.staged_arcs, ARCS)
                padded = torch.zeros((ROWS, staged_arcs, ARC + lags), dtype=torch.float64, device='cuda')
                padded[:, :, :ARC] = X[:, :staged_arcs * ARC].reshape(ROWS, staged_arcs, ARC)
                shifted = padded.as_strided((ROWS, staged_arcs, ARC, lags + 1), (padded.stride(0), padded.stride(1), 1, 1)).contiguous()      # [t][k] = x[t + k]
                values = X[:, :staged_arcs * ARC].reshape(ROWS, staged_arcs, 1, ARC).contiguous()
                G = torch.empty((ROWS, staged_arcs, 1, lags + 1), dtype=torch.float64, device='cuda')

                def staged_route():
                    for r in range(ROWS):
                        for a in range(staged_arcs):
                            ga.engine.gemm(values[r, a], shifted[r, a], out=G[r, a])
                routes['staged'] = staged_route
                record['staged_arcs'], record['staged_scale'] = staged_arcs, ARCS / staged_arcs
            for _ in range(2):
                for route in routes.values():
                    route()
            torch.cuda.synchronize()
            scale = S.abs().amax()
            if 'chain' in routes:
                record['chain_deviation'] = float(((S - C).abs().amax() / scale).item())
            if 'staged' in routes:
                record['staged_deviation'] = float(((S[:, :staged_arcs] - G[:, :, 0]).abs().amax() / scale).item())
            times = {name: [] for name in routes}
            for _ in range(args.rounds):
                for name, route in routes.items():
                    times[name].append(event_ms(route))
            for name, samples in times.items():
                factor = record['staged_scale'] if name == 'staged' else 1.0
                record[name + '_ms'] = round(float(np.median(samples)) * factor, 4)
                record[name + '_min_ms'] = round(float(np.min(samples)) * factor, 4)
            flop = 2.0 * ROWS * M * (lags + 1)
            record['long_tflops'] = round(flop / record['long_ms'] * 1e-9, 2)
            record['roof_ms'] = round(flop / PEAK_TFLOPS * 1e-9, 4)
            record['long_over_roof'] = round(record['long_ms'] / record['roof_ms'], 2)
            line = '{table}, lags {lags}: long {long_ms} ms (min {long_min_ms}; {long_tflops} TFLOP/s counted, {long_over_roof} x the {roof_ms} ms of the roof)'.format(**record)
            if 'chain' in routes:
                line += ', chain {chain_ms} ms (min {chain_min_ms}; differs by {chain_deviation:.1e})'.format(**record)
            if 'staged' in routes:
                line += (', staged {staged_ms} ms (min {staged_min_ms}; {staged_arcs} arcs timed, times {staged_scale:g}: extrapolated; differs by '
                         '{staged_deviation:.1e})').format(**record)
            print(line, flush=True)
            lines.append(line)
            summary.append(record)
            routes.clear()
            S = C = G = shifted = padded = values = None
            torch.cuda.empty_cache()
    lines.append(json.dumps({'lag_long_time': summary, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0), 'counters': 'none taken'}))
    print(lines[-1])
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
