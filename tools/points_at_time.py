"""Gravitational acceleration of time-variable fields along an orbit, every point at its own epoch, event-timed.
    python3 tools/points_at_time.py [--repeats R] [--degrees 96 180] [--output profiles/points_at_time.txt]
At each degree N, M = 1 M time-ordered positions:
  series     a device series of 248 fields (a month of 3-hourly fields), W = 2: TimeSeries.gravitational_acceleration_at with modified
             Julian dates (host weights and runs, upload, one shg_acceleration_points_at_om call), engine.acceleration_points_at with the
             weights on the device (host runs, the call), and the call alone with the run tables built before
  model      a trend, an annual and a semi-annual cycle as one batch of 5 fields, W = 5, one run: engine.acceleration_points_at
  floor      engine.acceleration_points with B = 2 at the same points: one sweep of the column recursion, the least the series can cost
  cross      what the package offered before: the [T, M, 3] call in slices of 16 epochs, then the gather of the two fields of every
             point and their blend in torch, on every 16th point and scaled by 16
Prints one line per measurement and a JSON summary line with the commit and the hashes of the kernel sources."""
import argparse
import datetime
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
from grates_amd import _lib  # noqa: E402

M, FIELDS, SUBSET = 1_000_000, 248, 16
START, STEP = datetime.datetime(2008, 1, 1), datetime.timedelta(hours=3)


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
    parser.add_argument('--repeats', type=int, default=7)
    parser.add_argument('--degrees', type=int, nargs='+', default=[96, 180])
    parser.add_argument('--output', default=None)
    args = parser.parse_args()
    ga.engine.require_gpu()
    dev = ga.engine.device()
    lines, rows = [], []

    def report(text):
        print(text, flush=True)
        lines.append(text)

    nodes = [START + k * STEP for k in range(FIELDS)]
    mjd = np.linspace(ga.utilities._mjd(nodes[0]), ga.utilities._mjd(nodes[-1]), M)
    for N in args.degrees:
        rng = np.random.default_rng(N)
        batch = torch.from_numpy(rng.standard_normal((FIELDS, N + 1, N + 1)) * 1e-10).to(dev)
        series = ga.gravityfield.TimeSeries.from_series(ga.engine.OrderMajorSeries.from_batch(batch), nodes, ai.GM, ai.R)
        om = series.to_device()
        xyz = ga.engine.to_device(ai.scattered_positions(M, N + M))
        first, weights = series.interpolation_windows(mjd)
        w = ga.engine.to_device(weights)
        order, run_first, run_begin = ga.engine.points_at_plan(first)
        assert order is None
        out = torch.empty((M, 3), dtype=torch.float64, device=dev)

        def call_alone():
            _lib.call('shg_acceleration_points_at_om', N, ga.engine._ptr(xyz), M, ga.engine._ptr(om.data), FIELDS, om.padded_epochs,
                      ga.engine._host_ptr(run_first), ga.engine._host_ptr(run_begin), len(run_first), ga.engine._ptr(w), 2, ai.GM, ai.R,
                      ga.engine._ptr(out), ga.engine._stream())
        public = median_ms(lambda: series.gravitational_acceleration_at(xyz, mjd, as_tensor=True), args.repeats)
        engine = median_ms(lambda: ga.engine.acceleration_points_at(N, xyz, om, first, w, ai.GM, ai.R), args.repeats)
        alone = median_ms(call_alone, args.repeats)
        floor = median_ms(lambda: ga.engine.acceleration_points(N, xyz, batch[:2], ai.GM, ai.R), args.repeats)
        model_w = ga.engine.to_device(rng.standard_normal((M, 5)))
        zeros = np.zeros(M, dtype=np.int64)
        model = median_ms(lambda: ga.engine.acceleration_points_at(N, xyz, batch[:5], zeros, model_w, ai.GM, ai.R), args.repeats)

        sub = xyz[::SUBSET].contiguous()
        rows_sub = torch.arange(sub.shape[0], device=dev)
        first_sub = torch.from_numpy(first[::SUBSET]).to(dev)
        w_sub = w[::SUBSET].contiguous()

        def cross():
            g = torch.cat([ga.engine.acceleration_points(N, sub, batch[s:s + 16], ai.GM, ai.R) for s in range(0, FIELDS, 16)])
            return w_sub[:, :1] * g[first_sub, rows_sub] + w_sub[:, 1:] * g[first_sub + 1, rows_sub]
        cross_ms = SUBSET * median_ms(cross, max(args.repeats // 2, 2), warmup=1)
        same = float((cross() - ga.engine.acceleration_points_at(N, sub, om, first[::SUBSET], w_sub, ai.GM, ai.R)).abs().max() /
                     cross().abs().max())
        rows.append({'degree': N, 'points': M, 'fields': FIELDS, 'runs': int(len(run_first)), 'public_ms': public, 'engine_ms': engine, 'call_ms': alone,
                     'floor_ms': floor, 'model_ms': model, 'cross_ms': cross_ms, 'call_over_floor': alone / floor, 'engine_over_floor': engine / floor,
                     'model_over_floor': model / floor, 'cross_over_call': cross_ms / alone, 'cross_difference_of_max': same})
        size = 'd/o {0:3d} M {1} fields {2}'.format(N, M, FIELDS)
        report('series {0}: the call alone {1:9.3f} ms = {2:.2f} x the floor; engine.acceleration_points_at {3:9.3f} ms ({4:.2f} x); '
               'TimeSeries.gravitational_acceleration_at {5:9.3f} ms'.format(size, alone, alone / floor, engine, engine / floor, public))
        report('model  d/o {0:3d} M {1} fields 5 (W = 5, one run): {2:9.3f} ms = {3:.2f} x the floor'.format(N, M, model, model / floor))
        report('floor  d/o {0:3d} M {1}: engine.acceleration_points with B = 2 {2:9.3f} ms'.format(N, M, floor))
        report('cross  {0}: [T, M, 3] in slices of 16, gather and blend {1:9.3f} ms (every {2}th point x {2}) = {3:.1f} x the call; the two differ '
               'by {4:.1e} of the largest value'.format(size, cross_ms, SUBSET, cross_ms / alone, same))
        del batch, series, om, xyz, w, out, model_w, sub
        torch.cuda.empty_cache()
    summary = json.dumps({'commit': source_hashes.commit(),
                          'sources': {name: source_hashes.file_hash(name) for name in ('common.h', 'solid.h', 'gravity_points.hip')},
                          'points_at': rows})
    report(summary)
    if args.output:
        with open(args.output, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
