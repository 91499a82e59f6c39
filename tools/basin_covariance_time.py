"""Basin functionals, basin covariances and basin averages, event-timed.
    python3 tools/basin_covariance_time.py [--repeats R]
(a) engine.basin_covariance(F, Sigma) at d/o 180 (Pn = 32761) for B = 1, 16, 64 and at d/o 96 (Pn = 9409) for B = 16, 64, alternating call
    by call with engine.congruence(F, Sigma) in the same process; bound = max(triangle bytes / 8 TB/s, triangle flop / 78.6 TFLOP/s) with
    bytes = 8 Pn (Pn + 1) / 2 and flop = 2 B Pn (Pn + 1) / 2;
(b) Grid.basin_functionals on a 0.25-degree grid, d/o 96, B = 64, end to end;
(c) Grid.basin_averages of 240 epochs at d/o 96 (device series) for B = 16, 64, next to to_grid + basin_statistics for the same output.
Prints one line per measurement and a JSON summary line."""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import grates_amd as ga  # noqa: E402

HBM, MFMA = 8.0e12, 78.6e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternating(fns, repeats, warmup=2):
    """median ms of every function, the calls interleaved"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            times[k].append(event_ms(fn))
    return [float(np.median(t)) for t in times]


def box_masks(grid, B, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        lon0, lat0 = rng.uniform(-175, 150), rng.uniform(-85, 60)
        out.append(grid.create_mask(ga.grid.Basin.from_extent(*np.deg2rad([lon0, lat0, lon0 + rng.uniform(5, 25), lat0 + rng.uniform(5, 25)]))))
    return np.array(out)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--covariance-only', action='store_true', help='(a) only, without congruence: the run of the counter passes')
    args = parser.parse_args()
    ga.engine.require_gpu()
    summary = {'covariance': [], 'functionals': None, 'averages': []}
    dev = ga.engine.device()
    for N, Bs in ((180, (1, 16, 64)), (96, (16, 64))):
        Pn = (N + 1) ** 2
        gen = torch.Generator(device=dev).manual_seed(N)
        S = torch.randn((Pn, Pn), dtype=torch.float64, device=dev, generator=gen)
        for B in Bs:
            F = torch.randn((B, Pn), dtype=torch.float64, device=dev, generator=gen)
            if args.covariance_only:
                alternating([lambda: ga.engine.basin_covariance(F, S)], args.repeats)
                print('basin_covariance d/o {0} B {1}: {2} calls'.format(N, B, args.repeats + 2), flush=True)
                continue
            ms, ms_cong = alternating([lambda: ga.engine.basin_covariance(F, S), lambda: ga.engine.congruence(F, S)], args.repeats)
            tri = Pn * (Pn + 1) / 2
            bound = max(8 * tri / HBM, 2 * B * tri / MFMA) * 1e3
            row = {'degree': N, 'Pn': Pn, 'B': B, 'ms': ms, 'bound_ms': bound, 'fraction_of_bound': bound / ms, 'congruence_ms': ms_cong,
                   'speedup_vs_congruence': ms_cong / ms, 'bound': 'HBM' if 8 * tri / HBM >= 2 * B * tri / MFMA else 'MFMA'}
            summary['covariance'].append(row)
            print('basin_covariance d/o {0:3d} Pn {1:6d} B {2:2d}: {3:8.3f} ms  bound {4:.3f} ms ({5}) -> {6:.2f} of it;  congruence {7:8.3f} ms ({8:.1f}x)'.format(
                N, Pn, B, ms, bound, row['bound'], row['fraction_of_bound'], ms_cong, row['speedup_vs_congruence']), flush=True)
            del F
        del S
        torch.cuda.empty_cache()
    if args.covariance_only:
        return

    grid = ga.grid.GeographicGrid(0.25, 0.25)
    N = 96
    masks64 = box_masks(grid, 64, 3)
    masks_dev = torch.as_tensor(masks64, device=dev)
    grid.basin_functionals(masks_dev, 0, N)
    ms = alternating([lambda: grid.basin_functionals(masks_dev, 0, N)], args.repeats)[0]
    summary['functionals'] = {'grid': '0.25 deg', 'degree': N, 'B': 64, 'ms': ms}
    print('basin_functionals 0.25 deg d/o {0} B 64: {1:.3f} ms'.format(N, ms), flush=True)

    T = 240
    rng = np.random.default_rng(9)
    x = rng.standard_normal((T, N + 1, N + 1)) * 1e-10
    epochs = [datetime.datetime(2002, 1, 1) + datetime.timedelta(days=30 * k) for k in range(T)]
    series = ga.gravityfield.TimeSeries.from_series(x, epochs)
    for B in (16, 64):
        m = masks_dev[:B].contiguous()
        ms_avg, ms_grid = alternating([lambda: grid.basin_averages(series, m),
                                       lambda: grid.basin_statistics(series.to_grid(grid, 'ewh', as_tensor=True), m)], args.repeats)
        summary['averages'].append({'epochs': T, 'degree': N, 'B': B, 'ms': ms_avg, 'grid_path_ms': ms_grid})
        print('basin_averages {0} epochs d/o {1} B {2:2d}: {3:.3f} ms;  to_grid + basin_statistics {4:.3f} ms'.format(T, N, B, ms_avg, ms_grid), flush=True)
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
