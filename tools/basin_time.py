"""Basin masks and basin statistics, event-timed.
    python3 tools/basin_time.py [--repeats R]
(a) the point-in-polygon mask of the 2000-vertex, 0.5-rad star of the fixtures (tests/golden/basin_inputs.py) on a 0.25-degree grid:
    Grid.create_mask(as_tensor=True), host tables included, and the device part alone;
(b) Grid.basin_statistics on 240 x 0.25-degree grids for B = 1, 16 (disjoint and overlapping), 64: the two passes over the series
    (mean / rms, then std) with their reductions; effective rate = bytes of the series read (2 x T x P x 8) over the time, against
    the 8 TB/s of the HBM.
Prints one line per measurement and a JSON summary line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import basin_inputs as bi  # noqa: E402
import grates_amd as ga  # noqa: E402

HBM = 8.0e12


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    grid = ga.grid.GeographicGrid(0.25, 0.25)
    P = grid.point_count
    result = {'device': torch.cuda.get_device_name(0), 'points': P}

    # (a) mask
    basin = ga.grid.Basin(bi.polygons()['star2000'])
    mask = grid.create_mask(basin, as_tensor=True)
    points = grid._mask_points()
    pip = [ga.grid._pip_tables(basin._Basin__polygons[0], ga.grid._A, ga.grid._F)]
    med, best = timed(lambda: ga.engine.polygon_mask(points, pip), args.repeats)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        grid.create_mask(basin, as_tensor=True)
    torch.cuda.synchronize()
    call_ms = (time.perf_counter() - t0) / 5 * 1e3
    inside = int(mask.sum().item())
    print('mask  star2000 (2000 edges) on 0.25 deg: {0} of {1} points inside; device {2:.3f} ms (best {3:.3f}); '
          'create_mask call {4:.3f} ms'.format(inside, P, med, best, call_ms), flush=True)
    result['mask'] = {'edges': 2000, 'inside': inside, 'device_ms': med, 'device_best_ms': best, 'call_ms': call_ms}

    # (b) statistics
    T, N = 240, 96
    gen = torch.Generator(device='cuda').manual_seed(5)
    batch = torch.randn((T, N + 1, N + 1), dtype=torch.float64, device='cuda', generator=gen) * 1e-10
    values = ga.gravityfield.synthesize(batch, grid, 'ewh').reshape(T, P)
    del batch
    nlat, nlon = grid.parallels.size, grid.meridians.size
    lat_idx = torch.arange(nlat, device='cuda')[:, None].expand(nlat, nlon).reshape(-1)
    lon_idx = torch.arange(nlon, device='cuda')[None, :].expand(nlat, nlon).reshape(-1)
    sector, band = lon_idx * 16 // nlon, lat_idx * 4 // nlat
    cases = {'B1': torch.ones((1, P), dtype=torch.bool, device='cuda'),
             'B16': torch.stack([sector == b for b in range(16)]),
             'B16_overlap': torch.stack([(sector == b) | (band == b % 4) for b in range(16)]),
             'B64': torch.stack([(sector == b % 16) & (band == b // 16) for b in range(64)])}
    w = ga.engine.to_device(grid.area)
    bytes_read = 2.0 * T * P * 8
    result['statistics'] = {}
    for tag, m in cases.items():
        bits = ga.engine.pack_masks(m)
        out = ga.engine.basin_statistics(values, w, bits, m.shape[0])
        med, best = timed(lambda: ga.engine.basin_statistics(values, w, bits, m.shape[0]), args.repeats)
        rate = bytes_read / (med * 1e-3)
        print('stats {0:12s} T={1} P={2}: {3:.3f} ms (best {4:.3f}), {5:.2f} TB/s effective = {6:.0%} of 8 TB/s; '
              'checksum {7:.12e}'.format(tag, T, P, med, best, rate / 1e12, rate / HBM, float(out[0].sum().item())), flush=True)
        result['statistics'][tag] = {'masks': m.shape[0], 'ms': med, 'best_ms': best, 'TBps': rate / 1e12, 'fraction_of_8TBps': rate / HBM}
    print(json.dumps(result))


if __name__ == '__main__':
    main()
