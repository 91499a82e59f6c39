"""From node values of radial basis functions to a map and its formal errors, the surface route against the route through spherical
harmonics, event-timed.
    python3 tools/rbf_surface_time.py [--repeats R] [--output profiles/rbf_surface_time.txt]
At each size (band 2 .. N, J scattered nodes on GRS80 with flat shape factors, a seeded covariance matrix C = B B^T / J of the node
values, the 0.25 degree grid of a 40 x 40 degree box as a point list: 25600 points, ewh):
  surface sigma    RadialBasisFunctions.covariance_propagation(grid, C): per block of points shg_rbf_surface, C St on engine.gemm,
                   shg_column_dots and the square root; C resident on the device
  surface values   RadialBasisFunctions.synthesize(grid): shg_rbf_surface and one engine.gemm row per block
  St alone         engine.rbf_surface of the first block of that size, with its fp64 operations (8 per degree and pair: 6
                   multiplications and 2 additions, none fused) over the time, as a fraction of the 78.6 TFLOP/s fp64 vector peak
                   counted in fused operations
  block            of that block: C St on engine.gemm, shg_column_dots of St and C St, one row of values times St on engine.gemm
  series           synthesize of 32 solutions [32, J] in one pass; on the other side 32 times `harmonic values`
  harmonic sigma   what the package offered before: engine.congruence(F, C) with F = to_potential_coefficients_matrix() resident on
                   the device ([P, P], P = (N + 1)^2 - 4), then IrregularGrid.covariance_propagation of it (shg_covprop_points)
  harmonic values  to_potential_coefficients().to_grid(grid)
  F                forming F itself (to_potential_coefficients_matrix, host result), once per basis: not part of `harmonic sigma`
Warm-up 2 calls, median of R (default 10).  Prints one line per measurement and a JSON summary line, and writes both to --output."""
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

import grates_amd as ga  # noqa: E402
import rbf_inputs as ri  # noqa: E402
import rbf_surface_inputs as si  # noqa: E402

PEAK = 78.6e12
SIZES = ((60, 3600), (96, 9000))                      # (max degree, nodes)
KERNEL = 'ewh'
SERIES = 32                                           # solutions of the series rows


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


def box_grid(step=0.25, west=0.0, south=10.0, extent=40.0):
    """the pixel centres of a geographic grid of `step` degrees over a box, parallel by parallel from the north, as a point list"""
    count = int(round(extent / step))
    lon = np.deg2rad(west + step * (np.arange(count) + 0.5))
    lat = np.deg2rad(south + extent - step * (np.arange(count) + 0.5))
    return ga.grid.IrregularGrid(np.tile(lon, count), np.repeat(lat, count), a=si.A, f=si.F)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=10)
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'rbf_surface_time.txt'))
    args = parser.parse_args()
    ga.engine.require_gpu()
    rows, lines = [], []

    def report(line):
        print(line, flush=True)
        lines.append(line)

    nmin = 2
    grid = box_grid()
    M = grid.point_count
    for N, J in SIZES:
        P = (N + 1) ** 2 - nmin ** 2
        lon, lat = ri.scattered_nodes(J, N + J)
        basis = ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat, a=si.A, f=si.F), ri.shape_factors(ri.degree_factors(nmin, N, flat=True)),
                                                     nmin, N, si.GM, si.R)
        basis.values = np.random.default_rng(N + J + 1).standard_normal(J)
        B = ga.engine.to_device(np.random.default_rng(N + J + 2).standard_normal((J, J)))
        C = ga.engine.gemm(B, B, transb=True, alpha=1.0 / J)
        del B
        size = 'band {0}..{1:3d} J {2:5d} M {3:5d}'.format(nmin, N, J, M)

        sigma = basis.covariance_propagation(grid, C, KERNEL, as_tensor=True)
        surface_sigma = median_ms(lambda: basis.covariance_propagation(grid, C, KERNEL, as_tensor=True), args.repeats)
        values = basis.synthesize(grid, KERNEL, as_tensor=True)
        surface_values = median_ms(lambda: basis.synthesize(grid, KERNEL, as_tensor=True), args.repeats)
        points, kn_t = ga.engine.rbf_surface_tables(grid, KERNEL, basis)
        block = slice(0, min(M, max((1 << 30) // (16 * J), 1)))
        p, kn = points[block], kn_t[:, block]
        st_ms = median_ms(lambda: ga.engine.rbf_surface(basis, p, kn), args.repeats)
        ops = 8.0 * N * J * p.shape[0]
        rows.append({'degree': N, 'nodes': J, 'points': M, 'what': 'surface', 'sigma_ms': surface_sigma, 'values_ms': surface_values,
                     'block_points': int(p.shape[0]), 'st_ms': st_ms, 'st_tops': ops / st_ms / 1e9, 'st_fraction_of_peak': 2 * ops / st_ms / 1e-3 / PEAK})
        report('surface  {0}: sigma {1:9.3f} ms  values {2:9.3f} ms; St of a block of {3} points {4:.3f} ms, {5:.2f} Tops/s fp64 = {6:.3f} of the '
               'vector peak'.format(size, surface_sigma, surface_values, p.shape[0], st_ms, rows[-1]['st_tops'], rows[-1]['st_fraction_of_peak']))
        # where the time of a block goes, and a series of solutions in one pass
        St = ga.engine.rbf_surface(basis, p, kn)
        product = median_ms(lambda: ga.engine.gemm(C, St), args.repeats)
        T = ga.engine.gemm(C, St)
        dots = median_ms(lambda: ga.engine.column_dots(St, T), args.repeats)
        one = ga.engine.to_device(basis.values).reshape(1, J)
        one_row = median_ms(lambda: ga.engine.gemm(one, St), args.repeats)
        series = np.random.default_rng(N + J + 3).standard_normal((SERIES, J))
        on_device = ga.engine.to_device(series)
        surface_series = median_ms(lambda: basis.synthesize(grid, KERNEL, values=on_device, as_tensor=True), args.repeats)
        rows[-1].update({'block_product_ms': product, 'block_dots_ms': dots, 'block_one_row_ms': one_row, 'series': SERIES, 'series_ms': surface_series})
        report('surface  {0}: of that block C St {1:.3f} ms ({2:.1f} TFLOP/s), the column dot products {3:.3f} ms ({4:.0f} GB/s read), one row of values times '
               'St {5:.3f} ms; a series of {6} solutions {7:9.3f} ms'.format(size, product, 2.0 * J * J * p.shape[0] / product / 1e9, dots,
                                                                             16.0 * J * p.shape[0] / dots / 1e6, one_row, SERIES, surface_series))
        del points, kn_t, p, kn, St, T

        started = time.perf_counter()
        F = basis.to_potential_coefficients_matrix()
        torch.cuda.synchronize()
        f_ms = (time.perf_counter() - started) * 1e3
        F = ga.engine.to_device(F)                                                   # [P, J]
        report('F        band {0}..{1:3d} J {2:5d}: {3:9.1f} ms once per basis (wall clock, host result), {4:.2f} GB resident, F C F^T {5:.2f} GB'.format(
            nmin, N, J, f_ms, 8.0 * P * J / 1e9, 8.0 * P * P / 1e9))

        def harmonic_sigma():
            return grid.covariance_propagation(ga.engine.congruence(F, C), nmin, N, KERNEL, si.GM, si.R)

        def harmonic_values():
            return basis.to_potential_coefficients().to_grid(grid, KERNEL).values

        def harmonic_series():
            kept = basis.values
            for values in series:
                basis.values = values
                harmonic_values()
            basis.values = kept

        sigma_difference = float(np.abs(ga.engine.to_host(sigma) - harmonic_sigma()).max() / float(sigma.max().item()))
        values_difference = float(np.abs(ga.engine.to_host(values) - harmonic_values()).max() / float(values.abs().max().item()))
        congruence = median_ms(lambda: ga.engine.congruence(F, C), args.repeats)
        harmonic_sigma_ms = median_ms(harmonic_sigma, args.repeats)
        harmonic_values_ms = median_ms(harmonic_values, args.repeats)
        harmonic_series_ms = median_ms(harmonic_series, args.repeats)
        rows.append({'degree': N, 'nodes': J, 'points': M, 'what': 'harmonic', 'sigma_ms': harmonic_sigma_ms, 'congruence_ms': congruence,
                     'values_ms': harmonic_values_ms, 'series_ms': harmonic_series_ms, 'series_over_surface': harmonic_series_ms / surface_series, 'sigma_over_surface': harmonic_sigma_ms / surface_sigma,
                     'values_over_surface': harmonic_values_ms / surface_values, 'sigma_difference_of_max': sigma_difference,
                     'values_difference_of_max': values_difference})
        report('harmonic {0}: sigma {1:9.3f} ms ({2:.2f} x the surface route; F C F^T {3:.3f} ms of it)  values {4:9.3f} ms ({5:.2f} x)  a series of {8} solutions, one to_grid each, {9:9.3f} ms '
               '({10:.2f} x); the routes differ by {6:.1e} of the largest sigma and {7:.1e} of the largest value'.format(
                   size, harmonic_sigma_ms, harmonic_sigma_ms / surface_sigma, congruence, harmonic_values_ms, harmonic_values_ms / surface_values,
                   sigma_difference, values_difference, SERIES, harmonic_series_ms, harmonic_series_ms / surface_series))
        grid.values = None
        del F, C, sigma, values
        torch.cuda.empty_cache()
    report(json.dumps({'rbf_surface': rows}))
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
