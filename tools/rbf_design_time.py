"""Acceleration design matrix with respect to the node values of radial basis functions, direct against composed, event-timed
(DESIGN.md section 4.19).
    python3 tools/rbf_design_time.py [--repeats R] [--kinds KIND ...] [--output profiles/rbf_design_time.txt]
At each size (band 2 .. N, J scattered nodes on GRS80 with flat shape factors, M scattered points), for the acceleration kind:
  direct    engine.rbf_design_checked (one shg_rbf_design call, without the Python checks: the Legendre sum of every (point, node)
            pair), with its fp64 operations (15 per degree and pair: 10 multiplications and 5 additions, none fused) over the time,
            as a fraction of the 78.6 TFLOP/s fp64 vector peak counted in fused operations, and the bytes of At [J][3][M] it writes
  composed  what the package offered before: engine.acceleration_design_checked of the block (At_sh [P][3][M]), then
            engine.gemm with F^T = to_potential_coefficients_matrix()^T resident on the device (F^T At_sh, 2 (3 M) P J flop)
  F         forming F itself (to_potential_coefficients_matrix, host result), once per basis: not part of `composed`
--kinds names the kinds of engine.RBF_KINDS to time (default: acceleration).  The other three get a `direct` line each, the time of
one engine.rbf_design_checked call and the bytes of At [J][M] it writes; the pair kinds run at b = a + 220 km along seeded unit vectors,
the line of sight with those vectors as directions.  There is no composed route for them here.
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

import acceleration_inputs as ai  # noqa: E402
import grates_amd as ga  # noqa: E402
import rbf_inputs as ri  # noqa: E402

PEAK = 78.6e12
SIZES = ((60, 3600, 2048), (96, 9000, 1024))          # (max degree, nodes, points)


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
    parser.add_argument('--kinds', nargs='+', choices=ga.engine.RBF_KINDS, default=['acceleration'])
    parser.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'rbf_design_time.txt'))
    args = parser.parse_args()
    ga.engine.require_gpu()
    rows, lines = [], []

    def report(line):
        print(line, flush=True)
        lines.append(line)

    nmin = 2
    for N, J, M in SIZES:
        P = (N + 1) ** 2 - nmin ** 2
        lon, lat = ri.scattered_nodes(J, N + J)
        basis = ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat), ri.shape_factors(ri.degree_factors(nmin, N, flat=True)), nmin, N,
                                                     ai.GM, ai.R)
        x = ga.engine.to_device(ai.scattered_positions(M, N + M))
        started = time.perf_counter()
        F = basis.to_potential_coefficients_matrix()
        torch.cuda.synchronize()
        f_ms = (time.perf_counter() - started) * 1e3
        Ft = ga.engine.to_device(np.ascontiguousarray(F.T))                         # [J, P]
        report('F        band {0}..{1:3d} J {2:5d}: {3:9.1f} ms once per basis (wall clock, host result), {4:.2f} GB resident'.format(
            nmin, N, J, f_ms, 8.0 * P * J / 1e9))

        for kind in args.kinds:
            if kind == 'acceleration':
                continue
            d = np.random.default_rng(N + M + 1).standard_normal((M, 3))
            d = ga.engine.to_device(d / np.sqrt(np.sum(d * d, axis=1))[:, None])
            b = x + ri.SEPARATION * d if kind in ('line_of_sight', 'potential_difference') else None
            e = d if kind == 'line_of_sight' else None
            ms = median_ms(lambda: ga.engine.rbf_design_checked(kind, basis, x, b, e, None), args.repeats)
            rows.append({'degree': N, 'nodes': J, 'points': M, 'what': 'direct ' + kind, 'ms': ms, 'gbytes_per_s': 8.0 * J * M / ms / 1e6})
            report('direct   band {0}..{1:3d} J {2:5d} M {3:5d} {4}: {5:9.3f} ms  {6:7.1f} GB/s written'.format(nmin, N, J, M, kind, ms,
                                                                                                          rows[-1]['gbytes_per_s']))
        if 'acceleration' not in args.kinds:
            continue

        direct = ga.engine.rbf_design_checked('acceleration', basis, x, None, None, None)
        ms = median_ms(lambda: ga.engine.rbf_design_checked('acceleration', basis, x, None, None, None), args.repeats)
        ops = 15.0 * N * J * M
        rows.append({'degree': N, 'nodes': J, 'points': M, 'what': 'direct', 'ms': ms, 'tops': ops / ms / 1e9, 'fraction_of_peak': 2 * ops / ms / 1e-3 / PEAK,
                     'gbytes_per_s': 8.0 * 3 * J * M / ms / 1e6})
        report('direct   band {0}..{1:3d} J {2:5d} M {3:5d}: {4:9.3f} ms  {5:6.2f} Tops/s fp64 = {6:.3f} of the vector peak  {7:7.1f} GB/s written'.format(
            nmin, N, J, M, ms, rows[-1]['tops'], rows[-1]['fraction_of_peak'], rows[-1]['gbytes_per_s']))
        direct_ms = ms

        def composed():
            At = ga.engine.acceleration_design_checked(N, nmin, x, None, ai.GM, ai.R)
            return ga.engine.gemm(Ft, At.reshape(P, 3 * M))

        difference = float((composed().reshape(J, 3, M) - direct).abs().max().item() / direct.abs().max().item())
        ms = median_ms(composed, args.repeats)
        flop = 2.0 * 3 * M * P * J
        rows.append({'degree': N, 'nodes': J, 'points': M, 'what': 'composed', 'ms': ms, 'gemm_tflops_at_most': flop / ms / 1e9, 'over_direct': ms / direct_ms,
                     'difference_of_max': difference})
        report('composed band {0}..{1:3d} J {2:5d} M {3:5d}: {4:9.3f} ms  ({5:.2f} x the direct call; the two differ by {6:.1e} of max|A|)'.format(
            nmin, N, J, M, ms, ms / direct_ms, difference))
        del x, Ft, direct
        torch.cuda.empty_cache()
    report(json.dumps({'rbf_design': rows}))
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
