"""
Golden vectors of the design matrix of the gravitational gradient tensor (g25_gradient_design.npz).  Run once:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gradient_design.py [--processes P]

A comes column by column from the mp oracle of make_golden_gradients.py (the potential with mpmath at 50 digits, central differences
at mp precision) applied to unit coefficient fields: that module is imported as it is and handed the tables of the unit fields.
Stored:

    xyz, frames       gradient_design_inputs.positions() and the seeded proper rotations for them (the first is the identity)
    A8, A2            d/o 8 and d/o 2 in the Earth-fixed frame, all six components, min_degree 0: [6 M, P], row 6 i + j for component
                      j of xx, xy, xz, yy, yz, zz at point i (min_degree 2 is the column slice [:, 4:])

and scalars, all computed here on the CPU in NumPy:

    restatement_err   gradient_design_inputs.restatement (the kernels' formulas in float64 NumPy) against A8 and A2, of max|A|
    ax_err            the restatement's A at d/o 96 times the coefficients of the g23 case anomaly96, against T_anomaly96 of
                      g23_gradients.npz at xyz_anomaly96, of max|T|
    loop_cond_all, host_rel_err_all, loop_cond_goce, host_rel_err_goce
                      the closed loop of gradient_design_inputs.LOOP in the seeded instrument frames, for all six components and for
                      (xx, yy, zz, xz): cond(A) and |x^ - x| / |x| (2-norms) of the solution through host normals
"""

import argparse
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import gradient_design_inputs as gdi  # noqa: E402
import gradient_inputs as gi  # noqa: E402
import make_golden_gradients as oracle  # noqa: E402
from mpmath import mp, mpf  # noqa: E402


def _unit_tables(n, m, sine, N):
    """what make_golden_gradients._setup builds for a case, for the field with the single coefficient (n, m, sine) set to 1"""
    mp.dps = oracle.DPS
    C = [[mpf(0)] * (N + 1) for _ in range(N + 1)]                  # C[m][n]
    S = [[mpf(0)] * (N + 1) for _ in range(N + 1)]
    (S if sine else C)[m][n] = mpf(1)
    a = [[mpf(0)] * (N + 1) for _ in range(N + 1)]
    b = [[mpf(0)] * (N + 1) for _ in range(N + 1)]
    for k in range(N + 1):
        for j in range(k + 2, N + 1):
            a[k][j] = mp.sqrt(mpf((2 * j - 1) * (2 * j + 1)) / ((j - k) * (j + k)))
            b[k][j] = mp.sqrt(mpf((2 * j + 1) * (j - k - 1) * (j + k - 1)) / ((2 * j - 3) * (j - k) * (j + k)))
    return N, C, S, a, b


def column(args):
    """one column of A [6 M]: the oracle tensor of a unit field at every position"""
    n, m, sine, N, xyz = args
    tag = ('unit', n, m, sine, N)
    oracle._tables[tag] = _unit_tables(n, m, sine, N)
    T = np.stack([oracle.tensor((tag, x)) for x in xyz])
    del oracle._tables[tag]
    return np.stack([T[:, c, d] for c, d in gdi.PAIRS], axis=1).ravel()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--processes', type=int, default=min(os.cpu_count() or 1, 8))
    args = parser.parse_args()
    xyz = gdi.positions()
    out = {'xyz': xyz, 'frames': gdi.frames(xyz.shape[0])}
    assert np.abs(np.einsum('iac,ibc->iab', out['frames'], out['frames']) - np.eye(3)).max() <= 1e-14
    assert np.allclose(np.linalg.det(out['frames']), 1.0) and np.array_equal(out['frames'][0], np.eye(3))
    restatement_err = 0.0
    with multiprocessing.Pool(args.processes) as pool:
        for N in gdi.DEGREES:
            tasks = [(n, m, sine, N, xyz) for n, m, sine in gdi.degreewise(0, N)]
            A = np.stack(pool.map(column, tasks, chunksize=1), axis=1)
            assert A.shape == (6 * xyz.shape[0], (N + 1) ** 2) and np.all(np.isfinite(A))
            out['A{0}'.format(N)] = A
            err = np.abs(gdi.restatement(xyz, 0, N) - A).max() / np.abs(A).max()
            restatement_err = max(restatement_err, err)
            print('d/o {0}: A {1}, max|A| {2:.3e}, restatement {3:.2e} of max|A|'.format(N, A.shape, np.abs(A).max(), err))

    tag, N = gdi.AX
    g23 = np.load(os.path.join(HERE, 'g23_gradients.npz'))
    points, T = g23['xyz_' + tag], g23['T_' + tag]
    degree, kind, seed, _ = gi.CASES[tag]
    assert degree == N
    x = gdi.ravel(gi.coefficients(N, kind, seed), 0, N)
    ax_err = np.abs(gdi.restatement(points, 0, N) @ x - gdi.rotate_tensor(T, None).ravel()).max() / np.abs(T).max()
    print('A @ x at d/o {0}, {1} points: {2:.2e} of max|T|'.format(N, points.shape[0], ax_err))
    out.update(restatement_err=restatement_err, ax_err=ax_err)

    loop = gdi.LOOP
    points, anm, F = gdi.loop_positions(), gdi.loop_field(), gdi.loop_frames()
    x = gdi.ravel(anm, loop['min_degree'], loop['N'])
    for name, components in gdi.LOOP_SETS.items():
        A = gdi.restatement(points, loop['min_degree'], loop['N'], F, components)
        obs = A @ x
        solution = np.linalg.solve(A.T @ A, A.T @ obs)
        host_rel_err = np.linalg.norm(solution - x) / np.linalg.norm(x)
        loop_cond = np.linalg.cond(A)
        print('closed loop on the host, {0}: relative error {1:.2e}, cond(A) {2:.1f}'.format(components, host_rel_err, loop_cond))
        assert loop_cond <= 1e4 and host_rel_err <= 1e-8
        out['host_rel_err_' + name], out['loop_cond_' + name] = host_rel_err, loop_cond

    path = os.path.join(HERE, 'g25_gradient_design.npz')
    np.savez_compressed(path, **out)
    print('g25_gradient_design {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
