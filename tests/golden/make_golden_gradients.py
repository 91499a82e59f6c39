"""
Golden vectors of the gravitational gradient tensor at points (g23_gradients.npz).  An independent oracle: it shares nothing with the
kernel's algorithm (no coefficient combination, no column recursion in float64).  Run once:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gradients.py [--processes P]

For every case of gradient_inputs.CASES the potential V(x, y, z) = GM/R sum (R/r)^(n+1) P_nm (C cos m lon + S sin m lon) of the seeded
coefficients is evaluated with mpmath at 50 digits (a fully normalised Legendre recursion in mp arithmetic, the longitude terms from
x / rho and y / rho), and T = d^2 V / dx_i dx_j is taken by second-order central differences at mp precision with the step
h = 1e-12 r: the truncation error is about (h / r)^2 = 1e-24 of |T| and the rounding error about 1e-50 / (h / r)^2 = 1e-26, both far
below float64.  Off-diagonal values are computed once and stored twice.  Stored per case: xyz [M, 3] and T [M, 3, 3] (float64).
"""

import argparse
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import gradient_inputs as gi  # noqa: E402
import mpmath  # noqa: E402
from mpmath import mp, mpf  # noqa: E402

DPS = 50
STEP = mpf('1e-12')

_tables = {}


def _setup(tag):
    """mp copies of the coefficients and of the recursion factors a_nm, b_nm of the case (once per process)"""
    if tag in _tables:
        return _tables[tag]
    mp.dps = DPS
    N, kind, seed, _ = gi.CASES[tag]
    anm = gi.coefficients(N, kind, seed)
    C = [[mpf(float(anm[n, m])) for n in range(N + 1)] for m in range(N + 1)]                    # C[m][n]
    S = [[mpf(float(anm[m - 1, n])) if m >= 1 else mpf(0) for n in range(N + 1)] for m in range(N + 1)]
    a = [[mpf(0)] * (N + 1) for _ in range(N + 1)]
    b = [[mpf(0)] * (N + 1) for _ in range(N + 1)]
    for m in range(N + 1):
        for n in range(m + 2, N + 1):
            a[m][n] = mpmath.sqrt(mpf((2 * n - 1) * (2 * n + 1)) / ((n - m) * (n + m)))
            b[m][n] = mpmath.sqrt(mpf((2 * n + 1) * (n - m - 1) * (n + m - 1)) / ((2 * n - 3) * (n - m) * (n + m)))
    _tables[tag] = (N, C, S, a, b)
    return _tables[tag]


def potential(tag, x, y, z):
    N, C, S, a, b = _setup(tag)
    GM, R = mpf(gi.GM), mpf(gi.R)
    rho = mpmath.sqrt(x * x + y * y)
    r = mpmath.sqrt(rho * rho + z * z)
    t, s = z / r, rho / r
    cl, sl = (x / rho, y / rho) if rho != 0 else (mpf(1), mpf(0))
    u = R / r
    total = mpf(0)
    pmm, cm, sm, um = mpf(1), mpf(1), mpf(0), u                    # P_mm, cos m lon, sin m lon, (R/r)^(m+1)
    for m in range(N + 1):
        if m == 1:
            pmm = mpmath.sqrt(3) * s
        elif m >= 2:
            pmm = mpmath.sqrt(mpf(2 * m + 1) / (2 * m)) * s * pmm
        if m >= 1:
            cm, sm = cm * cl - sm * sl, sm * cl + cm * sl
            um = um * u
        Cm, Sm, am, bm = C[m], S[m], a[m], b[m]
        p2, p1, rad = mpf(0), pmm, um
        sc = p1 * rad * Cm[m]
        ss = p1 * rad * Sm[m]
        for n in range(m + 1, N + 1):
            p = (mpmath.sqrt(2 * m + 3) * t * p1) if n == m + 1 else (am[n] * t * p1 - bm[n] * p2)
            p2, p1 = p1, p
            rad = rad * u
            pr = p * rad
            sc += pr * Cm[n]
            ss += pr * Sm[n]
        total += sc * cm + ss * sm
    return GM / R * total


def tensor(args):
    """T [3, 3] at one position by central differences of the mp potential"""
    tag, xyz = args
    _setup(tag)
    mp.dps = DPS
    p = [mpf(float(v)) for v in xyz]
    h = STEP * mpmath.sqrt(p[0] ** 2 + p[1] ** 2 + p[2] ** 2)

    def V(*steps):
        q = list(p)
        for axis, sign in steps:
            q[axis] += sign * h
        return potential(tag, *q)

    v0 = V()
    T = np.empty((3, 3))
    for i in range(3):
        T[i, i] = float((V((i, 1)) - 2 * v0 + V((i, -1))) / (h * h))
        for j in range(i + 1, 3):
            d = (V((i, 1), (j, 1)) - V((i, 1), (j, -1)) - V((i, -1), (j, 1)) + V((i, -1), (j, -1))) / (4 * h * h)
            T[i, j] = T[j, i] = float(d)
    return T


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--processes', type=int, default=min(os.cpu_count() or 1, 8))
    args = parser.parse_args()
    tasks, spans = [], {}
    for tag in gi.CASES:
        xyz = gi.positions(tag)
        spans[tag] = (len(tasks), xyz)
        tasks += [(tag, x) for x in xyz]
    tasks_by_cost = sorted(range(len(tasks)), key=lambda i: -gi.CASES[tasks[i][0]][0])
    with multiprocessing.Pool(args.processes) as pool:
        done = pool.map(tensor, [tasks[i] for i in tasks_by_cost], chunksize=1)
    results = [None] * len(tasks)
    for i, T in zip(tasks_by_cost, done):
        results[i] = T
    out = {}
    for tag, (first, xyz) in spans.items():
        T = np.stack(results[first:first + xyz.shape[0]])
        assert np.all(np.isfinite(T)), tag
        out['xyz_' + tag] = xyz
        out['T_' + tag] = T
        trace = np.abs(np.trace(T, axis1=1, axis2=2)).max() / np.abs(T).max()
        print('{0:12s} d/o {1:3d} points {2:4d} max|T| {3:.3e} max|trace| / max|T| {4:.1e}'.format(
            tag, gi.CASES[tag][0], xyz.shape[0], np.abs(T).max(), trace))
    path = os.path.join(HERE, 'g23_gradients.npz')
    np.savez_compressed(path, **out)
    print('g23_gradients {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
