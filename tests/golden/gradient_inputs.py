"""Seeded inputs of the gravitational gradient fixture (tests/golden/make_golden_gradients.py -> g23_gradients.npz) and of the tests
that replay it.  The positions are stored in the fixture; the coefficients are rebuilt from the numbers below.  The constants, the
coefficient kinds and the position helpers are those of the acceleration fixture (acceleration_inputs)."""

import numpy as np

import acceleration_inputs as ai

GM, R = ai.GM, ai.R

# tag: (max degree, coefficient kind, seed, scattered positions)
CASES = {
    'point_mass': (0, 'point_mass', 2301, 800),
    'zonal2': (2, 'zonal', 2302, 400),
    'static60': (60, 'static', 2303, 200),
    'anomaly96': (96, 'anomaly', 2304, 60),
    'anomaly180': (180, 'anomaly', 2305, 12),
    'anomaly300': (300, 'anomaly', 2306, 2),
}
# anomaly300 keeps only these special positions: a pole, a pole below R, the equator, both signs of zero on the antimeridian and the
# points below R
FEW_SPECIAL = [0, 3, 4, 6, 7, 11]


def coefficients(max_degree, kind, seed):
    """anm [N+1, N+1]: 'zonal' C00 = 1 and C20 = -4.84e-4, nothing else; the other kinds are acceleration_inputs.coefficients"""
    if kind == 'zonal':
        anm = np.zeros((max_degree + 1, max_degree + 1))
        anm[0, 0], anm[2, 0] = 1.0, -4.84e-4
        return anm
    return ai.coefficients(max_degree, kind, seed)


def positions(tag):
    N, _, seed, count = CASES[tag]
    special = ai.special_positions()
    if N >= 300:
        special = special[FEW_SPECIAL]
    return np.vstack((special, ai.scattered_positions(count, seed + 1000)))


def point_mass_tensor(xyz, GM=GM):
    """T [M, 3, 3] of V = GM / r: GM (3 x x^T - r^2 I) / r^5"""
    xyz = np.asarray(xyz, dtype=float)
    r2 = np.sum(xyz ** 2, axis=1)
    r5 = r2 ** 2.5
    return GM * (3.0 * xyz[:, :, np.newaxis] * xyz[:, np.newaxis, :] - r2[:, np.newaxis, np.newaxis] * np.eye(3)) / r5[:, np.newaxis, np.newaxis]
