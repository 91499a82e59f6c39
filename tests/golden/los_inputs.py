"""Seeded inputs of the line-of-sight design matrix fixture (tests/golden/make_golden_line_of_sight.py -> g26_line_of_sight.npz) and
of the tests that replay it, with a float64 NumPy restatement of the formulas of the third part of grates_amd/csrc/design.hip (the
solid harmonics and the terms are those of design_inputs.restatement).  Needs NumPy only."""

import numpy as np

import acceleration_inputs as ai
import design_inputs as di

GM, R = di.GM, di.R
DEGREES = di.DEGREES                                  # design matrices of the fixture, each from degree 0 and from degree 2
SEPARATION = 220e3                                    # of most pairs [m]
SHORT = {4: 1e3, 14: 1e3, 5: 1.0, 15: 1.0}            # pair: separation [m] (4, 5 on the equator, 14, 15 scattered)
POLE_PAIR, SEAM_PAIRS = 12, (6, 7)                    # b on the exact pole (a is 1 mm off it); a on the antimeridian, b across it
PAIR_SEED, DIRECTION_SEED = 2601, 2602
L60 = ('static60', 60, 2611, 2612)                    # l60: a-points of this g22 case, degree, seeds of the anomaly field and of b
LOOP = {'N': 8, 'min_degree': 2, 'count': 600, 'position_seed': 2621, 'offset_seed': 2622, 'field_seed': 2623}      # closed loop


def unit_vectors(count, seed):
    """seeded directions, uniform on the sphere"""
    d = np.random.default_rng(seed).standard_normal((count, 3))
    return d / np.sqrt(np.sum(d * d, axis=1))[:, np.newaxis]


def pairs():
    """(a, b) [20, 3] each: a = design_inputs.positions() (13 special positions, 7 scattered), b = a + sep d with seeded unit d and
    sep = 220 km, but 1 km and 1 m for the pairs of SHORT; pair 12 ends on the exact pole and pairs 6 and 7 (a on the antimeridian
    with y = +0 and y = -0) end on the other side of it"""
    a = di.positions()
    d = unit_vectors(a.shape[0], PAIR_SEED)
    sep = np.full(a.shape[0], SEPARATION)
    for pair, value in SHORT.items():
        sep[pair] = value
    b = a + sep[:, np.newaxis] * d
    b[POLE_PAIR] = (0.0, 0.0, a[POLE_PAIR, 2] + SEPARATION)
    b[SEAM_PAIRS[0]] = a[SEAM_PAIRS[0]] + (0.0, -SEPARATION, 0.0)
    b[SEAM_PAIRS[1]] = a[SEAM_PAIRS[1]] + (0.0, SEPARATION, 0.0)
    return a, b


def separations():
    a, b = pairs()
    return np.sqrt(np.sum((b - a) ** 2, axis=1))


def directions():
    """explicit lines of sight of the 20 pairs: seeded unit vectors that have nothing to do with b - a"""
    return unit_vectors(20, DIRECTION_SEED)


def line_of_sight(xyz_a, xyz_b):
    """e = (b - a) / |b - a| in the operation order of los_design_kernel"""
    d = xyz_b - xyz_a
    return d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, np.newaxis]


def project(e, upper, lower):
    """e . (upper - lower) over axis 1 of [M, 3, ...] arrays: the difference per component first, then (e_x d_x + e_y d_y) + e_z d_z"""
    d = upper - lower
    e = e.reshape(e.shape + (1,) * (d.ndim - 2))
    return (e[:, 0] * d[:, 0] + e[:, 1] * d[:, 1]) + e[:, 2] * d[:, 2]


def from_acceleration_matrices(A_a, A_b, e):
    """A_los [M, P] from the acceleration design matrices [3 M, P] of the two satellites"""
    M = e.shape[0]
    return project(e, A_b.reshape(M, 3, -1), A_a.reshape(M, 3, -1))


def restatement(xyz_a, xyz_b, min_degree, max_degree, e=None, GM=GM, R=R):
    """A_los [M, P] in float64 NumPy: design_inputs.restatement at both satellites, the difference per component, the projection"""
    e = line_of_sight(xyz_a, xyz_b) if e is None else e
    return from_acceleration_matrices(di.restatement(xyz_a, min_degree, max_degree, GM, R), di.restatement(xyz_b, min_degree, max_degree, GM, R), e)


def l60_pairs():
    """the pairs of l60: a = the positions of the g22 case, b = a + 220 km d with seeded unit d"""
    a = ai.positions(L60[0])
    return a, a + SEPARATION * unit_vectors(a.shape[0], L60[3])


def l60_field():
    return ai.coefficients(L60[1], 'anomaly', L60[2])


def loop_pairs():
    """600 scattered pairs at heights of -25 .. 500 km, b = a + 220 km d with seeded unit d"""
    a = ai.scattered_positions(LOOP['count'], LOOP['position_seed'])
    return a, a + SEPARATION * unit_vectors(LOOP['count'], LOOP['offset_seed'])


def loop_field():
    """anm [9, 9]: the d/o-8 anomaly field of the closed loop (degrees 0 and 1 are zero)"""
    return ai.coefficients(LOOP['N'], 'anomaly', LOOP['field_seed'])
