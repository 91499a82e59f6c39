"""Seeded inputs of the radial basis function fixture (tests/golden/make_golden_radial_basis.py -> g29_radial_basis.npz) and of the
tests that replay it, with a float64 NumPy restatement of grates_amd/csrc/rbf.h and rbf.hip in the kernel's operation order: the
Legendre sums of one (point, node) pair, the four kinds of entry and the host-built node and degree tables.  Needs NumPy only."""

import numpy as np

import acceleration_inputs as ai
import design_inputs as di

GM, R = di.GM, di.R
A, F = ai.A, ai.F                                      # GRS80: the ellipsoid the nodes of the fixture lie on
KINDS = ('acc', 'los', 'pot', 'dif')

# tag: (min_degree, max_degree, nodes, seed of the nodes)
CASES = {'b0_8': (0, 8, 24, 2901), 'b2_8': (2, 8, 24, 2901), 'b2_2': (2, 2, 3, 2902)}
PAIR_SEED = 2903
SEPARATION = 220e3                                     # of most pairs [m]
NEAR_AXIS = 12                                         # the position of design_inputs 1 mm off the axis: beyond the reference's colatitude
SHORT = {21: 1e3, 24: 1.0, 26: 0.0}                    # pair: separation [m]; a pair at one position has explicit directions only
N96 = {'min_degree': 2, 'max_degree': 96, 'nodes': 8, 'node_seed': 2911, 'points': 300, 'point_seed': 2912}
FORWARD = {'min_degree': 2, 'max_degree': 12, 'nodes': 40, 'node_seed': 2921, 'points': 300, 'point_seed': 2922, 'value_seed': 2923}
LOOP = {'min_degree': 2, 'max_degree': 8, 'nodes': 48, 'depth': 10e3, 'count': 600, 'heights': (250e3, 500e3), 'shells': 8, 'arc_length': 50,
        'position_seed': 2931, 'offset_seed': 2932, 'value_seed': 2933, 'constant_seed': 2934}


# ---- the basis ---------------------------------------------------------------------------------------------------------------------
def degree_factors(min_degree, max_degree, flat=False):
    """k_n [N + 1], zero below min_degree: a smooth decaying shape with a ripple, or all ones in the band (flat: the hardest for the
    high degrees)"""
    n = np.arange(max_degree + 1, dtype=float)
    k = np.ones(max_degree + 1) if flat else (1.0 + 0.25 * np.sin(1.7 * n)) / (n + 1.0) ** 1.5
    k[:min_degree] = 0.0
    return k


def shape_factors(k):
    """K [N + 1, N + 1] in the coefficient layout from k_n: every C slot K[n, 0..n] and every S slot K[m - 1, n] of degree n is k_n"""
    N = k.size - 1
    K = np.zeros((N + 1, N + 1))
    for n in range(N + 1):
        K[n, :n + 1] = k[n]
        K[:n, n] = k[n]
    return K


def scattered_nodes(count, seed):
    """(longitude, latitude) [count] each, geodetic [rad], seeded and uniform on the sphere"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-np.pi, np.pi, count), np.arcsin(rng.uniform(-1.0, 1.0, count))


def fibonacci_nodes(count):
    """(longitude, latitude) of the Fibonacci lattice: an even cover of the sphere without a pole"""
    i = np.arange(count) + 0.5
    lat = np.arcsin(1.0 - 2.0 * i / count)
    lon = np.mod(i * np.pi * (3.0 - np.sqrt(5.0)) + np.pi, 2 * np.pi) - np.pi
    return lon, lat


def node_table(longitude, latitude, a=A, f=F, R=R):
    """nodes [J, 4] as engine.rbf_node_table builds them: the unit vector of (geocentric colatitude, longitude) of a point on the
    ellipsoid (utilities.colatitude, utilities.geocentric_radius, spelled out) and R / r_j"""
    e2 = f * (2 - f)
    nu = a / np.sqrt(1 - e2 * np.sin(latitude) ** 2)
    radius = nu * np.sqrt(np.cos(latitude) ** 2 + (1 - e2) ** 2 * np.sin(latitude) ** 2)
    colat = np.arccos(nu * (1 - e2) * np.sin(latitude) / radius)
    return np.stack((np.sin(colat) * np.cos(longitude), np.sin(colat) * np.sin(longitude), np.cos(colat), R / radius), axis=1)


def case_nodes(tag):
    _, _, count, seed = CASES[tag]
    return scattered_nodes(count, seed)


# ---- the points of the fixture -----------------------------------------------------------------------------------------------------
def positions(tag):
    """xyz [29, 3]: the 20 positions of design_inputs (poles, axis, equator, antimeridian, below R, seven scattered) and, for each of
    the first three nodes, a point exactly above it (400 km), one antipodal to it and one 1 m beside the first"""
    nodes = node_table(*case_nodes(tag))
    extra = []
    for j in range(3):
        e, r = nodes[j, :3], R / nodes[j, 3] + 400e3
        beside = np.cross(e, (0.0, 0.0, 1.0))
        extra += [r * e, -r * e, r * e + beside / np.sqrt(np.sum(beside * beside))]
    return np.vstack((di.positions(), np.array(extra)))


def separations():
    sep = np.full(29, SEPARATION)
    for pair, value in SHORT.items():
        sep[pair] = value
    return sep


def pairs(tag):
    """(a, b) [29, 3] each: a = positions(tag), b = a + sep d with seeded unit d (sep 0: b is a, bit for bit)"""
    a = positions(tag)
    d = np.random.default_rng(PAIR_SEED).standard_normal(a.shape)
    d = d / np.sqrt(np.sum(d * d, axis=1))[:, np.newaxis]
    sep = separations()
    b = a + sep[:, np.newaxis] * d
    b[sep == 0.0] = a[sep == 0.0]
    return a, b


def directions(tag):
    """e [29, 3]: (b - a) / |b - a| in the kernel's order, the seeded unit vector for the pair at one position.  The fixture passes
    them explicitly, so every pair has a line of sight."""
    a, b = pairs(tag)
    d = b - a
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    seeded = np.random.default_rng(PAIR_SEED).standard_normal(a.shape)
    seeded = seeded / np.sqrt(np.sum(seeded * seeded, axis=1))[:, np.newaxis]
    same = length == 0.0
    e = np.where(same[:, np.newaxis], seeded, d / np.where(same, 1.0, length)[:, np.newaxis])
    return e / np.sqrt(np.sum(e * e, axis=1))[:, np.newaxis]


def point_errors(A, ref, M=29):
    """max|A - ref| per point (pair) [M] of design matrices [K M, J]"""
    return np.abs(A - ref).reshape(M, -1).max(axis=1)


def project(e, gb, ga):
    """e . (g(b) - g(a)) [M]: the difference per component first, then (e_x d_x + e_y d_y) + e_z d_z"""
    d = gb - ga
    return (e[:, 0] * d[:, 0] + e[:, 1] * d[:, 1]) + e[:, 2] * d[:, 2]


# ---- the restatement of rbf.h ------------------------------------------------------------------------------------------------------
def degree_table(k, min_degree):
    """(alpha, beta, gamma, d, e) [N + 1] each, as rbf_degree_table builds them for RbfDegree<1>"""
    n = np.arange(k.size, dtype=float)
    safe = np.maximum(n, 1.0)
    alpha = np.where(n > 0, (2.0 * n - 1.0) / safe, 0.0)
    beta = np.where(n > 0, (n - 1.0) / safe, 0.0)
    gamma = np.where(n > 0, 2.0 * n - 1.0, 0.0)
    d = np.where(n < min_degree, 0.0, k * (2.0 * n + 1.0))
    return alpha, beta, gamma, d, (n + 1.0) * d


def chains(xyz, nodes, k, min_degree, GM=GM, R=R):
    """(V [M, J], g [M, J, 3]): RbfPoint, RbfChain<1> and the scaling of RbfObservation (rbf.hip) for every (point, node) pair"""
    alpha, beta, gamma, d, e = degree_table(k, min_degree)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r = np.sqrt((x * x + y * y) + z * z)
    xh = np.stack((x / r, y / r, z / r), axis=1)                                        # [M, 3]
    u, rinv = R / r, 1.0 / r
    t = (xh[:, None, 0] * nodes[None, :, 0] + xh[:, None, 1] * nodes[None, :, 1]) + xh[:, None, 2] * nodes[None, :, 2]      # [M, J]
    q = u[:, None] * nodes[None, :, 3]
    qn = q.copy()
    p1, p2, dp1, dp2 = np.ones_like(t), np.zeros_like(t), np.zeros_like(t), np.zeros_like(t)
    sv, sr, st = d[0] * qn, e[0] * qn, np.zeros_like(t)
    for n in range(1, k.size):
        p = (alpha[n] * t) * p1 - beta[n] * p2
        dp = dp2 + gamma[n] * p1
        p2, p1, dp2, dp1 = p1, p, dp1, dp
        qn = qn * q
        w = qn * p
        sv = sv + d[n] * w
        sr = sr + e[n] * w
        st = st + d[n] * (qn * dp)
    g = st[:, :, None] * (nodes[None, :, :3] - t[:, :, None] * xh[:, None, :]) - sr[:, :, None] * xh[:, None, :]
    GM_R = GM / R
    return sv * GM_R, g * (GM_R * rinv)[:, None, None]


def restatement(kind, nodes, k, min_degree, a, b=None, e=None, GM=GM, R=R):
    """A [K M, J] of `kind` (one of KINDS) in float64 NumPy, rows as the design matrices of gravityfield order them"""
    Va, ga = chains(a, nodes, k, min_degree, GM, R)
    if kind == 'acc':
        return ga.transpose(0, 2, 1).reshape(-1, nodes.shape[0])
    if kind == 'pot':
        return Va
    Vb, gb = chains(b, nodes, k, min_degree, GM, R)
    if kind == 'dif':
        return Vb - Va
    d = gb - ga
    return (e[:, None, 0] * d[:, :, 0] + e[:, None, 1] * d[:, :, 1]) + e[:, None, 2] * d[:, :, 2]


# ---- the further cases -------------------------------------------------------------------------------------------------------------
def n96_nodes():
    return scattered_nodes(N96['nodes'], N96['node_seed'])


def n96_positions():
    return ai.scattered_positions(N96['points'], N96['point_seed'])


def forward_nodes():
    return scattered_nodes(FORWARD['nodes'], FORWARD['node_seed'])


def forward_positions():
    return ai.scattered_positions(FORWARD['points'], FORWARD['point_seed'])


def forward_values():
    return np.random.default_rng(FORWARD['value_seed']).standard_normal(FORWARD['nodes'])


def on_sphere(lon, lat, radius):
    return radius[:, np.newaxis] * np.vstack((np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat))).T


def loop_shells():
    return R + np.linspace(LOOP['heights'][0], LOOP['heights'][1], LOOP['shells'])


def loop_positions():
    """(xyz [600, 3], radius [600]): seeded directions, point i on shell i % 8 of the eight between 250 and 500 km above R"""
    rng = np.random.default_rng(LOOP['position_seed'])
    lon = rng.uniform(-np.pi, np.pi, LOOP['count'])
    lat = np.arcsin(rng.uniform(-1.0, 1.0, LOOP['count']))
    radius = loop_shells()[np.arange(LOOP['count']) % LOOP['shells']]
    return on_sphere(lon, lat, radius), radius


def loop_pairs():
    """(a, b): a = loop_positions(), b about 220 km from a in a seeded direction, on the shell three above a's (cyclic)"""
    a, _ = loop_positions()
    d = np.random.default_rng(LOOP['offset_seed']).standard_normal(a.shape)
    d = d / np.sqrt(np.sum(d * d, axis=1))[:, np.newaxis]
    toward = a + SEPARATION * d
    radius_b = loop_shells()[(np.arange(a.shape[0]) + 3) % LOOP['shells']]
    return a, toward * (radius_b / np.sqrt(np.sum(toward * toward, axis=1)))[:, np.newaxis]


def loop_nodes():
    """(longitude, latitude, a, f): 48 Fibonacci nodes on the sphere 10 km below R"""
    lon, lat = fibonacci_nodes(LOOP['nodes'])
    return lon, lat, R - LOOP['depth'], 0.0


def loop_values():
    return np.random.default_rng(LOOP['value_seed']).standard_normal(LOOP['nodes'])


def loop_arcs():
    return np.arange(0, LOOP['count'], LOOP['arc_length'])


def loop_constants():
    """the planted constant of every arc [12], a thousandth of GM / R: of the size of the signal of the planted values"""
    return np.random.default_rng(LOOP['constant_seed']).uniform(-1.0, 1.0, loop_arcs().size) * (GM / R * 1e-3)


def arc_indicator():
    B = np.zeros((LOOP['count'], loop_arcs().size))
    B[np.arange(LOOP['count']), np.arange(LOOP['count']) // LOOP['arc_length']] = 1.0
    return B
