"""Seeded inputs of the potential fixture (tests/golden/make_golden_potential.py -> g28_potential.npz) and of the tests that replay
it, with a float64 NumPy restatement of the formulas of the fourth part of grates_amd/csrc/design.hip (the column recursion of
design_inputs.restatement at degree N itself, one harmonic per entry) and of the forward functional.  Needs NumPy only."""

import numpy as np

import acceleration_inputs as ai
import design_inputs as di

GM, R = di.GM, di.R
DEGREES = di.DEGREES                                  # design matrices of the fixture, each from degree 0 and from degree 2
SHELLS = ai.A + np.linspace(350e3, 550e3, 8)          # radii of the spheres the scattered points lie on [m]
SEPARATION = 220e3                                    # of most pairs [m]
SHORT = {4: 1e3, 14: 1e3, 5: 1.0, 15: 1.0, 3: 0.0, 16: 0.0}      # pair: separation [m] (3, 4, 5 special positions, 14 .. 16 scattered)
# a on the axis (0 .. 2) or 1 mm off it (12): b lies along the axis too.  Two degrees off it the form s = sqrt(1 - t^2) that the
# kernels share with the reference turns one rounding of t into 5e-14 of s, which no fixture can pin down to 1e-14 of max|A_pot|
AXIS_PAIRS = (0, 1, 2, 12)
POSITION_SEED, PAIR_SEED = 2801, 2802
V60 = (60, 400, 2811, 2812)                           # forward values: degree, scattered points, seeds of the points and of the anomaly field
AX = (60, 120, 2813)                                  # ax_err: degree, points (on the shells only), seed; the field is that of V60
LOOP = {'N': 8, 'min_degree': 2, 'count': 600, 'arc_length': 50, 'position_seed': 2821, 'offset_seed': 2822, 'field_seed': 2823,
        'constant_seed': 2824}                        # the three closed loops: V, V(b) - V(a), V with one constant per arc


def shell_positions(count, seed):
    """(xyz [count, 3], radius [count]): seeded directions uniform on the sphere, point i on the sphere of radius SHELLS[i % 8]"""
    rng = np.random.default_rng(seed)
    lon = rng.uniform(-np.pi, np.pi, count)
    lat = np.arcsin(rng.uniform(-1.0, 1.0, count))
    radius = SHELLS[np.arange(count) % SHELLS.size]
    return on_sphere(lon, lat, radius), radius


def on_sphere(lon, lat, radius):
    return radius[:, np.newaxis] * np.vstack((np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat))).T


def radius_of(xyz):
    """r in the operation order of the kernels"""
    return np.sqrt((xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2])


def positions():
    """(xyz [20, 3], radius [20]): the special positions of the acceleration fixture (exact poles, on the axis below R, equator, +-0
    on the antimeridian, below R next to the pole), each on a sphere of its own, and seven points on the shells"""
    special = ai.special_positions()
    xyz, radius = shell_positions(7, POSITION_SEED)
    return np.vstack((special, xyz)), np.concatenate((radius_of(special), radius))


def pairs():
    """(a, b) [20, 3] each: a = positions(), b = a + sep d with seeded unit d and sep = 220 km, but 1 km, 1 m and 0 for the pairs of
    SHORT (sep 0: b is a, bit for bit); the pairs of AXIS_PAIRS are displaced along the axis instead"""
    a = positions()[0]
    d = np.random.default_rng(PAIR_SEED).standard_normal(a.shape)
    d = d / np.sqrt(np.sum(d * d, axis=1))[:, np.newaxis]
    sep = separations()
    b = a + sep[:, np.newaxis] * d
    for pair in AXIS_PAIRS:                           # outward along the axis
        b[pair] = a[pair] + (0.0, 0.0, np.copysign(sep[pair], a[pair, 2]))
    b[sep == 0.0] = a[sep == 0.0]
    return a, b


def separations():
    sep = np.full(20, SEPARATION)
    for pair, value in SHORT.items():
        sep[pair] = value
    return sep


def solid_harmonics(xyz, max_degree, R=R):
    """(Yc, Ys): dicts (n, k) -> [M] of the solid harmonics of degree max_degree by the column recursion of design_harmonics_kernel
    (design_inputs.restatement runs the same one at degree N + 1)"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r = np.sqrt((x * x + y * y) + z * z)
    th = np.arctan2(np.sqrt(x * x + y * y), z)
    lam = np.arctan2(y, x)
    u, t = R / r, np.cos(th)
    s = np.sqrt(1.0 - t * t)
    Yc, Ys = {}, {}
    pmm, rk = np.ones_like(t), u.copy()
    for k in range(max_degree + 1):
        if k == 1:
            pmm = np.sqrt(3.0) * s
        elif k >= 2:
            pmm = np.sqrt((2.0 * k + 1.0) / (2.0 * k)) * s * pmm
        if k >= 1:
            rk = rk * u
        ck, sk = np.cos(k * lam), np.sin(k * lam)
        p1, p2, rad = pmm, np.zeros_like(t), rk
        for n in range(k, max_degree + 1):
            if n > k:
                a = np.sqrt((2 * n - 1) / (n - k) * (2 * n + 1) / (n + k))
                b = np.sqrt((2 * n + 1) / (2 * n - 3) * (n - k - 1) / (n - k) * (n + k - 1) / (n + k)) if n > k + 1 else 0.0
                p1, p2 = (a * t) * p1 - b * p2, p1
            pk = p1 * rad
            rad = rad * u
            Yc[n, k], Ys[n, k] = pk * ck, pk * sk
    return Yc, Ys


def _columns(Yc, Ys, min_degree, max_degree):
    return np.stack([(Ys if sine else Yc)[n, m] for n, m, sine in di.degreewise(min_degree, max_degree)], axis=1)


def restatement(xyz, min_degree, max_degree, GM=GM, R=R):
    """A_pot [M, P] in float64 NumPy: an entry is Y * (GM / R)"""
    return _columns(*solid_harmonics(xyz, max_degree, R), min_degree, max_degree) * (GM / R)


def difference_restatement(xyz_a, xyz_b, min_degree, max_degree, GM=GM, R=R):
    """A_dV [M, P] in float64 NumPy: an entry is (Y(b) - Y(a)) * (GM / R), the kernel's order"""
    Ya = _columns(*solid_harmonics(xyz_a, max_degree, R), min_degree, max_degree)
    Yb = _columns(*solid_harmonics(xyz_b, max_degree, R), min_degree, max_degree)
    return (Yb - Ya) * (GM / R)


def forward(xyz, anm, GM=GM, R=R):
    """V [M] in float64 NumPy: the sum over (n, k) of Yc C + Ys S in the kernel's order (orders outermost), then * GM / R"""
    N = anm.shape[0] - 1
    Yc, Ys = solid_harmonics(xyz, N, R)
    acc = np.zeros(xyz.shape[0])
    for k in range(N + 1):
        for n in range(k, N + 1):
            acc = acc + Yc[n, k] * anm[n, k]
            if k >= 1:
                acc = acc + Ys[n, k] * anm[k - 1, n]
    return acc * (GM / R)


def v60_positions():
    """(xyz [413, 3], radius): the special positions and 400 points on the shells"""
    special = ai.special_positions()
    xyz, radius = shell_positions(V60[1], V60[2])
    return np.vstack((special, xyz)), np.concatenate((radius_of(special), radius))


def v60_field():
    return ai.coefficients(V60[0], 'anomaly', V60[3])


def ax_positions():
    return shell_positions(AX[1], AX[2])


def loop_positions():
    """(xyz [600, 3], radius): points on the shells, 12 arcs of 50 consecutive points"""
    return shell_positions(LOOP['count'], LOOP['position_seed'])


def loop_pairs():
    """(a, b, radius_a, radius_b): a = loop_positions(), b on the shell three above a's (cyclic) in the direction of a + 220 km d with
    seeded unit d: about 220 km apart, every point of both satellites on one of the eight shells"""
    a, radius_a = loop_positions()
    d = np.random.default_rng(LOOP['offset_seed']).standard_normal(a.shape)
    d = d / np.sqrt(np.sum(d * d, axis=1))[:, np.newaxis]
    toward = a + SEPARATION * d
    radius_b = SHELLS[(np.arange(a.shape[0]) + 3) % SHELLS.size]
    return a, toward * (radius_b / radius_of(toward))[:, np.newaxis], radius_a, radius_b


def loop_arcs():
    return np.arange(0, LOOP['count'], LOOP['arc_length'])


def loop_field():
    """anm [9, 9]: the d/o-8 anomaly field of the closed loops (degrees 0 and 1 are zero)"""
    return ai.coefficients(LOOP['N'], 'anomaly', LOOP['field_seed'])


def loop_constants():
    """the planted energy constant of every arc [12], of the size of the signal (GM / R 1e-10 sqrt(77) is 0.05 m^2/s^2)"""
    return np.random.default_rng(LOOP['constant_seed']).uniform(-0.1, 0.1, loop_arcs().size)


def arc_indicator():
    """B [600, 12]: column a is one on the points of arc a, what lstsq.arc_basis(arcs, 600, degree=0) spreads over the arcs"""
    B = np.zeros((LOOP['count'], loop_arcs().size))
    B[np.arange(LOOP['count']), np.arange(LOOP['count']) // LOOP['arc_length']] = 1.0
    return B
