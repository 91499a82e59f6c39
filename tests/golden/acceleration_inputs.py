"""Seeded inputs of the gravitational acceleration fixture (tests/golden/make_golden_acceleration.py -> g22_acceleration.npz) and of
the tests that replay it.  The positions are stored in the fixture; the coefficients are rebuilt from the numbers below."""

import numpy as np

GM, R = 3.9860044150e+14, 6.3781363000e+06            # the default constants of PotentialCoefficients
A, F = 6378137.0, 298.2572221010 ** -1                 # GRS80 ellipsoid of the positions
HEIGHTS = (-25e3, 500e3)                               # ellipsoidal heights of the scattered positions [m]

# tag: (max degree, coefficient kind, seed, scattered positions)
CASES = {
    'point_mass': (0, 'point_mass', 2201, 300),
    'static60': (60, 'static', 2202, 400),
    'anomaly96': (96, 'anomaly', 2203, 400),
    'anomaly180': (180, 'anomaly', 2204, 250),
    'anomaly300': (300, 'anomaly', 2205, 24),
}


def coefficients(max_degree, kind, seed):
    """anm [N+1, N+1]: 'point_mass' C00 = 1; 'static' C00 = 1, C20 = -4.84e-4 and the other degrees >= 2 at 1e-6 / n^2;
    'anomaly' degrees >= 2 at 1e-10 (degrees 0 and 1 zero)"""
    N = max_degree
    anm = np.zeros((N + 1, N + 1))
    if kind == 'point_mass':
        anm[0, 0] = 1.0
        return anm
    rng = np.random.default_rng(seed)
    idx = np.arange(N + 1)
    degree = np.maximum(idx[:, np.newaxis], idx[np.newaxis, :])
    values = rng.standard_normal((N + 1, N + 1))
    if kind == 'static':
        anm = np.where(degree >= 2, values * 1e-6 / np.maximum(degree, 1) ** 2, 0.0)
        anm[0, 0], anm[2, 0] = 1.0, -4.84e-4
    else:
        anm = np.where(degree >= 2, values * 1e-10, 0.0)
    return anm


def special_positions(radius=A + 400e3):
    """exact poles (x = y = 0), points on the equator, negative-x points on the antimeridian (y = +0 and y = -0) and a point below R
    near the pole, all as Cartesian triples"""
    r = radius
    pts = [(0.0, 0.0, r), (0.0, 0.0, -r), (0.0, 0.0, 6.33e6), (0.0, 0.0, -6.33e6),
           (r, 0.0, 0.0), (0.0, r, 0.0), (-r, 0.0, 0.0), (-r, -0.0, 0.0), (0.0, -r, 0.0),
           (-r * np.cos(0.3), 0.0, r * np.sin(0.3)), (-r * np.cos(0.3), -0.0, -r * np.sin(0.3)),
           (-6.34e6, 0.0, 1e3), (1e-3, 0.0, 6.35e6)]
    return np.array(pts, dtype=float)


def scattered_positions(count, seed, heights=HEIGHTS):
    """`count` positions uniform on the sphere in direction, at ellipsoidal heights uniform in `heights` (geodetic2cartesian of
    the GRS80 ellipsoid, spelled out so that the tests need no grid module)"""
    rng = np.random.default_rng(seed)
    lon = rng.uniform(-np.pi, np.pi, count)
    lat = np.arcsin(rng.uniform(-1.0, 1.0, count))
    h = rng.uniform(heights[0], heights[1], count)
    e2 = 2 * F - F ** 2
    nu = A / np.sqrt(1 - e2 * np.sin(lat) ** 2)
    return np.vstack(((nu + h) * np.cos(lat) * np.cos(lon), (nu + h) * np.cos(lat) * np.sin(lon), ((1 - e2) * nu + h) * np.sin(lat))).T


def positions(tag):
    _, _, seed, count = CASES[tag]
    return np.vstack((special_positions(), scattered_positions(count, seed + 1000)))
