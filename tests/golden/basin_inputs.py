"""Seeded inputs of the basin fixtures (tests/golden/make_golden_basin.py -> g20_basin.npz) and of the tests that replay them.
The polygons themselves are stored in the fixture; grids and point sets are rebuilt from the numbers below."""

import numpy as np

EXTENT = tuple(np.deg2rad([10.0, 40.0, 20.0, 50.0]))      # from_extent box whose edges lie on meridians and parallels
GAUSS_PARALLELS = 120
STATS_STEP = 1.0
SCATTER_SEED, SCATTER_COUNT = 2020, 100_000
STATS_SEED = 2021


def star(n, lon0, lat0, radius, seed):
    """star-shaped polygon of n vertices around (lon0, lat0) [deg], counter-clockwise, radius [rad]"""
    rng = np.random.default_rng(seed)
    theta = 2 * np.pi * np.arange(n) / n
    r = radius * (1 + 0.25 * np.sin(7 * theta)) * (1 + 0.05 * rng.random(n))
    lat0, lon0 = np.deg2rad(lat0), np.deg2rad(lon0)
    lon = lon0 + r * np.cos(theta) / np.cos(lat0)
    lat = lat0 + r * np.sin(theta)
    return np.column_stack((np.mod(lon + np.pi, 2 * np.pi) - np.pi, lat))


def polygons():
    theta = 2 * np.pi * np.arange(300) / 300
    ring = np.column_stack((theta - np.pi, -1.2 + 0.05 * np.sin(5 * theta)))
    return {'star500': star(500, -60.0, -5.0, 0.15, 1),
            'star2000': star(2000, 20.0, 10.0, 0.5, 2),
            'antimeridian': star(400, 180.0, 30.0, 0.2, 3),
            'southpole': ring,
            'multi': [star(400, 100.0, 40.0, 0.3, 4), star(100, 100.0, 40.0, 0.1, 5), star(80, 125.0, 40.0, 0.08, 6)]}


def edge_grid_axes():
    """0.5-degree meridians and parallels on whole degrees and half degrees: the EXTENT box's edges run through grid points"""
    return np.deg2rad(np.arange(-180.0, 180.0, 0.5)), np.deg2rad(np.arange(89.5, -89.75, -0.5))


def scattered_points():
    rng = np.random.default_rng(SCATTER_SEED)
    return rng.uniform(-np.pi, np.pi, SCATTER_COUNT), rng.uniform(-0.5 * np.pi, 0.5 * np.pi, SCATTER_COUNT)


def scalar_points():
    lon = np.deg2rad([-60.0, -60.5, 0.0, -52.0, 120.0, -62.0])
    lat = np.deg2rad([-5.0, -4.0, 0.0, -5.0, 45.0, -10.0])
    return lon, lat


def stats_values(count):
    return np.random.default_rng(STATS_SEED).standard_normal(count) * 0.3 + 1.0
