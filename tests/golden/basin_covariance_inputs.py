"""Seeded inputs of the basin covariance fixture (tests/golden/make_golden_basin_covariance.py -> g21_basin_covariance.npz) and of
the tests that replay it.  The masks themselves are stored in the fixture; grids, point sets and covariance matrices are rebuilt from
the numbers below."""

import numpy as np

from basin_inputs import star

MAX_DEGREE = 30
GAUSS_PARALLELS = 40
SCATTER_SEED, SCATTER_COUNT = 2121, 2000
COV_SEED, COV_RANK = 2122, 40
FILTER_RADIUS = 300e3


def grids(module):
    """(tag, grid) of the fixture's cases built with `module` (the reference's grates.grid or grates_amd.grid)"""
    rng = np.random.default_rng(SCATTER_SEED)
    lon = rng.uniform(-np.pi, np.pi, SCATTER_COUNT)
    lat = np.arcsin(rng.uniform(-1.0, 1.0, SCATTER_COUNT))
    return [('geographic', module.GeographicGrid(3, 3)), ('gauss', module.GaussGrid(GAUSS_PARALLELS)),
            ('irregular', module.IrregularGrid(lon, lat))]


def basin_polygons():
    """four basins: two star polygons, a box (Basin.from_extent) and one too small to hold a point of any case (the empty mask)"""
    return {'star_a': star(300, -60.0, -5.0, 0.5, 11),
            'star_b': star(200, 20.0, 45.0, 0.4, 12),
            'box': tuple(np.deg2rad([100.0, -40.0, 150.0, -10.0])),
            'empty': star(12, 1.3, 0.7, 0.002, 13)}


def basins(module):
    p = basin_polygons()
    return [module.Basin(p['star_a']), module.Basin(p['star_b']), module.Basin.from_extent(*p['box']), module.Basin(p['empty'])]


def covariance(min_degree, max_degree=MAX_DEGREE):
    """Sigma = L L^T + diag(d) of the degrees min_degree .. max_degree: (L, d), L [Pn, COV_RANK]"""
    Pn = (max_degree + 1) ** 2 - min_degree ** 2
    rng = np.random.default_rng(COV_SEED + min_degree)
    L = rng.standard_normal((Pn, COV_RANK)) * 1e-10
    d = rng.uniform(0.5, 1.5, Pn) * 1e-21
    return L, d


def sigma(L, d):
    return L @ L.T + np.diag(d)


CASES = [(grid, kernel, nmin) for grid in ('geographic', 'gauss', 'irregular') for kernel in ('ewh', 'potential') for nmin in (0, 2)]
FILTERED = [case for case in CASES if case[1] == 'ewh']


def tag(grid, kernel, nmin):
    return '{0}_{1}_{2}'.format(grid, kernel, nmin)
