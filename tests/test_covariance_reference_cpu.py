"""
The long-double reference of grid covariance propagation (tests/covariance_reference.py) against the float64 oracle, its own row
selection, the positivity condition of every case of tests/test_gpu_covariance_routes.py, and the route table of the direct kernels
(shg_covprop_route, host logic only) against its Python twin.  No GPU.
"""

import numpy as np
import pytest

import covariance_reference as cr
import grates_amd as ga
from grates_amd import engine
from oracle import shg_oracle as orc


def test_oracle_against_long_double_reference():
    """The float64 oracle (per parallel F @ Sigma, then the row dot) on a 10 degree geographic grid at d/o 20, nmin 2, P = 437, per
    point against the reference on the oracle's own tables.  A P-term float64 dot product of terms of one size is off by at most
    about P eps / 2 = 4.9e-14 relative, the square root halves it: the bound asserted.  Measured: 3.1e-15 at the worst point."""
    N, nmin = 20, 2
    grid = ga.grid.GeographicGrid(10.0, 10.0)
    cov = cr.general_matrix(5, cr.size(N, nmin))
    colat, _, kn = orc.kn_table(orc.KernelTable('potential'), N, grid.parallels, orc.GM_DEFAULT, orc.R_DEFAULT)
    got = orc.covariance_propagation_regular(cov, nmin, N, grid.meridians, grid.parallels, orc.KernelTable('potential'))
    ref, norm = cr.sigma_grid(cov, nmin, N, colat, kn, grid.meridians, with_norm=True)
    cr.assert_positive(ref, norm, 'oracle grid')
    worst = float(np.max(np.abs(got.astype(cr.LD) - ref) / ref))
    print('oracle against the long-double reference, worst point: {0:.2e}'.format(worst))
    assert worst < 0.25 * cr.size(N, nmin) * np.finfo(float).eps


def test_quadratic_form_range_of_the_issue():
    """d/o 20 on 35 points: a^T Sigma a / |a|^2 stays inside [0.5, 1.5] +- a few eps = 0.05 for both matrix kinds"""
    colat, kn, lon = cr.grid_tables(3, 20, 7, 5)
    for S in (cr.general_matrix(3, 441), cr.symmetric_matrix(3, 441)):
        ref, norm = cr.sigma_grid(S, 0, 20, colat, kn, lon, with_norm=True)
        ratio = (ref ** 2 / norm).astype(float)
        assert ratio.min() > 0.8 and ratio.max() < 1.25, (ratio.min(), ratio.max())


def test_rows_chunks_and_matrix_kinds():
    colat, kn, lon = cr.grid_tables(4, 6, 5, 7)
    assert colat[0] == 0.0 and colat[1] == np.pi and colat[2] == 0.5 * np.pi and colat[3] == 1e-3
    assert lon[0] == -np.pi and cr.ODD_MERIDIAN in lon and np.all(np.diff(lon) > 0)
    head = cr.grid_tables(4, 6, 3, 7)
    assert np.array_equal(head[0], colat[:3]) and np.array_equal(head[1], kn[:3]) and np.array_equal(head[2], lon)
    S = cr.general_matrix(4, 45)
    assert not np.array_equal(S, S.T) and np.unique(np.diag(S)).size == 45
    full = cr.sigma_grid(S, 2, 6, colat, kn, lon)
    assert full.dtype == cr.LD and full.shape == (35,)
    rows = np.array([34, 0, 7, 6, 20])
    assert np.array_equal(cr.sigma_grid(S, 2, 6, colat, kn, lon, rows=rows), full[rows])
    rechunked = cr.sigma_grid(S, 2, 6, colat, kn, lon, chunk=7)
    assert float(np.max(np.abs(rechunked - full) / full)) < 1e-17
    # only the symmetric part counts, and a transposed matrix gives the same form: the reference reads the matrix as it is
    assert float(np.max(np.abs(cr.sigma_grid(S.T.copy(), 2, 6, colat, kn, lon) - full) / full)) < 1e-17
    swapped = S.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert float(np.max(np.abs(cr.sigma_grid(swapped, 2, 6, colat, kn, lon) - full) / full)) > 1e-3
    assert cr.sigma_grid(np.zeros((0, 0)), 7, 6, colat, kn, lon).tolist() == [0.0] * 35
    assert cr.slots(2, 1).tolist() == [0, 1, 2, 0, 1, 2, 3, 4] and [cr.size(*p) for p in cr.DEGREE_PAIRS] == list(cr.PAIR_SIZES)


@pytest.mark.parametrize('key', cr.small_references(), ids=lambda k: '{0}-N{1}-min{2}-{3}x{4}'.format(*k))
def test_positivity_of_every_small_case(key):
    ref, norm = cr.grid_reference(*key)
    cr.assert_positive(ref, norm, key)


def test_positivity_of_the_large_cases():
    """the 16 referenced rows of the two padded-copy cases and the six points of the permute-segment case"""
    nlon, nlat = cr.PADDED_GRID
    for N, nmin in cr.PADDED_PAIRS:
        colat, kn, lon = cr.grid_tables(cr.GRID_SEED, N, nlat, nlon)
        ref, norm = cr.sigma_grid(cr.general_matrix(1000 + N, cr.size(N, nmin)), nmin, N, colat, kn, lon, rows=cr.padded_rows(), with_norm=True)
        cr.assert_positive(ref, norm, (N, nmin))
    N, nmin, nlat, nlon = cr.PERMUTE_CASE
    colat, kn, lon = cr.grid_tables(cr.GRID_SEED, N, nlat, nlon)
    ref, norm = cr.sigma_grid(cr.general_matrix(1000 + N, cr.size(N, nmin)), nmin, N, colat, kn, lon, with_norm=True)
    cr.assert_positive(ref, norm, cr.PERMUTE_CASE)


def test_route_table_matches_the_dispatcher_at_every_seam():
    """shg_covprop_route (what covprop_diag_impl asks) against covariance_reference.route on both sides of every threshold"""
    assert cr.ROUTES == engine.COVPROP_ROUTE_KINDS
    seen = set()
    for nlon in (1, 3, 123, 124, 127, 128, 129, 130, 246, 247, 256, 257, 369, 370, 384, 385, 720):
        for P in (1, 128, 129, 3969, 4095, 4096):
            below = int(1e12 // (P * P))                           # M P^2 <= 1e12 < (M + 1) P^2
            for M in (nlon, 130 * nlon, below, below + 1):
                if not 0 < M < 2 ** 31:
                    continue
                for aligned in (False, True):
                    for symmetric in (False, True):
                        want = cr.route(nlon, P, aligned, M, symmetric)
                        assert engine.covprop_route(nlon, P, aligned, M, symmetric) == want, (nlon, P, aligned, M, symmetric)
                        seen.add(want)
    assert seen == set(cr.ROUTES) - {'NONE'}
    for nlon, kind in ((123, 'DIRECT'), (124, 'ROWS'), (128, 'ROWS'), (129, 'DIRECT'), (246, 'DIRECT'), (247, 'ROWS'), (256, 'ROWS'), (257, 'DIRECT'),
                       (720, 'DIRECT')):
        assert cr.route(nlon, 256, True, 3 * nlon, False) == kind
    assert cr.route(360, 3969, True, 64800, False) == 'PADDED' and cr.route(360, 3969, True, 63000, False) == 'REGISTER'
    assert cr.route(360, 4096, False, 64800, False) == 'PADDED' and cr.route(360, 4096, True, 64800, False) == 'DIRECT'
    assert engine.covprop_route(5, 0, True, 10, False) == 'NONE' and engine.covprop_route(5, 9, True, 0, True) == 'NONE'
    with pytest.raises(ga._lib.ShgError):
        engine.covprop_route(0, 9, True, 10, False)
    assert cr.padded_row_length(3969) == 3970 and cr.padded_row_length(4095) == 4098 and cr.padded_row_length(4096) == 4098


def test_case_list_reaches_every_route():
    """the shapes of the GPU module, by the table: every route kind has a case"""
    kinds = {cr.route(nlon, cr.size(N, nmin), True, cr.ROWS_NLAT * nlon, False) for nlon in cr.ROWS_NLON for N, nmin in cr.DEGREE_PAIRS}
    assert kinds == {'ROWS'}
    for nlon, nlat in cr.GENERAL_SHAPES:
        for N, nmin in cr.DEGREE_PAIRS:
            P = cr.size(N, nmin)
            assert cr.route(nlon, P, True, nlon * nlat, False) == ('DIRECT' if P % 2 == 0 else 'REGISTER')
            assert cr.route(nlon, P, False, nlon * nlat, False) == 'REGISTER'
    nlon, nlat = cr.PADDED_GRID
    assert all(cr.route(nlon, cr.size(N, nmin), True, nlon * nlat, False) == 'PADDED' for N, nmin in cr.PADDED_PAIRS)
