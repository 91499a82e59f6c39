"""
Every route of covariance propagation on regular grids at its seams, per point against the long-double reference of
tests/covariance_reference.py: covprop_rows_kernel, the three covariance instantiations of gemm_f64_kernel (Sigma copied straight
into LDS, the register path, the symmetric path), the padded copy of Sigma in front of the general kernel, and the separable chain
(full and half), all through engine.Plan.covariance_propagation; shg_symmetry_defect and the guard values behind the output
through the C ABI.

Per case: the route the case is meant for is asserted first (covariance_reference.route, the Python twin of shg_covprop_route, and
shg_covprop_route itself with the alignment of the tensor that is passed); the reference passes a^T Sigma a > |a|^2 / 2; the
output starts as NaN and must come back finite; every point obeys |sigma - ref| <= pr.TOL_SIGMA * ref (the worst ratio is printed
first); a band of the direct kernels equals the same rows of the full result bit for bit.

Left out: a Sigma of more than 4 GB (b_rows_cap of the general kernel) stays with test_full_size_properties_config4 of
tests/test_gpu_covariance.py, which needs the 8.6 GB matrix of d/o 180.
"""

import ctypes

import numpy as np
import pytest

import covariance_reference as cr
import points_reference as pr
from grates_amd import _lib, engine

pytestmark = pytest.mark.gpu

_plans = {}


def plan_of(N, nlat, nlon):
    key = (N, nlat, nlon)
    if key not in _plans:
        _plans[key] = engine.Plan(N, *cr.grid_tables(cr.GRID_SEED, N, nlat, nlon))
    return _plans[key]


def device_matrix(S, odd_base=False):
    """S on the device, 16-byte aligned, or as a contiguous view that starts one double into a larger tensor"""
    import torch
    P = S.shape[0]
    if not odd_base:
        t = engine.to_device(np.array(S))                          # (a copy: the shared matrices are read-only)
        assert t.data_ptr() % 16 == 0
        return t
    big = torch.empty(P * P + 2, dtype=torch.float64, device='cuda')
    assert big.data_ptr() % 16 == 0
    t = big[1:1 + P * P].view(P, P)
    t.copy_(torch.from_numpy(np.array(S)))
    assert t.data_ptr() % 16 == 8 and t.is_contiguous()
    return t


def expect_route(want, plan, cov, band, symmetric=False):
    M, P = (band[1] - band[0]) * plan.nlon, cov.shape[0]
    aligned = cov.data_ptr() % 16 == 0
    assert cr.route(plan.nlon, P, aligned, M, symmetric) == want
    assert engine.covprop_route(plan.nlon, P, aligned, M, symmetric) == want


def propagate(plan, cov, nmin, band=None, **kw):
    """sigma of the band on the host; the output tensor starts as NaN"""
    import torch
    lat0, lat1 = (0, plan.nlat) if band is None else band
    out = torch.full(((lat1 - lat0) * plan.nlon,), float('nan'), dtype=torch.float64, device='cuda')
    got = plan.covariance_propagation(cov, nmin, lat0, lat1, out=out, **kw)
    assert got is out
    return engine.to_host(out)


def check(got, ref, what):
    """per point against the long-double reference"""
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    worst = float(np.max(np.abs(got.astype(cr.LD) - ref) / ref))
    print('{0}: worst point {1:.2e} ({2:.3f} of the tolerance)'.format(what, worst, worst / pr.TOL_SIGMA))
    assert worst <= pr.TOL_SIGMA, what


def reference(kind, N, nmin, nlat, nlon):
    ref, norm = cr.grid_reference(kind, N, nmin, nlat, nlon)
    cr.assert_positive(ref, norm, (kind, N, nmin, nlat, nlon))
    return ref


def band_rows(full, band, nlon):
    return full[band[0] * nlon:band[1] * nlon]


def direct_case(want, plan, cov, nmin, ref, bands, what, symmetric=False):
    """the full grid against the reference, the bands bit for bit against the full grid; returns the full result"""
    expect_route(want, plan, cov, (0, plan.nlat), symmetric)
    full = propagate(plan, cov, nmin, symmetric=symmetric)
    check(full, ref, what)
    for band in bands:
        if band == (0, plan.nlat):
            continue
        expect_route(want, plan, cov, band, symmetric)
        got = propagate(plan, cov, nmin, band, symmetric=symmetric)
        assert np.array_equal(got, band_rows(full, band, plan.nlon)), '{0}: band {1}'.format(what, band)
    return full


# ---- covprop_rows_kernel
@pytest.mark.parametrize('pair', cr.DEGREE_PAIRS, ids=lambda p: 'N{0}min{1}'.format(*p))
@pytest.mark.parametrize('nlon', cr.ROWS_NLON)
def test_rows_kernel(nlon, pair):
    """P < 16 (no full K tile), P % 16 == 0 (no tail), the clamped table loads and the row guard of nlon = 124, 127, 247 and bands
    with lat0 > 0"""
    N, nmin = pair
    P = cr.size(N, nmin)
    ref = reference('general', N, nmin, cr.ROWS_NLAT, nlon)
    plan = plan_of(N, cr.ROWS_NLAT, nlon)
    direct_case('ROWS', plan, device_matrix(cr.small_matrix('general', P)), nmin, ref, cr.ROWS_BANDS, 'rows kernel nlon {0} P {1}'.format(nlon, P))


# ---- general kernel: Sigma copied to LDS (even P, aligned base), register path (odd P; even P on a base 8 bytes off)
@pytest.mark.parametrize('pair', cr.DEGREE_PAIRS, ids=lambda p: 'N{0}min{1}'.format(*p))
@pytest.mark.parametrize('shape', cr.GENERAL_SHAPES, ids=lambda s: '{0}x{1}'.format(s[1], s[0]))
def test_general_kernel(shape, pair):
    """row blocks that span many parallels (nlon 1 and 3), both sides of the rows-kernel seams (123, 129, 130), bands that end at
    the last parallel (the Legendre descriptor returns zeros to the speculative tile) and bands that do not"""
    (nlon, nlat), (N, nmin) = shape, pair
    P = cr.size(N, nmin)
    S = cr.small_matrix('general', P)
    ref = reference('general', N, nmin, nlat, nlon)
    plan, bands = plan_of(N, nlat, nlon), cr.general_bands(nlat)
    what = 'general kernel {0} x {1} P {2}'.format(nlat, nlon, P)
    if P % 2 == 0:
        direct_case('DIRECT', plan, device_matrix(S), nmin, ref, bands, what + ' LDS copy')
        direct_case('REGISTER', plan, device_matrix(S, odd_base=True), nmin, ref, bands, what + ' registers, odd base')
    else:
        direct_case('REGISTER', plan, device_matrix(S), nmin, ref, bands, what + ' registers')


# ---- symmetric kernel
@pytest.mark.parametrize('pair', cr.SYMMETRIC_PAIRS, ids=lambda p: 'N{0}min{1}'.format(*p))
@pytest.mark.parametrize('shape', cr.GENERAL_SHAPES, ids=lambda s: '{0}x{1}'.format(s[1], s[0]))
def test_symmetric_kernel_reads_the_upper_triangle_only(shape, pair):
    """the symmetric matrix as it is, and with NaN in the whole strict lower triangle: the same bits.  M = 130 (130 x 1, one parallel
    of 3 x 130) keeps rows 60 .. 63 of a wave tile in play."""
    (nlon, nlat), (N, nmin) = shape, pair
    P = cr.size(N, nmin)
    S = cr.small_matrix('symmetric', P)
    ref = reference('symmetric', N, nmin, nlat, nlon)
    plan, bands = plan_of(N, nlat, nlon), cr.general_bands(nlat)
    what = 'symmetric kernel {0} x {1} P {2}'.format(nlat, nlon, P)
    clean = direct_case('SYMMETRIC', plan, device_matrix(S), nmin, ref, bands, what, symmetric=True)
    junk = np.array(S)
    junk[np.tril_indices(P, -1)] = np.nan
    poisoned = direct_case('SYMMETRIC', plan, device_matrix(junk), nmin, ref, bands, what + ', NaN below the diagonal', symmetric=True)
    assert np.array_equal(poisoned, clean)


# ---- padded copy of Sigma
@pytest.mark.parametrize('pair', cr.PADDED_PAIRS, ids=lambda p: 'N{0}min{1}'.format(*p))
def test_padded_copy(pair):
    """odd P with M P^2 > 1e12 on 180 x 360: rows of P + 1 doubles (3970), and of P + 3 where P + 1 is a multiple of 512 (4098)"""
    N, nmin = pair
    nlon, nlat = cr.PADDED_GRID
    P = cr.size(N, nmin)
    assert cr.padded_row_length(P) == {3969: 3970, 4095: 4098}[P]
    S = cr.general_matrix(1000 + N, P)
    colat, kn, lon = cr.grid_tables(cr.GRID_SEED, N, nlat, nlon)
    rows = cr.padded_rows()
    ref, norm = cr.sigma_grid(S, nmin, N, colat, kn, lon, rows=rows, with_norm=True)
    cr.assert_positive(ref, norm, pair)
    plan, cov = plan_of(N, nlat, nlon), device_matrix(S)
    expect_route('PADDED', plan, cov, (0, nlat))
    full = propagate(plan, cov, nmin)
    assert np.all(np.isfinite(full))
    check(full[rows], ref, 'padded copy P {0}'.format(P))
    sep = propagate(plan, cov, nmin, method='separable')
    worst = float(np.max(np.abs(sep - full)) / np.max(np.abs(full)))
    print('padded copy P {0} against the separable chain: {1:.2e}'.format(P, worst))
    assert worst < 1e-12


# ---- separable chain, full and half
@pytest.mark.parametrize('pair', [p for p in cr.separable_pairs() if cr.size(*p) > 0], ids=lambda p: 'N{0}min{1}'.format(*p))
def test_separable_chain(pair):
    """S = 1, 5, 31, 33, 63, 65 slots (one ragged chunk, the chunk seam between the cosine and the sine slot of order 16, two and
    three chunks), 1, 31 and 33 parallels as whole grids and as bands from parallel 2 on.  Half: the symmetric matrix clean and with
    NaN wherever slot(p) < slot(q), the entries shg_covprop_diag_separable_symmetric does not read: the same bits."""
    N, nmin = pair
    P, nlon, lat0 = cr.size(N, nmin), cr.SEPARABLE_NLON, cr.SEPARABLE_LAT0
    ref = {kind: reference(kind, N, nmin, cr.SEPARABLE_NLAT, nlon) for kind in ('general', 'symmetric')}
    general, symmetric = cr.small_matrix('general', P), cr.small_matrix('symmetric', P)
    slot = cr.slots(N, nmin)
    junk = np.array(symmetric)
    junk[slot[:, None] < slot[None, :]] = np.nan
    general, symmetric, junk = device_matrix(general), device_matrix(symmetric), device_matrix(junk)
    for nb in cr.SEPARABLE_NB:
        for plan, band in ((plan_of(N, nb, nlon), (0, nb)), (plan_of(N, cr.SEPARABLE_NLAT, nlon), (lat0, lat0 + nb))):
            what = 'separable S {0} P {1} parallels {2} of {3}'.format(2 * N + 1, P, band, plan.nlat)
            check(propagate(plan, general, nmin, band, method='separable'), band_rows(ref['general'], band, nlon), what + ' full')
            half = propagate(plan, symmetric, nmin, band, method='separable', symmetric=True)
            check(half, band_rows(ref['symmetric'], band, nlon), what + ' half')
            assert np.array_equal(propagate(plan, junk, nmin, band, method='separable', symmetric=True), half), what + ' half, NaN in the unread entries'


def test_separable_chain_across_the_permute_segment():
    """P = 8281 > 8192: the rows of Sigma pass through covsep_permute_kernel in two segments"""
    N, nmin, nlat, nlon = cr.PERMUTE_CASE
    P = cr.size(N, nmin)
    assert P == 8281
    S = cr.general_matrix(1000 + N, P)
    colat, kn, lon = cr.grid_tables(cr.GRID_SEED, N, nlat, nlon)
    ref, norm = cr.sigma_grid(S, nmin, N, colat, kn, lon, with_norm=True)
    cr.assert_positive(ref, norm, cr.PERMUTE_CASE)
    check(propagate(plan_of(N, nlat, nlon), device_matrix(S), nmin, method='separable'), ref, 'separable across the permute segment')


# ---- no coefficients, no parallels
ENTRY_POINTS = {'shg_covprop_diag': {}, 'shg_covprop_diag_symmetric': {'symmetric': True}, 'shg_covprop_diag_separable': {'method': 'separable'},
                'shg_covprop_diag_separable_symmetric': {'method': 'separable', 'symmetric': True}}


@pytest.mark.parametrize('name', sorted(ENTRY_POINTS))
def test_no_degrees_gives_zeros_and_an_empty_band_writes_nothing(name):
    import torch
    N, nlat, nlon = 3, 3, 130
    plan = plan_of(N, nlat, nlon)
    empty = torch.empty((0, 0), dtype=torch.float64, device='cuda')
    assert propagate(plan, empty, N + 1, (1, 3), **ENTRY_POINTS[name]).tolist() == [0.0] * (2 * nlon)
    cov = device_matrix(cr.small_matrix('symmetric', 16))
    out = torch.full((2 * nlon,), -7.0, dtype=torch.float64, device='cuda')
    _lib.call(name, plan._handle, ctypes.c_void_p(cov.data_ptr()), 0, 2, 2, ctypes.c_void_p(out.data_ptr()), engine._stream())
    assert engine.to_host(out).tolist() == [-7.0] * (2 * nlon)


@pytest.mark.parametrize('name', sorted(ENTRY_POINTS))
def test_guard_behind_the_output(name):
    """C ABI: the output buffer is longer than the band; what lies behind the band stays as it was"""
    import torch
    N, nmin, nlat, nlon, band = 16, 0, 3, 130, (1, 3)
    plan, M = plan_of(N, nlat, nlon), 2 * nlon
    cov = device_matrix(cr.small_matrix('symmetric', cr.size(N, nmin)))
    want = propagate(plan, cov, nmin, band, **ENTRY_POINTS[name])
    out = torch.full((M + 300,), -7.0, dtype=torch.float64, device='cuda')
    _lib.call(name, plan._handle, ctypes.c_void_p(cov.data_ptr()), nmin, band[0], band[1], ctypes.c_void_p(out.data_ptr()), engine._stream())
    got = engine.to_host(out)
    assert np.array_equal(got[:M], want) and got[M:].tolist() == [-7.0] * 300
    check(got[:M], band_rows(reference('symmetric', N, nmin, nlat, nlon), band, nlon), name)


# ---- shg_symmetry_defect
def defect_of(S, n, ld):
    """through the C ABI, with NaN in the padding of the rows and a stale value in the output"""
    import torch
    host = np.full((n, ld), np.nan)
    host[:, :n] = S
    dev = engine.to_device(host)
    out = torch.full((1,), 5.0, dtype=torch.float64, device='cuda')
    _lib.call('shg_symmetry_defect', ctypes.c_void_p(dev.data_ptr()), n, ld, ctypes.c_void_p(out.data_ptr()), engine._stream())
    return float(out.item())


@pytest.mark.parametrize('pad', (0, 3))
@pytest.mark.parametrize('n', (1, 31, 32, 33, 65))
def test_symmetry_defect(n, pad):
    """exactly |S[p][q] - S[q][p]| of numpy for one differing pair in the corner tile, its mirror image and the last (partial) diagonal
    tile; 0.0 for a symmetric matrix; never 0.0 when one side of a pair is NaN or infinite"""
    S = cr.symmetric_matrix(77, n)
    assert defect_of(S, n, n + pad) == 0.0
    if n == 1:
        return
    for p, q in ((0, n - 1), (n - 1, 0), (n - 2, n - 1), (n - 1, n - 2)):
        T = S.copy()
        T[p, q] += 0.3
        assert defect_of(T, n, n + pad) == abs(T[p, q] - T[q, p]) > 0.0, (p, q)
        two = T.copy()
        two[1, 0] += 1e-3                                          # a second, smaller defect does not hide the first
        assert defect_of(two, n, n + pad) == abs(T[p, q] - T[q, p]), (p, q)
        for bad in (np.nan, np.inf, -np.inf):
            T[p, q] = bad
            got = defect_of(T, n, n + pad)
            assert got != 0.0, (p, q, bad)
            assert got == np.inf or np.isnan(got), (p, q, bad, got)


@pytest.mark.parametrize('where', ((5, 2), (128, 3), (2, 5)))
def test_automatic_choice_keeps_the_general_path_for_a_nan_on_one_side(where):
    """symmetric=None: a NaN at (p, q) beside a finite (q, p) is no symmetric matrix; the result is the one of symmetric=False"""
    N, nmin, nlat, nlon = 22, 20, 2, 123
    S = np.array(cr.small_matrix('symmetric', 129))
    S[where] = np.nan
    plan, cov = plan_of(N, nlat, nlon), device_matrix(S)
    np.testing.assert_array_equal(propagate(plan, cov, nmin, symmetric=None), propagate(plan, cov, nmin, symmetric=False))
    np.testing.assert_array_equal(propagate(plan, cov, nmin, symmetric=None, method='separable'), propagate(plan, cov, nmin, method='separable'))
    clean = device_matrix(cr.small_matrix('symmetric', 129))
    assert np.array_equal(propagate(plan, clean, nmin, symmetric=None), propagate(plan, clean, nmin, symmetric=True))


def test_case_list_reaches_every_route():
    """from the case lists above: each kind of shg_covprop_route_kind is run by at least one case"""
    planned = {'NONE'}                                                                             # test_no_degrees_gives_zeros_...
    planned |= {cr.route(nlon, cr.size(*p), True, cr.ROWS_NLAT * nlon, False) for nlon in cr.ROWS_NLON for p in cr.DEGREE_PAIRS}
    for nlon, nlat in cr.GENERAL_SHAPES:
        for p in cr.DEGREE_PAIRS:
            planned |= {cr.route(nlon, cr.size(*p), aligned, nlon * nlat, False) for aligned in ((True, False) if cr.size(*p) % 2 == 0 else (True,))}
        planned |= {cr.route(nlon, cr.size(*p), True, nlon * nlat, True) for p in cr.SYMMETRIC_PAIRS}
    planned |= {cr.route(cr.PADDED_GRID[0], cr.size(*p), True, cr.PADDED_GRID[0] * cr.PADDED_GRID[1], False) for p in cr.PADDED_PAIRS}
    assert planned == set(cr.ROUTES) == set(engine.COVPROP_ROUTE_KINDS)
