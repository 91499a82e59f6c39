"""
Basin functionals, basin covariances and basin averages on the GPU (Grid.basin_functionals / basin_covariance / basin_averages):
against the reference (tests/golden/g21_basin_covariance.npz), against an independent path through synthesised grids and
basin_statistics at full size, against engine.congruence, and for the kernel's contract (upper triangle only, exact symmetry,
bitwise reproducibility, filtered fields, the analysis left untouched).
"""
import datetime

import numpy as np
import pytest

import basin_covariance_inputs as ci
import basin_inputs as bi
import grates_amd as ga

pytestmark = pytest.mark.gpu


def _masks(g, gtag):
    n = int(g['count_' + gtag][0])
    return np.unpackbits(g['masks_' + gtag], axis=1, count=n).astype(bool)


def _close(value, ref, tol, what):
    value = ga.engine.to_host(value) if not isinstance(value, np.ndarray) else value
    assert value.shape == ref.shape, what
    finite = np.isfinite(ref)
    assert np.array_equal(np.isfinite(value), finite), what
    err = np.abs(value[finite] - ref[finite]).max()
    assert err <= tol * np.abs(ref[finite]).max(), '{0}: {1:.3e} relative'.format(what, err / np.abs(ref[finite]).max())


@pytest.mark.parametrize('case', ci.CASES, ids=[ci.tag(*c) for c in ci.CASES])
def test_functionals_and_covariance_match_reference(golden, case):
    g = golden('g21_basin_covariance')
    gtag, kernel, nmin = case
    grid = dict(ci.grids(ga.grid))[gtag]
    masks = _masks(g, gtag)
    t = ci.tag(*case)
    S = ci.sigma(*ci.covariance(nmin))
    _close(grid.basin_functionals(masks, nmin, ci.MAX_DEGREE, kernel), g['F_' + t], 1e-12, 'F ' + t)
    C = grid.basin_covariance(S, masks, nmin, ci.MAX_DEGREE, kernel)
    _close(C, g['C_' + t], 1e-12, 'C ' + t)
    if case in ci.FILTERED:
        flt = ga.filter.Gaussian(ci.FILTER_RADIUS)
        _close(grid.basin_functionals(masks, nmin, ci.MAX_DEGREE, kernel, spatial_filter=flt), g['FW_' + t], 1e-12, 'FW ' + t)
        _close(grid.basin_covariance(S, masks, nmin, ci.MAX_DEGREE, kernel, spatial_filter=flt), g['CW_' + t], 1e-12, 'CW ' + t)


def _basins16(grid):
    basins = []
    for k in range(8):
        lon0, lat0 = -170.0 + 42.0 * k, -60.0 + 15.0 * k
        basins.append(ga.grid.Basin.from_extent(*np.deg2rad([lon0, lat0, lon0 + 20.0 + 3 * k, lat0 + 8.0 + 2 * k])))
        basins.append(ga.grid.Basin(bi.star(200 + 50 * k, -150.0 + 40.0 * k, 50.0 - 12.0 * k, 0.1 + 0.05 * k, 100 + k)))
    return np.array([grid.create_mask(b) for b in basins])


def _series(N, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, N + 1, N + 1)) * 1e-10 / (1.0 + np.arange(N + 1))[None, None, :] ** 1.5
    return x


@pytest.fixture(scope='module')
def full_size():
    grid = ga.grid.GeographicGrid(0.25, 0.25)
    return grid, _basins16(grid)


def test_full_size_means_and_covariance_against_grid_path(full_size):
    torch = ga.engine.require_gpu()
    grid, masks = full_size
    N, T = 96, 240
    x = _series(N, T, 7)
    epochs = [datetime.datetime(2002, 1, 1) + datetime.timedelta(days=30 * k) for k in range(T)]
    series = ga.gravityfield.TimeSeries.from_series(x, epochs)
    means = grid.basin_averages(series, masks)
    ref = grid.basin_statistics(series.to_grid(grid, 'ewh', as_tensor=True), masks)[0]
    assert tuple(means.shape) == (T, 16)
    err = (means - ref).abs().max().item()
    assert err <= 1e-12 * ref.abs().max().item(), err / ref.abs().max().item()
    # covariance of L L^T against M M^T, M[b, k] = basin mean of the field of column k of L, through grids
    Pn = (N + 1) ** 2
    K = 24
    xk = _series(N, K, 8)
    L = ga.engine.ravel(ga.engine.to_device(xk), 0, N).t().contiguous()          # [Pn, K]
    S = ga.engine.gemm(L, L, transb=True)
    assert tuple(S.shape) == (Pn, Pn)
    C = grid.basin_covariance(S, masks, 0, N)
    M = grid.basin_statistics(ga.gravityfield.synthesize(ga.engine.to_device(xk), grid), masks)[0].t()       # [B, K]
    ref = M @ M.t()
    err = (C - ref).abs().max().item()
    assert err <= 1e-11 * ref.abs().max().item(), err / ref.abs().max().item()
    assert torch.equal(C, C.t())
    # the upper triangle only: NaN below the diagonal changes nothing
    S.masked_fill_(torch.ones_like(S, dtype=torch.bool).tril(-1), float('nan'))
    assert torch.equal(grid.basin_covariance(S, masks, 0, N), C)
    # reproducible
    F = grid.basin_functionals(masks, 0, N)
    assert torch.equal(F, grid.basin_functionals(masks, 0, N))
    assert torch.equal(grid.basin_covariance(S, masks, 0, N), C)


def test_against_congruence_64_masks():
    torch = ga.engine.require_gpu()
    grid = ga.grid.GeographicGrid(1.0, 1.0)
    rng = np.random.default_rng(31)
    masks = []
    for k in range(64):
        lon0, lat0 = rng.uniform(-175, 150), rng.uniform(-85, 60)
        masks.append(grid.create_mask(ga.grid.Basin.from_extent(*np.deg2rad([lon0, lat0, lon0 + rng.uniform(5, 25), lat0 + rng.uniform(5, 25)]))))
    masks = np.array(masks)
    N = 96
    Pn = (N + 1) ** 2
    F = grid.basin_functionals(masks, 0, N)
    L = ga.engine.to_device(rng.standard_normal((Pn, 48)))
    S = ga.engine.gemm(L, L, transb=True) + torch.diag(ga.engine.to_device(rng.uniform(0.5, 1.5, Pn)))
    C = ga.engine.basin_covariance(F, S)
    ref = ga.engine.congruence(F, S)
    assert tuple(C.shape) == (64, 64)
    assert torch.equal(C, C.t())
    err = (C - ref).abs().max().item()
    assert err <= 1e-13 * ref.abs().max().item(), err / ref.abs().max().item()
    for B in (1, 5, 17, 40):                          # every row tile count, partial tiles
        sub = ga.engine.basin_covariance(F[:B].contiguous(), S)
        assert (sub - ref[:B, :B]).abs().max().item() <= 1e-13 * ref.abs().max().item(), B


def _ddk_like(N, seed):
    rng = np.random.default_rng(seed)
    blocks = []
    for s in range(2 * N + 1):
        m = (s + 1) // 2
        d = N + 1 - m
        A = rng.standard_normal((d, d)) * 0.02
        W = np.eye(d) * np.exp(-np.arange(m, N + 1) / 20.0)[:, None] + A @ A.T / d
        for a in range(d):                         # degrees 0 and 1 pass unchanged (filter() restores them from the input)
            if m + a < 2:
                W[a, :] = 0.0
                W[:, a] = 0.0
                W[a, a] = 1.0
        blocks.append(W)
    return ga.filter.OrderWiseFilter(blocks)


def test_filtered_covariance_and_averages():
    torch = ga.engine.require_gpu()
    grid = ga.grid.GeographicGrid(1.0, 1.0)
    masks = _basins16(grid)
    N = 60
    flt = _ddk_like(N, 41)
    Pn = (N + 1) ** 2
    rng = np.random.default_rng(42)
    L = rng.standard_normal((Pn, 30)) * 1e-10
    S = L @ L.T
    C = grid.basin_covariance(S, masks, 0, N, spatial_filter=flt)
    ref = grid.basin_covariance(flt.filter_covariance(S, 0, N), masks, 0, N)
    assert (C - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    T = 12
    x = _series(N, T, 43)
    epochs = [datetime.datetime(2005, 1 + k, 1) for k in range(T)]
    series = ga.gravityfield.TimeSeries.from_series(x, epochs)
    means = grid.basin_averages(flt.filter(series), masks)
    FW = grid.basin_functionals(masks, 0, N, spatial_filter=flt)
    ref = ga.engine.gemm(ga.engine.ravel(ga.engine.to_device(x), 0, N), FW, transb=True)
    assert (means - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    # the same means from a host series, one field, and a raw batch
    host = ga.gravityfield.TimeSeries(series._fields())
    assert (grid.basin_averages(host, masks) - grid.basin_averages(ga.engine.to_device(x), masks)).abs().max().item() == 0.0
    one = grid.basin_averages(host[3], masks)
    assert tuple(one.shape) == (1, 16)


def test_analysis_unchanged_by_functionals():
    torch = ga.engine.require_gpu()
    grid = ga.grid.GeographicGrid(1.0, 1.0)
    N = 60
    plan = grid._basin_plan('ewh', N, 3.9860044150e+14, 6.3781363000e+06)
    area = ga.engine.to_device(grid.area.reshape(grid.parallels.size, grid.meridians.size))
    rng = np.random.default_rng(5)
    values = ga.engine.to_device(rng.standard_normal((8, grid.parallels.size, grid.meridians.size)))
    before = plan.analysis(values, area, 2, trusted_weights=False)
    masks = _basins16(grid)
    grid.basin_functionals(masks, 2, N)
    grid.basin_functionals(masks, 0, N)
    after = plan.analysis(values, area, 2, trusted_weights=False)
    assert torch.equal(before, after)


@pytest.mark.parametrize('min_degree', [0, 1])
def test_multi_block_pieces_against_congruence(min_degree):
    """d/o 140: Pn = 19881 (odd leading dimension, 8-byte loads) or 19880 (even, 16-byte loads); the launch cuts every column block
    into pieces of two block heights, the last block and the last piece of a column are partial"""
    torch = ga.engine.require_gpu()
    N = 140
    Pn = (N + 1) ** 2 - min_degree ** 2
    gen = torch.Generator(device=ga.engine.device()).manual_seed(140 + min_degree)
    S = torch.randn((Pn, Pn), dtype=torch.float64, device=ga.engine.device(), generator=gen)
    S = S + S.t()
    F = torch.randn((3, Pn), dtype=torch.float64, device=S.device, generator=gen)
    C = ga.engine.basin_covariance(F, S)
    ref = ga.engine.congruence(F, S)
    assert torch.equal(C, C.t())
    err = (C - ref).abs().max().item()
    assert err <= 1e-12 * ref.abs().max().item(), err / ref.abs().max().item()
    del S
    torch.cuda.empty_cache()


@pytest.mark.parametrize('dlon, N', [(4.0, 20), (1.0, 130)], ids=['no-fourfold-symmetry', 'degree-above-126'])
def test_functionals_of_other_transform_branches_against_grid_path(dlon, N):
    """a grid whose meridian count is not a multiple of 4 (weight transpose + GEMM) and d/o 130 (fold + GEMMs) against the means
    of synthesised grids"""
    grid = ga.grid.GeographicGrid(dlon, dlon)
    info = grid._basin_plan('ewh', N, 3.9860044150e+14, 6.3781363000e+06).info()
    assert info['fourfold_symmetry'] == (N > 126)
    masks = _basins16(grid)
    x = _series(N, 6, 51)
    F = grid.basin_functionals(masks, 0, N)
    means = ga.engine.gemm(ga.engine.ravel(ga.engine.to_device(x), 0, N), F, transb=True)
    ref = grid.basin_statistics(ga.gravityfield.synthesize(ga.engine.to_device(x), grid), masks)[0]
    _close(means, ga.engine.to_host(ref), 1e-12, 'means')
