"""
From node values of radial basis functions to maps, on the GPU: the surface synthesis of shg_rbf_surface (RadialBasisFunctions.surface_matrix,
.synthesize, engine.rbf_surface), its formal errors (.covariance_propagation: engine.gemm and shg_column_dots) and the basin means
(.basin_functionals, .basin_averages, .basin_covariance): against the reference's route through spherical harmonics
(tests/golden/g31_rbf_surface.npz), against the package's own spherical harmonic route on the GPU (the check that needs no reference), for
the kernels' contracts at their seams (an entry depends on its point and its node only; a column dot product on the rows only) and at
the end of the road from observations to a map.

The bounds against the fixture are 4 times the figures its generator recorded for the float64 restatement (rbf_surface_inputs.surface:
the kernel has no transcendental function, so it follows the restatement to the last bit).
"""
import ctypes
import functools

import numpy as np
import pytest

import grates_amd as ga
import rbf_inputs as ri
import rbf_surface_inputs as si

pytestmark = pytest.mark.gpu

GM, R = si.GM, si.R
U = 2.0 ** -53


def _host(t):
    return t if isinstance(t, np.ndarray) else ga.engine.to_host(t)


def _basis(lon, lat, k, min_degree, a=si.A, f=si.F):
    return ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat, a=a, f=f), ri.shape_factors(k), min_degree, k.size - 1, GM, R)


def _grid(lon, lat, area=None):
    return ga.grid.IrregularGrid(lon, lat, area, a=si.A, f=si.F)


def _own_factors(kernel, max_degree, glat):
    """kn [M, N + 1] as the package builds it on the host: what engine.rbf_surface_tables uploads, degree-major"""
    return ga.gravityfield.surface_factors(ga.kernel.get_kernel(kernel), max_degree, glat, GM, R, si.A, si.F)[2]


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', sorted(si.CASES))
def test_surface_matrix_and_sigmas_match_the_reference(golden, tag):
    data = golden('g31_rbf_surface')
    min_degree, max_degree, count, _ = si.CASES[tag]
    lon, lat, k, glon, glat = (data[name + tag] for name in ('lon_', 'lat_', 'k_', 'glon_', 'glat_'))
    basis, grid = _basis(lon, lat, k, min_degree), _grid(glon, glat)
    C = si.covariance(count, si.COVARIANCE_SEED[tag])
    failures = []
    for i, kernel in enumerate(si.KERNELS):
        S_ref, sigma_ref = data['S_{0}_{1}'.format(tag, kernel)], data['sigma_{0}_{1}'.format(tag, kernel)]
        S = basis.surface_matrix(grid, kernel)
        sigma = basis.covariance_propagation(grid, C, kernel)
        assert isinstance(S, np.ndarray) and S.shape == S_ref.shape and isinstance(sigma, np.ndarray) and sigma.shape == sigma_ref.shape
        assert np.all(np.isfinite(S)) and np.all(np.isfinite(sigma)) and grid.values is None              # the grid is not modified
        rows = np.abs(S - S_ref).max(axis=1) / np.abs(S_ref).max()
        sigma_err = np.abs(sigma - sigma_ref).max() / sigma_ref.max()
        restated = si.surface(ri.node_table(lon, lat), k, min_degree, si.unit_vectors(glon, glat), _own_factors(kernel, max_degree, glat))
        bits = np.abs(S - restated).max() / np.abs(S_ref).max()
        print('{0} {1}: S {2:.2e} of max|S| (bound {3:.2e}), above and antipodal to a node {4:.2e}; sigma {5:.2e} of the largest (bound {6:.2e}); '
              '{7:.2e} from the restatement'.format(tag, kernel, rows.max(), 4 * data['S_err_' + tag][i], rows[si.SCATTERED:].max(), sigma_err,
                                                    4 * data['sigma_err_' + tag][i], bits))
        if not (rows.max() <= 4 * data['S_err_' + tag][i] and sigma_err <= 4 * data['sigma_err_' + tag][i] and np.array_equal(S, restated)):
            failures.append(kernel)
    assert not failures


def test_degree_96_matches_the_reference(golden):
    data = golden('g31_rbf_surface')
    c = si.N96
    basis, grid = _basis(data['lon_n96'], data['lat_n96'], data['k_n96'], c['min_degree']), _grid(data['glon_n96'], data['glat_n96'])
    S = basis.surface_matrix(grid, c['kernel'])
    sigma = basis.covariance_propagation(grid, si.covariance(ri.N96['nodes'], si.COVARIANCE_SEED['n96']), c['kernel'])
    S_err = np.abs(S - data['S_n96']).max() / np.abs(data['S_n96']).max()
    sigma_err = np.abs(sigma - data['sigma_n96']).max() / data['sigma_n96'].max()
    print('d/o 96, 60 points, 8 nodes: S {0:.2e} of max|S| (bound {1:.2e}), sigma {2:.2e} of the largest (bound {3:.2e})'.format(
        S_err, 4 * float(data['S_err_n96']), sigma_err, 4 * float(data['sigma_err_n96'])))
    assert S.shape == (c['points'], ri.N96['nodes']) and S_err <= 4 * float(data['S_err_n96']) and sigma_err <= 4 * float(data['sigma_err_n96'])


# ---- the check that needs no reference ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _package_case():
    c = si.PACKAGE
    basis = _basis(*si.package_nodes(), ri.degree_factors(c['min_degree'], c['max_degree']), c['min_degree'])
    basis.values = si.package_values()
    return basis, si.package_points()


@pytest.mark.parametrize('kernel', ('ewh', 'geoid'))
def test_surface_route_is_the_spherical_harmonic_route(golden, kernel):
    """band 2..12, 40 nodes, 300 points, both sides on the GPU: S against the grid's synthesis matrix times F =
    to_potential_coefficients_matrix(), synthesize against to_grid of to_potential_coefficients(), covariance_propagation against the
    point-list propagation (shg_covprop_points) of F C F^T.  The bounds are 4 times the fixture's figures of the nearest band (2..8)."""
    data = golden('g31_rbf_surface')
    c = si.PACKAGE
    i = si.KERNELS.index(kernel)
    S_bound, sigma_bound = 4 * data['S_err_' + c['nearest']][i], 4 * data['sigma_err_' + c['nearest']][i]
    basis, (glon, glat) = _package_case()
    grid = _grid(glon, glat)
    F = ga.engine.to_device(basis.to_potential_coefficients_matrix())
    S = basis.surface_matrix(grid, kernel, as_tensor=True)
    composed = ga.engine.gemm(grid.synthesis_matrix_device(c['min_degree'], c['max_degree'], kernel, GM, R), F)
    S_err = float((S - composed).abs().max().item() / composed.abs().max().item())
    values = basis.synthesize(grid, kernel)
    through = basis.to_potential_coefficients().to_grid(grid, kernel).values
    value_err = np.abs(values - through).max() / np.abs(through).max()
    C = si.covariance(c['nodes'], c['covariance_seed'])
    sigma = basis.covariance_propagation(grid, C, kernel)
    propagated = _grid(glon, glat).covariance_propagation(_host(ga.engine.congruence(F, ga.engine.to_device(C))), c['min_degree'], c['max_degree'], kernel, GM, R)
    sigma_err = np.abs(sigma - propagated).max() / propagated.max()
    print('{0}: S {1:.2e} of max|S| and synthesize {2:.2e} of the largest value (bound {3:.2e}); sigma {4:.2e} of the largest (bound {5:.2e})'.format(
        kernel, S_err, value_err, S_bound, sigma_err, sigma_bound))
    assert tuple(S.shape) == (c['points'], c['nodes']) and values.shape == sigma.shape == (c['points'],)
    assert S_err <= S_bound and value_err <= S_bound and sigma_err <= sigma_bound


# ---- seams and contracts ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seam_case():
    """band 2..8, tile + 5 nodes, 700 grid points (two full workgroups and a partial one), ewh: (lon, lat, k, points [700, 3], kn_t [9, 700])"""
    tile = ga.engine.rbf_surface_info()[0]
    lon, lat = ri.scattered_nodes(tile + 5, 3141)
    k = ri.degree_factors(2, 8)
    points, kn_t = ga.engine.rbf_surface_tables(_grid(*ri.scattered_nodes(700, 3142)), 'ewh', _basis(lon, lat, k, 2))
    return lon, lat, k, points, kn_t


def _seam_basis(J):
    lon, lat, k = _seam_case()[:3]
    return _basis(lon[:J], lat[:J], k, 2)


def test_entries_do_not_depend_on_the_batch():
    """M in {1, 255, 256, 257, 700} and J in {1, T - 1, T, T + 1, T + 5}, a slice and a permutation of the points: the entry of a point and
    a node is the same bits whatever the batch, the node count and the place of the point; two runs are bit-identical"""
    import torch
    tile = ga.engine.rbf_surface_info()[0]
    points, kn_t = _seam_case()[3:]
    assert tuple(points.shape) == (700, 3) and tuple(kn_t.shape) == (9, 700) and bool((kn_t[:2] == 0.0).all())
    full = ga.engine.rbf_surface(_seam_basis(tile + 5), points, kn_t)
    assert tuple(full.shape) == (tile + 5, 700) and bool(torch.isfinite(full).all()) and bool((full.abs().amax(dim=1) > 0).all())
    assert torch.equal(full, ga.engine.rbf_surface(_seam_basis(tile + 5), points, kn_t))
    for J in (1, tile - 1, tile, tile + 1, tile + 5):
        basis = _seam_basis(J)
        for M in (1, 255, 256, 257, 700):
            assert torch.equal(ga.engine.rbf_surface(basis, points[:M], kn_t[:, :M]), full[:J, :M]), (J, M)                # ldk = 700
            assert torch.equal(ga.engine.rbf_surface(basis, points[:M], kn_t[:, :M].contiguous()), full[:J, :M]), (J, M)   # ldk = M
    basis = _seam_basis(tile + 1)
    for first, last in ((699, 700), (256, 700), (300, 557), (1, 258)):
        assert torch.equal(ga.engine.rbf_surface(basis, points[first:last], kn_t[:, first:last]), full[:tile + 1, first:last]), (first, last)
    order = torch.from_numpy(np.random.default_rng(3143).permutation(700)).to(points.device)
    assert torch.equal(ga.engine.rbf_surface(_seam_basis(tile + 5), points[order].contiguous(), kn_t[:, order].contiguous()), full[:, order])


def test_rows_below_the_band_are_never_read():
    """NaN in the rows of kn below min_degree: the same bits as zeros"""
    import torch
    tile = ga.engine.rbf_surface_info()[0]
    points, kn_t = _seam_case()[3:]
    poisoned = kn_t.clone()
    poisoned[:2] = float('nan')
    basis = _seam_basis(tile + 5)
    assert torch.equal(ga.engine.rbf_surface(basis, points, poisoned), ga.engine.rbf_surface(basis, points, kn_t))


def test_leading_dimensions_beyond_the_points():
    """ldt = 300 and ldk = 300 for 257 points through the C entry point: the same bits, and the entries from M to ldt of a row of St are
    not touched"""
    import torch
    from grates_amd import _lib
    tile = ga.engine.rbf_surface_info()[0]
    J, M, ld = tile + 1, 257, 300
    points, kn_t = _seam_case()[3:]
    basis = _seam_basis(J)
    shape, nodes = ga.engine.rbf_node_table(basis)
    p, kn = points[:M].contiguous(), kn_t[:, :ld].contiguous()
    out = torch.full((J, ld), 7.0, dtype=torch.float64, device=p.device)
    _lib.call('shg_rbf_surface', 8, 2, ctypes.c_void_p(shape.ctypes.data), ctypes.c_void_p(nodes.data_ptr()), J, ctypes.c_void_p(p.data_ptr()),
              ctypes.c_void_p(kn.data_ptr()), ld, M, ctypes.c_void_p(out.data_ptr()), ld, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert torch.equal(out[:, :M], ga.engine.rbf_surface(basis, points[:M], kn_t[:, :M])) and bool((out[:, M:] == 7.0).all())


def test_regular_grid_equals_the_list_of_its_points():
    lon, lat, k = _seam_case()[:3]
    basis = _basis(lon, lat, k, 2)
    regular = ga.grid.GeographicGrid(30, 30, a=si.A, f=si.F)
    listed = _grid(regular.longitude, regular.latitude)
    for kernel in ('ewh', 'potential'):
        S = basis.surface_matrix(regular, kernel)
        assert S.shape == (72, lon.size) and np.array_equal(S, basis.surface_matrix(listed, kernel))
    basis.values = np.random.default_rng(3144).standard_normal(lon.size)
    assert np.array_equal(basis.synthesize(regular), basis.synthesize(listed)) and regular.values is None


# ---- column dot products -----------------------------------------------------------------------------------------------------------------
def test_column_dots():
    """rows in {1, 63, 64, 65, 1000}, cols in {1, 255, 257}, leading dimensions above cols: within rows 2^-53 sum|x y| of the float64
    sequential sum (every product within 2^-53 of itself, every partial sum of at most rows terms), the bits of the restated order
    (rbf_surface_inputs.column_dots), independent of the batch and of the position of the column, and reproducible"""
    import torch
    rng = np.random.default_rng(3151)
    X, Y = rng.standard_normal((1000, 300)), rng.standard_normal((1000, 300))
    dX, dY = ga.engine.to_device(X), ga.engine.to_device(Y)
    for rows in (1, 63, 64, 65, 1000):
        sequential, magnitude = np.zeros(300), np.zeros(300)
        for r in range(rows):
            sequential = sequential + X[r] * Y[r]
            magnitude = magnitude + np.abs(X[r] * Y[r])
        whole = ga.engine.column_dots(dX[:rows], dY[:rows])
        assert tuple(whole.shape) == (300,) and torch.equal(whole, ga.engine.column_dots(dX[:rows], dY[:rows]))
        assert np.array_equal(_host(whole), si.column_dots(X[:rows], Y[:rows]))
        err = np.abs(_host(whole) - sequential) / (rows * U * magnitude)
        print('column_dots, {0} rows: {1:.3f} of rows 2^-53 sum|x y|'.format(rows, err.max()))
        assert err.max() <= 1.0
        for cols in (1, 255, 257):
            assert torch.equal(ga.engine.column_dots(dX[:rows, :cols], dY[:rows, :cols]), whole[:cols]), (rows, cols)                    # ld 300 > cols
            assert torch.equal(ga.engine.column_dots(dX[:rows, 43:43 + cols], dY[:rows, 43:43 + cols].contiguous()), whole[43:43 + cols]), (rows, cols)
    with pytest.raises(ValueError, match='one shape'):
        ga.engine.column_dots(dX[:5], dY[:6])


# ---- blocks ------------------------------------------------------------------------------------------------------------------------------
def test_blocks_of_points_give_the_same_bits():
    """block_points 100 over 257 points (100 + 100 + 57) against one block; a series [3, J] against three single calls"""
    basis, (glon, glat) = _package_case()
    grid = _grid(glon[:257], glat[:257])
    J = si.PACKAGE['nodes']
    C = si.covariance(J, si.PACKAGE['covariance_seed'])
    whole = basis.synthesize(grid)
    assert whole.shape == (257,) and np.array_equal(basis.synthesize(grid, block_points=100), whole)
    assert np.array_equal(basis.synthesize(grid, block_points=257), whole) and np.array_equal(basis.synthesize(grid, block_points=1000), whole)
    sigma = basis.covariance_propagation(grid, C)
    assert sigma.shape == (257,) and np.array_equal(basis.covariance_propagation(grid, C, block_points=100), sigma)
    assert np.array_equal(basis.covariance_propagation(grid, ga.engine.to_device(C), block_points=100), sigma)                # C on the device
    series = np.random.default_rng(3161).standard_normal((3, J))
    maps = basis.synthesize(grid, values=series, block_points=100)
    assert maps.shape == (3, 257)
    for t in range(3):
        assert np.array_equal(basis.synthesize(grid, values=series[t]), maps[t]), t
    assert np.array_equal(basis.synthesize(grid, values=basis.values), whole)
    on_device = basis.synthesize(grid, values=ga.engine.to_device(series), as_tensor=True)
    assert on_device.is_cuda and np.array_equal(_host(on_device), maps)


# ---- basins ------------------------------------------------------------------------------------------------------------------------------
def test_basin_means_and_their_covariance(golden):
    """two masks on 300 weighted points, ewh"""
    import torch
    data = golden('g31_rbf_surface')
    c = si.PACKAGE
    basis, (glon, glat) = _package_case()
    rng = np.random.default_rng(3171)
    area = rng.uniform(0.5, 2.0, c['points'])
    grid = _grid(glon, glat, area)
    masks = np.stack((glat > 0.2, (glon < 0.0) & (glat < 0.5)))
    assert masks.sum(axis=1).min() >= 30
    S = basis.surface_matrix(grid)
    F = basis.basin_functionals(grid, masks)
    expected = (area * masks) @ S / (area * masks).sum(axis=1)[:, None]
    F_err = np.abs(F - expected).max() / np.abs(S).max()
    bound = 4 * data['S_err_' + c['nearest']][si.KERNELS.index('ewh')]
    print('basin functionals: {0:.2e} of max|S| (bound {1:.2e})'.format(F_err, bound))
    assert isinstance(F, np.ndarray) and F.shape == (2, c['nodes']) and F_err <= bound
    on_device = basis.basin_functionals(grid, torch.from_numpy(masks), as_tensor=True)
    assert on_device.is_cuda and np.array_equal(_host(on_device), F)
    # the means are the functionals times the values: sums of J products
    means = _host(basis.basin_averages(grid, masks))
    assert means.shape == (2,) and np.all(np.abs(means - F @ basis.values) <= c['nodes'] * U * (np.abs(F) @ np.abs(basis.values)))
    series = rng.standard_normal((3, c['nodes']))
    many = _host(basis.basin_averages(grid, masks, values=series))
    assert many.shape == (3, 2) and np.all(np.abs(many - series @ F.T) <= c['nodes'] * U * (np.abs(series) @ np.abs(F.T)))
    # the covariance of the means
    C = si.covariance(c['nodes'], c['covariance_seed'])
    cov = basis.basin_covariance(grid, C, masks)
    assert torch.equal(cov, cov.t()) and tuple(cov.shape) == (2, 2)
    host = F @ C @ F.T
    cov_err = np.abs(_host(cov) - host).max() / np.abs(host).max()
    print('basin covariance: {0:.2e} of max|F C F^T| (bound 1e-13)'.format(cov_err))
    assert cov_err <= 1e-13
    lower_ignored = basis.basin_covariance(grid, np.triu(C) + np.tril(np.full_like(C, np.nan), -1), masks)
    assert torch.equal(lower_ignored, cov)                                                   # the contract of engine.basin_covariance
    # a basin of one point: its variance is that point's propagated variance, the quadratic form s^T C s of its row s of S twice;
    # either within (2 J + 4) 2^-53 of |s|^T |C| |s| (s within an ulp, J^2 products and their sums), together below 1e-13 of it
    sigma = basis.covariance_propagation(grid, C)
    for point in (0, 137, 299):
        one = np.zeros(c['points'], dtype=bool)
        one[point] = True
        variance = float(_host(basis.basin_covariance(grid, C, one))[0, 0])
        size = float(np.abs(S[point]) @ np.abs(C) @ np.abs(S[point]))
        assert abs(variance - sigma[point] ** 2) <= 1e-13 * size, point


# ---- the end of the road -----------------------------------------------------------------------------------------------------------------
def test_from_observations_to_a_map_with_error_bars(golden):
    """the closed loop of rbf_inputs.LOOP: planted node values, accelerations of their field, solve, compute_covariance(sparse=False); the
    map of the estimate is the map of the planted values within 10 times the host's relative error of the node values times cond(A)
    (|S dx| / |S x| <= cond |dx| / |x|, 2-norms, with the conditioning the fixture recorded for this geometry), and the formal errors of
    the map are finite and positive"""
    g29 = golden('g29_radial_basis')
    c = ri.LOOP
    lon, lat, a_nodes, f_nodes = ri.loop_nodes()
    basis = _basis(lon, lat, ri.degree_factors(c['min_degree'], c['max_degree']), c['min_degree'], a_nodes, f_nodes)
    basis.values = ri.loop_values()
    xyz = ri.loop_pairs()[0]
    ne = ga.lstsq.RadialBasisParameters(basis).from_accelerations(xyz, basis.to_potential_coefficients().gravitational_acceleration(xyz))
    estimate = _host(ne.solve())[:, 0]
    ne.compute_covariance(sparse=False)
    upper = np.triu(ne.matrix.to_array())                                                     # the inverse holds its upper triangle
    covariance = upper + np.triu(upper, 1).T
    grid = ga.grid.GeographicGrid(15, 15)
    planted = basis.synthesize(grid)
    solved = basis.synthesize(grid, values=estimate)
    rel = np.linalg.norm(solved - planted) / np.linalg.norm(planted)
    bound = 10 * float(g29['host_rel_err'][0]) * float(g29['loop_cond'][0])
    sigma = basis.covariance_propagation(grid, covariance)
    print('end of the road: map of the estimate {0:.2e} from the map of the planted values (bound {1:.2e}); sigma {2:.3e} .. {3:.3e}'.format(
        rel, bound, sigma.min(), sigma.max()))
    assert planted.shape == solved.shape == sigma.shape == (grid.point_count,) and rel <= bound
    assert np.all(np.isfinite(sigma)) and np.all(sigma > 0.0)
