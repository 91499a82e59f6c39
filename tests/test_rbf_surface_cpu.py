"""
CPU checks of the surface synthesis of radial basis functions: shg_rbf_surface and shg_column_dots reject bad arguments before any HIP
call, shg_rbf_surface_info is sane, the new engine functions and the six methods of RadialBasisFunctions have the listed signatures,
the Python layers refuse bad input before anything reaches the device, and the fixture g31_rbf_surface.npz is consistent with itself,
with the package's surface factors and with the float64 NumPy restatement of the kernels.
"""
import ctypes
import inspect

import numpy as np
import pytest

import grates_amd as ga
import rbf_inputs as ri
import rbf_surface_inputs as si

GM, R = si.GM, si.R


def _error(lib):
    return lib.shg_last_error().decode()


def _basis(tag='b2_8'):
    min_degree, max_degree = ri.CASES[tag][:2]
    lon, lat = ri.case_nodes(tag)
    K = ri.shape_factors(ri.degree_factors(min_degree, max_degree))
    return ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat, a=si.A, f=si.F), K, min_degree, max_degree, GM, R)


def _grid(tag='b2_8'):
    return ga.grid.IrregularGrid(*si.grid_points(tag), a=si.A, f=si.F)


def test_surface_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    shape = (ctypes.c_double * 9)(*([1.0] * 9))

    def call(N=8, min_degree=2, shape=shape, nodes=dummy, J=5, points=dummy, kn=dummy, ldk=10, M=10, St=dummy, ldt=10):
        return lib.shg_rbf_surface(N, min_degree, shape, nodes, J, points, kn, ldk, M, St, ldt, None)
    for bad in (dict(N=-1, min_degree=0), dict(min_degree=-1), dict(J=-1), dict(M=-1, ldk=0, ldt=0)):
        assert call(**bad) == -1
        assert 'shg_rbf_surface: negative size' in _error(lib)
    assert call(N=4, min_degree=5) == -1
    assert 'min_degree 5 above N 4' in _error(lib)
    assert call(N=32768) == -1
    assert 'N 32768 is too large' in _error(lib)
    most = ga.engine.rbf_surface_info()[3]
    assert call(J=most + 1) == -1
    assert 'above the {0} nodes of one call'.format(most) in _error(lib)
    assert call(ldk=9) == -1
    assert 'ldk 9 below M 10' in _error(lib)
    assert call(ldt=9) == -1
    assert 'ldt 9 below M 10' in _error(lib)
    assert call(J=1 << 19, M=1 << 22, ldk=1 << 22, ldt=1 << 22) == -1                          # 2^41 values
    assert 'is too large' in _error(lib)
    for missing in ('shape', 'nodes', 'points', 'kn', 'St'):
        assert call(**{missing: None}) == -1
        assert 'shg_rbf_surface: NULL pointer' in _error(lib)
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(M=0, ldk=0, ldt=0, shape=None, nodes=None, points=None, kn=None, St=None) == 0
    assert call(J=0, shape=None, nodes=None, points=None, kn=None, St=None) == 0
    with pytest.raises(_lib.ShgError, match='min_degree 3 above N 2'):
        _lib.call('shg_rbf_surface', 2, 3, shape, dummy, 5, dummy, dummy, 10, 10, dummy, 10, None)


def test_column_dots_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)

    def call(rows=7, cols=10, X=dummy, ldx=10, Y=dummy, ldy=10, out=dummy):
        return lib.shg_column_dots(rows, cols, X, ldx, Y, ldy, out, None)
    for bad in (dict(rows=-1), dict(cols=-1, ldx=0, ldy=0)):
        assert call(**bad) == -1
        assert 'shg_column_dots: negative size' in _error(lib)
    for bad in (dict(ldx=9), dict(ldy=9)):
        assert call(**bad) == -1
        assert 'below the 10 columns' in _error(lib)
    for missing in ('X', 'Y', 'out'):
        assert call(**{missing: None}) == -1
        assert 'shg_column_dots: NULL pointer' in _error(lib)
    assert call(rows=0, out=None) == -1                                                       # an empty sum still writes its zeros
    assert call(cols=0, ldx=0, ldy=0, X=None, Y=None, out=None) == 0
    with pytest.raises(_lib.ShgError, match='negative size'):
        _lib.call('shg_column_dots', -3, 10, dummy, 10, dummy, 10, dummy, None)


def test_info_is_sane_and_prototypes_are_present():
    from grates_amd import _lib
    tile, unroll, lanes, most = ga.engine.rbf_surface_info()
    assert lanes == 256 and 1 <= unroll <= tile <= 256 and tile % unroll == 0
    assert most == 65535 * tile
    assert _lib.load().shg_rbf_surface_info(None) == -1
    assert 'shg_rbf_surface_info: NULL pointer' in _error(_lib.load())
    assert len(_lib.PROTOTYPES['shg_rbf_surface']) == 12 and len(_lib.PROTOTYPES['shg_column_dots']) == 8
    assert _lib.PROTOTYPES['shg_rbf_surface_info'] == [ctypes.POINTER(ctypes.c_int)]


def test_signatures():
    def names(function):
        return list(inspect.signature(function).parameters)

    def defaults(function):
        return {name: prm.default for name, prm in inspect.signature(function).parameters.items() if prm.default is not inspect.Parameter.empty}
    engine, cls = ga.engine, ga.gravityfield.RadialBasisFunctions
    assert names(engine.rbf_surface_tables) == ['grid', 'kernel', 'basis']
    assert names(engine.rbf_surface) == ['basis', 'points', 'kn_t']
    assert names(engine.column_dots) == ['X', 'Y']
    assert names(cls.surface_matrix) == ['self', 'grid', 'kernel', 'as_tensor']
    assert names(cls.synthesize) == ['self', 'grid', 'kernel', 'values', 'as_tensor', 'block_points']
    assert names(cls.covariance_propagation) == ['self', 'grid', 'covariance_matrix', 'kernel', 'as_tensor', 'block_points']
    assert names(cls.basin_functionals) == ['self', 'grid', 'masks', 'kernel', 'as_tensor']
    assert names(cls.basin_averages) == ['self', 'grid', 'masks', 'kernel', 'values']
    assert names(cls.basin_covariance) == ['self', 'grid', 'covariance_matrix', 'masks', 'kernel']
    assert defaults(cls.surface_matrix) == dict(kernel='ewh', as_tensor=False)
    assert defaults(cls.synthesize) == dict(kernel='ewh', values=None, as_tensor=False, block_points=None)
    assert defaults(cls.covariance_propagation) == dict(kernel='ewh', as_tensor=False, block_points=None)
    assert defaults(cls.basin_functionals) == dict(kernel='ewh', as_tensor=False)
    assert defaults(cls.basin_averages) == dict(kernel='ewh', values=None)
    assert defaults(cls.basin_covariance) == dict(kernel='ewh')
    assert names(cls.to_grid) == ['self', 'grid', 'kernel']                                   # the reference's route stays as it is


def test_python_checks_run_before_the_device():
    """every ValueError fires on the host: on a machine without a GPU the first upload would raise a RuntimeError instead"""
    basis, grid = _basis(), _grid()
    J, M = 24, grid.point_count
    C, mask = np.eye(J), np.ones(M, dtype=bool)
    routes = (lambda **kw: basis.surface_matrix(grid, **kw), lambda **kw: basis.synthesize(grid, **kw), lambda **kw: basis.covariance_propagation(grid, C, **kw),
              lambda **kw: basis.basin_functionals(grid, mask, **kw), lambda **kw: basis.basin_averages(grid, mask, **kw),
              lambda **kw: basis.basin_covariance(grid, C, mask, **kw))
    for route in routes:
        with pytest.raises(ValueError, match='Unrecognized kernel'):
            route(kernel='no such kernel')
    for bad in (np.zeros(J + 1), np.zeros((3, J + 1)), np.zeros((2, 3, J)), np.float64(1.0)):
        with pytest.raises(ValueError, match=r'values must have shape \(24,\) or \(T, 24\)'):
            basis.synthesize(grid, values=bad)
        with pytest.raises(ValueError, match=r'values must have shape \(24,\) or \(T, 24\)'):
            basis.basin_averages(grid, mask, values=bad)
    for bad in (np.zeros((J, J + 1)), np.zeros((J + 1, J + 1)), np.zeros(J)):
        with pytest.raises(ValueError, match=r'covariance matrix must have shape \(24, 24\)'):
            basis.covariance_propagation(grid, bad)
        with pytest.raises(ValueError, match=r'covariance matrix must have shape \(24, 24\)'):
            basis.basin_covariance(grid, bad, mask)
    for block_points in (0, -5):
        with pytest.raises(ValueError, match='block_points must be positive'):
            basis.synthesize(grid, block_points=block_points)
        with pytest.raises(ValueError, match='block_points must be positive'):
            basis.covariance_propagation(grid, C, block_points=block_points)
    for route in (lambda m: basis.basin_functionals(grid, m), lambda m: basis.basin_averages(grid, m), lambda m: basis.basin_covariance(grid, C, m)):
        with pytest.raises(ValueError, match='masks must be boolean'):
            route(np.ones(M))
        with pytest.raises(ValueError, match='do not fit a grid of 46 points'):
            route(np.ones(M + 1, dtype=bool))
        with pytest.raises(ValueError, match='1 to 64 masks'):
            route(np.ones((65, M), dtype=bool))
    lon, lat = ri.case_nodes('b2_8')
    K = ri.shape_factors(ri.degree_factors(2, 8))
    K[3, 1] = np.nextafter(K[3, 1], 1.0)
    anisotropic = ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat), K, 2, 8, GM, R)
    for route in (lambda: anisotropic.surface_matrix(grid), lambda: anisotropic.synthesize(grid), lambda: anisotropic.covariance_propagation(grid, C),
                  lambda: anisotropic.basin_functionals(grid, mask), lambda: anisotropic.basin_averages(grid, mask),
                  lambda: anisotropic.basin_covariance(grid, C, mask)):
        with pytest.raises(ValueError, match='isotropic'):
            route()


def test_fixture_geometry_and_surface_factors(golden):
    data = golden('g31_rbf_surface')
    for tag, (min_degree, max_degree, count, _) in si.CASES.items():
        lon, lat, glon, glat = (data[name + tag] for name in ('lon_', 'lat_', 'glon_', 'glat_'))
        assert np.array_equal(lon, ri.case_nodes(tag)[0]) and np.array_equal(lat, ri.case_nodes(tag)[1])
        assert np.array_equal(glon, si.grid_points(tag)[0]) and np.array_equal(glat, si.grid_points(tag)[1]) and glon.shape == (si.SCATTERED + 6,)
        assert np.array_equal(data['k_' + tag], ri.degree_factors(min_degree, max_degree))
        t = si.unit_vectors(glon, glat)[si.SCATTERED:] @ ri.node_table(lon, lat)[:3, :3].T
        for j in range(3):
            assert abs(t[j, j] - 1.0) <= 2.3e-16 and abs(t[3 + j, j] + 1.0) <= 2.3e-16         # above a node, antipodal to it
        for kernel in si.KERNELS:
            S, sigma, kn = (data['{0}_{1}_{2}'.format(name, tag, kernel)] for name in ('S', 'sigma', 'kn'))
            assert S.shape == (si.SCATTERED + 6, count) and sigma.shape == (si.SCATTERED + 6,) and kn.shape == (si.SCATTERED + 6, max_degree + 1)
            assert np.all(np.isfinite(S)) and sigma.min() > 1e-4 * sigma.max()
            # the package's surface factors are the reference's: what engine.rbf_surface_tables uploads
            own = ga.gravityfield.surface_factors(ga.kernel.get_kernel(kernel), max_degree, glat, GM, R, si.A, si.F)[2]
            band = slice(min_degree, None)
            assert np.abs(own[:, band] - kn[:, band]).max() <= 4 * 2.0 ** -53 * np.abs(kn[:, band]).max()
    assert data['S_n96'].shape == (si.N96['points'], ri.N96['nodes']) and np.array_equal(data['glon_n96'], si.n96_points()[0])
    assert np.array_equal(data['k_n96'], ri.degree_factors(2, 96, flat=True)) and data['sigma_n96'].min() > 1e-4 * data['sigma_n96'].max()


def test_fixture_matches_the_restatement(golden):
    """The recorded figures are what this machine computes.  Recorded: S within 5.0e-15 of max|S| and sigma within 4.3e-15 of the largest
    in the bands up to degree 8, 5.2e-13 both at d/o 96; the GPU tests take 4 times these figures as their bounds."""
    data = golden('g31_rbf_surface')
    for tag, (min_degree, _, count, _) in si.CASES.items():
        nodes, k = ri.node_table(data['lon_' + tag], data['lat_' + tag]), data['k_' + tag]
        points = si.unit_vectors(data['glon_' + tag], data['glat_' + tag])
        C = si.covariance(count, si.COVARIANCE_SEED[tag])
        for i, kernel in enumerate(si.KERNELS):
            S_ref, sigma_ref = data['S_{0}_{1}'.format(tag, kernel)], data['sigma_{0}_{1}'.format(tag, kernel)]
            S = si.surface(nodes, k, min_degree, points, data['kn_{0}_{1}'.format(tag, kernel)])
            S_err, sigma_err = np.abs(S - S_ref).max() / np.abs(S_ref).max(), np.abs(si.sigmas(S, C) - sigma_ref).max() / sigma_ref.max()
            print('{0} {1}: restatement S {2:.2e}, sigma {3:.2e}'.format(tag, kernel, S_err, sigma_err))
            assert S_err <= 2 * data['S_err_' + tag][i] and sigma_err <= 2 * data['sigma_err_' + tag][i]
        assert np.all(data['S_err_' + tag] <= 1e-14) and np.all(data['sigma_err_' + tag] <= 1e-14)
    nodes, points = ri.node_table(data['lon_n96'], data['lat_n96']), si.unit_vectors(data['glon_n96'], data['glat_n96'])
    S = si.surface(nodes, data['k_n96'], 2, points, data['kn_n96'])
    S_err = np.abs(S - data['S_n96']).max() / np.abs(data['S_n96']).max()
    sigma_err = np.abs(si.sigmas(S, si.covariance(ri.N96['nodes'], si.COVARIANCE_SEED['n96'])) - data['sigma_n96']).max() / data['sigma_n96'].max()
    print('n96: restatement S {0:.2e}, sigma {1:.2e}'.format(S_err, sigma_err))
    assert S_err <= 2 * float(data['S_err_n96']) <= 2e-12 and sigma_err <= 2 * float(data['sigma_err_n96']) <= 2e-12


def test_restated_column_dots_is_a_sum_of_products():
    """rbf_surface_inputs.column_dots against the exact sum: within rows 2^-53 sum|x y|, the bound the GPU test takes"""
    import math
    rng = np.random.default_rng(3131)
    for rows in (1, 7, 8, 9, 65):
        X, Y = rng.standard_normal((rows, 5)), rng.standard_normal((rows, 5))
        exact = np.array([math.fsum(float(x) * float(y) for x, y in zip(X[:, c], Y[:, c])) for c in range(5)])
        assert np.all(np.abs(si.column_dots(X, Y) - exact) <= rows * 2.0 ** -53 * np.abs(X * Y).sum(axis=0))
