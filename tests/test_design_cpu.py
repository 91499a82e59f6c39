"""
CPU checks of the acceleration design matrix and of NormalEquations.from_accelerations: the C entry point rejects bad arguments
before any HIP call, the Python functions reject bad shapes, weights and degrees before anything reaches the device, and the
fixture g24_acceleration_design.npz is consistent with itself and with the host acceleration.
"""
import ctypes

import numpy as np
import pytest

import acceleration_inputs as ai
import design_inputs as di
import grates_amd as ga


def _error(lib):
    return lib.shg_last_error().decode()


def test_design_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    GM, R = di.GM, di.R
    call = lib.shg_acceleration_design
    for N, nmin, M in ((-1, 0, 10), (4, -1, 10), (4, 0, -1)):
        assert call(N, nmin, dummy, M, None, 0, GM, R, dummy, max(M, 0), None) == -1
        assert 'negative size' in _error(lib)
    assert call(4, 5, dummy, 10, None, 0, GM, R, dummy, 10, None) == -1
    assert 'min_degree 5 above N 4' in _error(lib)
    assert call(40000, 0, dummy, 10, None, 0, GM, R, dummy, 10, None) == -1
    assert 'N 40000 is too large' in _error(lib)
    for layout in (-1, 3):
        assert call(4, 0, dummy, 10, dummy, layout, GM, R, dummy, 10, None) == -1
        assert 'weight layout {0}, expected 0 (none), 1 (per point) or 2 (per component)'.format(layout) in _error(lib)
    for gm, r in ((float('nan'), R), (GM, 0.0), (GM, -R), (GM, float('inf'))):
        assert call(4, 0, dummy, 10, None, 0, gm, r, dummy, 10, None) == -1
        assert 'GM and R must be finite and R positive' in _error(lib)
    assert call(4, 0, dummy, 10, None, 0, GM, R, dummy, 9, None) == -1
    assert 'ldt 9 below M 10' in _error(lib)
    for xyz, w, layout, At in ((None, None, 0, dummy), (dummy, None, 0, None), (dummy, None, 1, dummy), (dummy, None, 2, dummy)):
        assert call(4, 0, xyz, 10, w, layout, GM, R, At, 10, None) == -1
        assert 'shg_acceleration_design: NULL pointer' in _error(lib)
    assert call(2000, 0, dummy, 1 << 20, None, 0, GM, R, dummy, 1 << 20, None) == -1        # 4e6 rows x 3 x 2^20 points
    assert 'is too large' in _error(lib)
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(4, 2, None, 0, None, 0, GM, R, None, 0, None) == 0
    assert call(4, 2, None, 0, None, 1, GM, R, None, 5, None) == 0
    with pytest.raises(_lib.ShgError, match='min_degree 3 above N 2'):
        _lib.call('shg_acceleration_design', 2, 3, dummy, 10, None, 0, GM, R, dummy, 10, None)


BAD_SHAPES = ((5,), (5, 2), (5, 4), (2, 5, 3))


def test_design_matrix_python_checks():
    design = ga.gravityfield.acceleration_design_matrix
    for shape in BAD_SHAPES:
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
            design(np.zeros(shape), 0, 4)
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
            ga.engine.acceleration_design(4, np.zeros(shape), di.GM, di.R)
    xyz = di.positions()[:5]
    with pytest.raises(ValueError, match='min_degree 5 must lie between 0 and max_degree 4'):
        design(xyz, 5, 4)
    with pytest.raises(ValueError, match='min_degree -1'):
        design(xyz, -1, 4)
    for shape in ((4,), (5, 2), (5, 3, 1), (3, 5), ()):
        with pytest.raises(ValueError, match=r'weights must have shape \(5,\) or \(5, 3\)'):
            design(xyz, 0, 4, weights=np.ones(shape))
    for bad in (-1.0, np.nan, np.inf):
        for shape in ((5,), (5, 3)):
            w = np.ones(shape)
            w[2] = bad
            with pytest.raises(ValueError, match='weights must be finite and not negative'):
                design(xyz, 0, 4, weights=w)


def test_from_accelerations_python_checks():
    build = ga.lstsq.NormalEquations.from_accelerations
    good = np.ones((5, 3))
    for shape in BAD_SHAPES:
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
            build(np.zeros(shape), good, 0, 4)
        with pytest.raises(ValueError, match=r'accelerations must have shape \(M, 3\)'):
            build(good, np.zeros(shape), 0, 4)
    with pytest.raises(ValueError, match='5 positions but 6 accelerations'):
        build(good, np.ones((6, 3)), 0, 4)
    with pytest.raises(ValueError, match='min_degree 5 must lie between 0 and max_degree 4'):
        build(good, good, 5, 4)
    with pytest.raises(ValueError, match=r'weights must have shape \(5,\) or \(5, 3\)'):
        build(good, good, 0, 4, weights=np.ones(6))
    with pytest.raises(ValueError, match='weights must be finite and not negative'):
        build(good, good, 0, 4, weights=np.array([1.0, 1.0, -0.5, 1.0, 1.0]))
    with pytest.raises(ValueError, match='weights must be finite and not negative'):
        build(good, good, 0, 4, weights=np.full((5, 3), np.nan))
    with pytest.raises(ValueError, match='block_points must be positive'):
        build(good, good, 0, 4, block_points=0)


def test_default_block_is_a_multiple_of_256_within_the_budget():
    """the rule of from_accelerations' default block_points, restated: d/o 96 gives 1024 points, small systems a whole 256 MB"""
    budget = ga.lstsq.NormalEquations.DESIGN_BLOCK_BYTES
    assert budget == 256 << 20
    for N, nmin, expected in ((96, 0, 1024), (96, 2, 1024), (8, 2, 145152), (720, 0, 256)):
        P = di.parameter_count(nmin, N)
        block = max(budget // (24 * P) // 256 * 256, 256)
        assert block == expected and block % 256 == 0
        assert block == 256 or (24 * P * block <= budget < 24 * P * (block + 256))


def test_fixture_min_degree_is_a_column_slice(golden):
    data = golden('g24_acceleration_design')
    xyz = data['xyz']
    assert xyz.shape == (20, 3)
    for N in di.DEGREES:
        A, A2 = data['A{0}'.format(N)], data['A{0}_min2'.format(N)]
        assert A.shape == (60, (N + 1) ** 2) and np.all(np.isfinite(A))
        assert np.array_equal(A2, A[:, 4:])
    r = np.sqrt(np.sum(xyz ** 2, axis=1))
    assert np.any((xyz[:, 0] == 0) & (xyz[:, 1] == 0))                                  # exact poles
    assert np.any((xyz[:, 0] == 1e-3) & (xyz[:, 1] == 0))                               # 1 mm off the pole
    assert np.any((xyz[:, 0] < 0) & (xyz[:, 1] == 0) & np.signbit(xyz[:, 1]))           # antimeridian, y = -0
    assert np.any((xyz[:, 0] < 0) & (xyz[:, 1] == 0) & ~np.signbit(xyz[:, 1]))          # antimeridian, y = +0
    assert np.any(r < di.R) and np.any(r > di.R + 400e3)


def _host_acceleration(xyz):
    def acceleration(anm):
        gf = ga.gravityfield.PotentialCoefficients(di.GM, di.R)
        gf.anm = anm
        return gf.gravitational_acceleration(xyz)
    return acceleration


def test_fixture_times_coefficients_is_the_host_acceleration(golden):
    """A @ x of the fixture against the host acceleration (bitwise the reference's) of seeded fields, with and without min_degree"""
    data = golden('g24_acceleration_design')
    xyz = data['xyz']
    for N in di.DEGREES:
        anm = ai.coefficients(N, 'static', 2430 + N)
        g = _host_acceleration(xyz)(anm).ravel()
        assert np.abs(data['A{0}'.format(N)] @ di.ravel(anm, 0, N) - g).max() <= 1e-14 * np.abs(g).max()
        anm = ai.coefficients(N, 'anomaly', 2440 + N)                                  # nothing below degree 2
        g = _host_acceleration(xyz)(anm).ravel()
        assert np.abs(data['A{0}_min2'.format(N)] @ di.ravel(anm, 2, N) - g).max() <= 1e-14 * np.abs(g).max()
        assert np.array_equal(di.ravel(anm, 2, N), ga.utilities.ravel_coefficients(anm, 2, N))


def test_fixture_matches_the_restatement_and_unit_fields(golden):
    """the recorded scalars are what this machine computes: the NumPy restatement of the kernel's formulas and a sample of unit
    fields of the host acceleration against the stored A; the scalars leave the GPU tests their own bounds (a quarter of them)"""
    data = golden('g24_acceleration_design')
    xyz = data['xyz']
    worst = 0.0
    for N in di.DEGREES:
        A = data['A{0}'.format(N)]
        worst = max(worst, np.abs(di.restatement(xyz, 0, N) - A).max() / np.abs(A).max())
        assert np.array_equal(di.restatement(xyz, 2, N), di.restatement(xyz, 0, N)[:, 4:])
    assert worst <= 2 * float(data['restatement_err']) and float(data['restatement_err']) <= 5e-14 / 4
    assert float(data['ax_err']) <= 1e-13 / 4
    assert float(data['host_rel_err']) <= 1e-8 and float(data['loop_cond']) <= 1e4
    columns = di.degreewise(0, 8)
    for col in (0, 1, 2, 3, 4, 17, 80):
        n, m, sine = columns[col]
        assert np.array_equal(_host_acceleration(xyz)(di.unit_field(n, m, sine, 8)).ravel(), data['A8'][:, col]), (n, m, sine)
