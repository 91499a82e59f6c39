"""
CPU checks of the line-of-sight design matrix and of NormalEquations.from_line_of_sight: the C entry point rejects bad arguments
before any HIP call, the Python functions reject bad shapes, directions, coincident pairs, weights and degrees before anything
reaches the device, and the fixture g26_line_of_sight.npz is consistent with itself.
"""
import ctypes
import inspect

import numpy as np
import pytest

import design_inputs as di
import grates_amd as ga
import los_inputs as li

TOL = 5e-14          # of acc_scale = max|A_acc| over both satellites: the bound of the acceleration design matrix


def _error(lib):
    return lib.shg_last_error().decode()


def test_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    GM, R = li.GM, li.R
    call = lib.shg_los_design
    for N, nmin, M in ((-1, 0, 10), (4, -1, 10), (4, 0, -1)):
        assert call(N, nmin, dummy, dummy, None, M, None, GM, R, dummy, max(M, 0), None) == -1
        assert 'shg_los_design: negative size' in _error(lib)
    assert call(4, 5, dummy, dummy, None, 10, None, GM, R, dummy, 10, None) == -1
    assert 'min_degree 5 above N 4' in _error(lib)
    assert call(40000, 0, dummy, dummy, None, 10, None, GM, R, dummy, 10, None) == -1
    assert 'N 40000 is too large' in _error(lib)
    assert call(32767, 0, dummy, dummy, None, 10, None, GM, R, dummy, 10, None) == -1
    assert 'N 32767 is too large' in _error(lib)
    for gm, r in ((float('nan'), R), (float('inf'), R), (GM, 0.0), (GM, -R), (GM, float('inf')), (GM, float('nan'))):
        assert call(4, 0, dummy, dummy, None, 10, None, gm, r, dummy, 10, None) == -1
        assert 'GM and R must be finite and R positive' in _error(lib)
    assert call(4, 0, dummy, dummy, None, 10, None, GM, R, dummy, 9, None) == -1
    assert 'ldt 9 below M 10' in _error(lib)
    for a, b, At in ((None, dummy, dummy), (dummy, None, dummy), (dummy, dummy, None)):
        for directions, weights in ((None, None), (dummy, dummy)):
            assert call(4, 0, a, b, directions, 10, weights, GM, R, At, 10, None) == -1
            assert 'shg_los_design: NULL pointer' in _error(lib)
    assert call(2000, 0, dummy, dummy, None, 1 << 20, None, GM, R, dummy, 1 << 20, None) == -1       # 4e6 rows x 2^20 pairs
    assert 'is too large' in _error(lib)
    assert call(1023, 0, dummy, dummy, None, 10, None, GM, R, dummy, (1 << 20) + 1, None) == -1      # 2^20 rows x (2^20 + 1)
    assert 'is too large' in _error(lib)
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(4, 2, None, None, None, 0, None, GM, R, None, 0, None) == 0
    assert call(4, 2, None, None, dummy, 0, dummy, GM, R, None, 5, None) == 0
    with pytest.raises(_lib.ShgError, match='min_degree 3 above N 2'):
        _lib.call('shg_los_design', 2, 3, dummy, dummy, None, 10, None, GM, R, dummy, 10, None)


def test_pass_size_follows_the_documented_rule():
    """both satellites' harmonics of degree N + 1 share 256 MB: half the points of the acceleration's pass, in whole workgroups"""
    for N, expected in ((96, 1536), (8, 152320), (60, 4096), (300, 256), (2000, 256)):
        packed = (N + 2) * (N + 3) // 2
        rule = max((256 << 20) // 8 // (4 * packed) // 256 * 256, 256)
        assert ga.engine.los_design_pass(N) == rule == expected
        acceleration = max((256 << 20) // 8 // (2 * packed) // 256 * 256, 256)
        assert rule <= max(acceleration // 2, 256) and (rule == 256 or 8 * 4 * packed * rule <= 256 << 20)
    for N in (-1, 32767):
        with pytest.raises(ValueError, match='out of range'):
            ga.engine.los_design_pass(N)


def test_signatures():
    def names(function):
        return list(inspect.signature(function).parameters)
    assert names(ga.engine.los_design) == ['max_degree', 'xyz_a', 'xyz_b', 'GM', 'R', 'min_degree', 'directions', 'weights']
    assert names(ga.gravityfield.line_of_sight_design_matrix) == ['xyz_a', 'xyz_b', 'min_degree', 'max_degree', 'GM', 'R', 'directions', 'weights',
                                                                  'as_tensor']
    assert names(ga.lstsq.NormalEquations.from_line_of_sight) == ['xyz_a', 'xyz_b', 'differences', 'min_degree', 'max_degree', 'GM', 'R',
                                                                  'directions', 'weights', 'block_points']
    for cls in (ga.gravityfield.PotentialCoefficients, ga.gravityfield.TimeSeries):
        assert names(cls.line_of_sight_acceleration) == ['self', 'xyz_a', 'xyz_b', 'directions', 'as_tensor']
    reference = inspect.signature(ga.gravityfield.acceleration_design_matrix).parameters
    for function in (ga.gravityfield.line_of_sight_design_matrix, ga.lstsq.NormalEquations.from_line_of_sight):
        for name in ('GM', 'R'):
            assert inspect.signature(function).parameters[name].default == reference[name].default


BAD_SHAPES = ((5,), (5, 2), (5, 4), (2, 5, 3))


def _all_routes(a, b, **kwargs):
    """the four callers that check pairs before anything reaches the device"""
    gf = ga.gravityfield.PotentialCoefficients(li.GM, li.R)
    gf.anm = np.zeros((5, 5))
    keys = {k: v for k, v in kwargs.items() if k == 'directions'}
    return (lambda: ga.gravityfield.line_of_sight_design_matrix(a, b, 0, 4, **kwargs),
            lambda: ga.engine.los_design(4, a, b, li.GM, li.R, **kwargs),
            lambda: ga.lstsq.NormalEquations.from_line_of_sight(a, b, np.ones(a.shape[0]), 0, 4, **kwargs),
            lambda: gf.line_of_sight_acceleration(a, b, **keys))


def test_python_checks_of_positions_and_degrees():
    a, b = (x[:5] for x in li.pairs())
    for shape in BAD_SHAPES:
        for route in _all_routes(np.zeros(shape), b):
            with pytest.raises(ValueError, match=r'positions of the first satellite must have shape \(M, 3\)'):
                route()
        for route in _all_routes(a, np.zeros(shape)):
            with pytest.raises(ValueError, match=r'positions of the second satellite must have shape \(M, 3\)'):
                route()
    for route in _all_routes(a, li.pairs()[1][:6]):
        with pytest.raises(ValueError, match='5 positions of the first satellite but 6 of the second'):
            route()
    design = ga.gravityfield.line_of_sight_design_matrix
    build = ga.lstsq.NormalEquations.from_line_of_sight
    with pytest.raises(ValueError, match='min_degree 5 must lie between 0 and max_degree 4'):
        design(a, b, 5, 4)
    with pytest.raises(ValueError, match='min_degree -1'):
        design(a, b, -1, 4)
    with pytest.raises(ValueError, match='min_degree 5 must lie between 0 and max_degree 4'):
        build(a, b, np.ones(5), 5, 4)
    for shape in ((5, 1), (5, 3), ()):
        with pytest.raises(ValueError, match=r'differences must have shape \(M,\)'):
            build(a, b, np.ones(shape), 0, 4)
    with pytest.raises(ValueError, match='5 pairs but 6 differences'):
        build(a, b, np.ones(6), 0, 4)
    with pytest.raises(ValueError, match='block_points must be positive'):
        build(a, b, np.ones(5), 0, 4, block_points=0)
    with pytest.raises(ValueError, match='block_points must be positive'):
        build(a, b, np.ones(5), 0, 4, block_points=-256)


def test_python_checks_of_directions_and_coincident_pairs():
    a, b = (x[:5] for x in li.pairs())
    e = li.directions()[:5]
    ga.engine.check_directions(e, 5)                                                     # seeded unit vectors pass
    ga.engine.check_directions(e * (1.0 + 5e-13), 5)                                     # within FRAME_TOLERANCE
    ga.engine.check_directions(np.zeros((0, 3)), 0)
    assert ga.engine.FRAME_TOLERANCE == 1e-12
    for shape in ((5,), (4, 3), (5, 2), (5, 3, 1), (3, 5)):
        for route in _all_routes(a, b, directions=np.ones(shape)):
            with pytest.raises(ValueError, match=r'directions must have shape \(5, 3\)'):
                route()
    for factor in (1.0 + 1e-9, 0.5, 0.0, np.nan, np.inf):
        bad = e.copy()
        bad[3] = bad[3] * factor
        for route in _all_routes(a, b, directions=bad):
            with pytest.raises(ValueError, match='directions must be finite unit vectors'):
                route()
    bad = e.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match='directions must be finite unit vectors'):
        ga.engine.check_directions(bad, 5)
    same = b.copy()
    same[2] = a[2]
    same[4] = a[4]
    for route in _all_routes(a, same):
        with pytest.raises(ValueError, match='2 pairs have both satellites at the same position'):
            route()
    ga.engine.check_pairs_apart(a, b)
    ga.engine.check_pairs_apart(a, a + np.array([0.0, 0.0, 1e-3]))                        # 1 mm apart is apart


def test_python_checks_of_weights():
    a, b = (x[:5] for x in li.pairs())
    design = ga.gravityfield.line_of_sight_design_matrix
    build = ga.lstsq.NormalEquations.from_line_of_sight
    for shape in ((4,), (5, 3), (5, 2), (3, 5), ()):
        with pytest.raises(ValueError, match=r'weights must have shape \(5,\)'):
            design(a, b, 0, 4, weights=np.ones(shape))
        with pytest.raises(ValueError, match=r'weights must have shape \(5,\)'):
            build(a, b, np.ones(5), 0, 4, weights=np.ones(shape))
    with pytest.raises(ValueError, match=r'weights must have shape \(5,\)'):
        design(a, b, 0, 4, weights=np.ones((5, 1)))
    for bad in (-1.0, np.nan, np.inf):
        w = np.ones(5)
        w[2] = bad
        with pytest.raises(ValueError, match='weights must be finite and not negative'):
            design(a, b, 0, 4, weights=w)
        with pytest.raises(ValueError, match='weights must be finite and not negative'):
            build(a, b, np.ones(5), 0, 4, weights=w)


def test_time_series_checks_positions_before_the_device():
    fields = [ga.gravityfield.PotentialCoefficients(li.GM, li.R, 4) for _ in range(3)]
    for epoch, field in enumerate(fields):
        field.epoch = epoch
    series = ga.gravityfield.TimeSeries(fields)
    a, b = (x[:5] for x in li.pairs())
    with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\) or \(3, M, 3\)'):
        series.line_of_sight_acceleration(np.zeros((2, 5, 3)), np.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match='must have the same shape'):
        series.line_of_sight_acceleration(a, np.stack((b, b, b)))
    with pytest.raises(ValueError, match=r'directions must have shape \(3, 5, 3\)'):
        series.line_of_sight_acceleration(np.stack((a, a, a)), np.stack((b, b, b)), directions=li.directions()[:5])
    with pytest.raises(ValueError, match='directions must be finite unit vectors'):
        series.line_of_sight_acceleration(a, b, directions=2.0 * li.directions()[:5])
    same = b.copy()
    same[1] = a[1]
    with pytest.raises(ValueError, match='3 pairs have both satellites at the same position'):
        series.line_of_sight_acceleration(np.stack((a, a, a)), np.stack((same, same, same)))


def test_default_block_is_a_multiple_of_256_within_the_budget():
    """the rule of from_line_of_sight's default block_points, restated: one row per pair, so three times the acceleration's block"""
    budget = ga.lstsq.NormalEquations.DESIGN_BLOCK_BYTES
    assert budget == 256 << 20
    for N, nmin, expected in ((96, 0, 3328), (96, 2, 3328), (8, 2, 435712), (2000, 0, 256)):
        P = di.parameter_count(nmin, N)
        block = max(budget // (8 * P) // 256 * 256, 256)
        assert block == expected and block % 256 == 0
        assert block == 256 or (8 * P * block <= budget < 8 * P * (block + 256))


def test_fixture_pairs(golden):
    data = golden('g26_line_of_sight')
    a, b, e = data['xyz_a'], data['xyz_b'], data['directions']
    pairs = li.pairs()
    assert a.shape == b.shape == e.shape == (20, 3)
    assert np.array_equal(a, di.positions()) and np.array_equal(a, pairs[0]) and np.array_equal(b, pairs[1]) and np.array_equal(e, li.directions())
    ga.engine.check_directions(e, 20)
    ga.engine.check_pairs_apart(a, b)
    sep = np.sqrt(np.sum((b - a) ** 2, axis=1))
    assert np.count_nonzero(np.abs(sep - 1e3) < 1e-6) >= 2 and np.count_nonzero(np.abs(sep - 1.0) < 1e-8) >= 2
    assert np.count_nonzero(np.abs(sep - 220e3) < 1e-6) >= 14
    assert np.any((b[:, 0] == 0) & (b[:, 1] == 0) & ((a[:, 0] != 0) | (a[:, 1] != 0)))        # b on the exact pole, a off it
    lon_a, lon_b = np.arctan2(a[:, 1], a[:, 0]), np.arctan2(b[:, 1], b[:, 0])
    assert np.count_nonzero(np.abs(lon_a - lon_b) > 6.0) >= 2                                 # across the antimeridian, both ways
    for N in li.DEGREES:
        assert float(data['acc_scale{0}'.format(N)]) > 0


def test_fixture_min_degree_is_a_column_slice(golden):
    data = golden('g26_line_of_sight')
    for N in li.DEGREES:
        for tag in ('', '_dir'):
            A, A2 = data['A_los{0}{1}'.format(N, tag)], data['A_los{0}{1}_min2'.format(N, tag)]
            assert A.shape == (20, (N + 1) ** 2) and np.all(np.isfinite(A))
            assert np.array_equal(A2, A[:, 4:])
        assert not np.array_equal(data['A_los{0}'.format(N)], data['A_los{0}_dir'.format(N)])


def test_fixture_matches_the_restatement(golden):
    """the recorded scalars are what this machine computes; the bound on the GPU stays at the acceleration design's 5e-14 because the
    restatement is within a quarter of it"""
    data = golden('g26_line_of_sight')
    a, b, e = data['xyz_a'], data['xyz_b'], data['directions']
    worst = 0.0
    for N in li.DEGREES:
        scale = float(data['acc_scale{0}'.format(N)])
        for tag, lines in (('', None), ('_dir', e)):
            A = data['A_los{0}{1}'.format(N, tag)]
            err = np.abs(li.restatement(a, b, 0, N, lines) - A).max() / scale
            print('d/o {0}{1}: restatement {2:.2e} of max|A_acc|, {3:.2e} of max|A_los| at 220 km'.format(
                N, tag, err, err * scale / np.abs(A[li.separations() > 100e3]).max()))
            assert err <= TOL
            worst = max(worst, err)
            assert np.array_equal(li.restatement(a, b, 2, N, lines), li.restatement(a, b, 0, N, lines)[:, 4:])
    assert worst <= 2 * float(data['restatement_err']) and float(data['restatement_err']) <= TOL / 4
    assert float(data['ax_err']) <= 1e-13 / 4
    assert float(data['host_rel_err']) <= 1e-8 and float(data['loop_cond']) <= 1e4
    # the same rounding errors relative to the difference itself grow as the pair closes: why the bounds are fractions of acc_scale
    assert np.all(data['restatement_err_by_separation'] <= TOL / 4)


def test_fixture_times_coefficients_is_l60(golden):
    """A @ x = l60 of the reference: A is the restatement at d/o 60 (the fixture does not hold a 413 x 3721 matrix), within the A x
    bound of 1e-13 of max|g| over both satellites"""
    data = golden('g26_line_of_sight')
    a, b = li.l60_pairs()
    N = li.L60[1]
    assert data['l60'].shape == (a.shape[0],) == (413,)
    x = di.ravel(li.l60_field(), 0, N)
    err = np.abs(li.restatement(a, b, 0, N) @ x - data['l60']).max() / float(data['g60_scale'])
    print('restatement @ x against l60: {0:.2e} of max|g|'.format(err))
    assert err <= 1e-13
    x2 = di.ravel(li.l60_field(), 2, N)                                                # the field has nothing below degree 2
    assert np.abs(li.restatement(a, b, 2, N) @ x2 - data['l60']).max() <= 1e-13 * float(data['g60_scale'])
    assert np.array_equal(x2, ga.utilities.ravel_coefficients(li.l60_field(), 2, N))
