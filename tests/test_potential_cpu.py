"""
CPU checks of the gravitational potential at points, of its two design matrices and of NormalEquations.from_potentials /
from_potential_differences: the four C entry points reject bad arguments before any HIP call, the Python functions reject bad shapes,
pair counts, weights and observations before anything reaches the device, and the fixture g28_potential.npz is consistent with itself
and with the float64 NumPy restatement of the kernel's formulas.
"""
import ctypes
import inspect

import numpy as np
import pytest

import design_inputs as di
import grates_amd as ga
import potential_inputs as pi

TOL = 5e-14          # of pot_scale = max|A_pot| over both satellites (design entries) and of max|V| (forward values)
TOL_AX = 1e-13       # of max|V|: design matrix times coefficients against the forward functional


def _error(lib):
    return lib.shg_last_error().decode()


def _design_calls(lib):
    """the two design entry points behind one signature (N, min_degree, positions, M, weights, GM, R, At, ldt)"""
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    return (('shg_potential_design', lambda N, nmin, x, M, w, GM, R, At, ldt: lib.shg_potential_design(N, nmin, x, M, w, GM, R, At, ldt, None)),
            ('shg_potential_difference_design',
             lambda N, nmin, x, M, w, GM, R, At, ldt: lib.shg_potential_difference_design(N, nmin, x, dummy if x else None, M, w, GM, R, At, ldt, None)))


def test_design_entry_points_reject_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)
    GM, R = pi.GM, pi.R
    for name, call in _design_calls(lib):
        for N, nmin, M in ((-1, 0, 10), (4, -1, 10), (4, 0, -1)):
            assert call(N, nmin, dummy, M, None, GM, R, dummy, max(M, 0)) == -1
            assert name + ': negative size' in _error(lib)
        assert call(4, 5, dummy, 10, None, GM, R, dummy, 10) == -1
        assert 'min_degree 5 above N 4' in _error(lib)
        for N in (40000, 32768):
            assert call(N, 0, dummy, 10, None, GM, R, dummy, 10) == -1
            assert 'N {0} is too large'.format(N) in _error(lib)
        for gm, r in ((float('nan'), R), (float('inf'), R), (GM, 0.0), (GM, -R), (GM, float('inf')), (GM, float('nan'))):
            assert call(4, 0, dummy, 10, None, gm, r, dummy, 10) == -1
            assert 'GM and R must be finite and R positive' in _error(lib)
        assert call(4, 0, dummy, 10, None, GM, R, dummy, 9) == -1
        assert 'ldt 9 below M 10' in _error(lib)
        for x, At in ((None, dummy), (dummy, None)):
            for weights in (None, dummy):
                assert call(4, 0, x, 10, weights, GM, R, At, 10) == -1
                assert name + ': NULL pointer' in _error(lib)
        assert call(2000, 0, dummy, 1 << 20, None, GM, R, dummy, 1 << 20) == -1                  # 4e6 rows x 2^20 points
        assert 'is too large' in _error(lib)
        # nothing to do: no pointer is looked at and no HIP call is made
        assert call(4, 2, None, 0, None, GM, R, None, 0) == 0
        assert call(4, 2, None, 0, dummy, GM, R, None, 5) == 0
    assert lib.shg_potential_difference_design(4, 0, dummy, None, 10, None, GM, R, dummy, 10, None) == -1
    assert 'shg_potential_difference_design: NULL pointer' in _error(lib)
    with pytest.raises(_lib.ShgError, match='min_degree 3 above N 2'):
        _lib.call('shg_potential_design', 2, 3, dummy, 10, None, GM, R, dummy, 10, None)


def test_forward_entry_points_reject_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)
    GM, R = pi.GM, pi.R
    calls = (('shg_potential_points', lambda N, x, M, layout, c, B, gm, r, V: lib.shg_potential_points(N, x, M, layout, c, B, gm, r, V, None)),
             ('shg_potential_points_om', lambda N, x, M, layout, c, B, gm, r, V: lib.shg_potential_points_om(N, x, M, layout, c, B, B, gm, r, V, None)))
    for name, call in calls:
        for N, M, B in ((-1, 10, 1), (4, -1, 1), (4, 10, -1)):
            assert call(N, dummy, M, 0, dummy, B, GM, R, dummy) == -1
            assert name + ': negative size' in _error(lib)
        for layout in (-1, 2):
            assert call(4, dummy, 10, layout, dummy, 1, GM, R, dummy) == -1
            assert 'expected 0 (shared points) or 1 (points per epoch)' in _error(lib)
        for gm, r in ((float('nan'), R), (float('inf'), R), (GM, 0.0), (GM, -R), (GM, float('nan'))):
            assert call(4, dummy, 10, 0, dummy, 1, gm, r, dummy) == -1
            assert 'GM and R must be finite and R positive' in _error(lib)
        for x, c, V in ((None, dummy, dummy), (dummy, None, dummy), (dummy, dummy, None)):
            assert call(4, x, 10, 0, c, 1, GM, R, V) == -1
            assert name + ': NULL pointer' in _error(lib)
        assert call(4, dummy, 1 << 30, 0, dummy, 1 << 11, GM, R, dummy) == -1
        assert 'is too large' in _error(lib)
        assert call(4, None, 0, 0, None, 3, GM, R, None) == 0                                    # nothing to do
        assert call(4, None, 10, 1, None, 0, GM, R, None) == 0
    assert lib.shg_potential_points_om(4, dummy, 10, 0, dummy, 3, 2, GM, R, dummy, None) == -1
    assert 'shg_potential_points_om: Bpad 2 below B 3' in _error(lib)


def test_signatures():
    def names(function):
        return list(inspect.signature(function).parameters)
    assert names(ga.engine.potential_points) == ['max_degree', 'xyz', 'coefficients', 'GM', 'R']
    assert names(ga.engine.potential_design) == ['max_degree', 'xyz', 'GM', 'R', 'min_degree', 'weights']
    assert names(ga.engine.potential_difference_design) == ['max_degree', 'xyz_a', 'xyz_b', 'GM', 'R', 'min_degree', 'weights']
    assert names(ga.gravityfield.potential_design_matrix) == ['xyz', 'min_degree', 'max_degree', 'GM', 'R', 'weights', 'as_tensor']
    assert names(ga.gravityfield.potential_difference_design_matrix) == ['xyz_a', 'xyz_b', 'min_degree', 'max_degree', 'GM', 'R', 'weights', 'as_tensor']
    tail = ['min_degree', 'max_degree', 'GM', 'R', 'weights', 'block_points']
    for owner in (ga.lstsq.NormalEquations, ga.lstsq.ColouredNoise, ga.lstsq.ArcParameters):
        skip = 0 if owner is ga.lstsq.NormalEquations else 1                            # self of the bound models
        assert names(owner.from_potentials)[skip:] == ['xyz', 'potentials'] + tail
        assert names(owner.from_potential_differences)[skip:] == ['xyz_a', 'xyz_b', 'differences'] + tail
    assert names(ga.lstsq.PostFit.of_potentials) == ['solution', 'xyz', 'potentials'] + tail + ['model', 'vectors']
    assert names(ga.lstsq.PostFit.of_potential_differences) == ['solution', 'xyz_a', 'xyz_b', 'differences'] + tail + ['model', 'vectors']
    for cls in (ga.gravityfield.PotentialCoefficients, ga.gravityfield.TimeSeries):
        assert names(cls.gravitational_potential) == ['self', 'xyz', 'as_tensor']
        assert names(cls.potential_difference) == ['self', 'xyz_a', 'xyz_b', 'as_tensor']
    reference = inspect.signature(ga.gravityfield.acceleration_design_matrix).parameters
    for function in (ga.gravityfield.potential_design_matrix, ga.gravityfield.potential_difference_design_matrix, ga.lstsq.NormalEquations.from_potentials,
                     ga.lstsq.NormalEquations.from_potential_differences, ga.lstsq.PostFit.of_potentials):
        for name in ('GM', 'R'):
            assert inspect.signature(function).parameters[name].default == reference[name].default
    from grates_amd import _lib
    for name in ('shg_potential_points', 'shg_potential_points_om', 'shg_potential_design', 'shg_potential_difference_design'):
        assert name in _lib.PROTOTYPES


BAD_SHAPES = ((5,), (5, 2), (5, 4), (2, 5, 3))


def _field():
    gf = ga.gravityfield.PotentialCoefficients(pi.GM, pi.R)
    gf.anm = np.zeros((5, 5))
    return gf


def test_python_checks_of_points():
    xyz = pi.positions()[0][:5]
    routes = (lambda x, **kw: ga.gravityfield.potential_design_matrix(x, 0, 4, **kw),
              lambda x, **kw: ga.engine.potential_design(4, x, pi.GM, pi.R, **kw),
              lambda x, **kw: ga.lstsq.NormalEquations.from_potentials(x, np.ones(x.shape[0]), 0, 4, **kw),
              lambda x, **kw: ga.lstsq.PostFit.of_potentials(np.zeros(25), x, np.ones(x.shape[0]), 0, 4, **kw))
    for shape in BAD_SHAPES:
        for route in routes:
            with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
                route(np.zeros(shape))
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
            _field().gravitational_potential(np.zeros(shape))
    for route in routes:
        for shape in ((4,), (5, 3), (5, 1), (3, 5), ()):
            with pytest.raises(ValueError, match=r'weights must have shape \(5,\)'):
                route(xyz, weights=np.ones(shape))
        for bad in (-1.0, np.nan, np.inf):
            w = np.ones(5)
            w[2] = bad
            with pytest.raises(ValueError, match='weights must be finite and not negative'):
                route(xyz, weights=w)
    design, build = ga.gravityfield.potential_design_matrix, ga.lstsq.NormalEquations.from_potentials
    with pytest.raises(ValueError, match='min_degree 5 must lie between 0 and max_degree 4'):
        design(xyz, 5, 4)
    with pytest.raises(ValueError, match='min_degree -1'):
        design(xyz, -1, 4)
    with pytest.raises(ValueError, match='min_degree 5 must lie between 0 and max_degree 4'):
        build(xyz, np.ones(5), 5, 4)
    for shape in ((5, 1), (5, 3), ()):
        with pytest.raises(ValueError, match=r'potentials must have shape \(M,\)'):
            build(xyz, np.ones(shape), 0, 4)
    with pytest.raises(ValueError, match='5 positions but 6 potentials'):
        build(xyz, np.ones(6), 0, 4)
    for block_points in (0, -256):
        with pytest.raises(ValueError, match='block_points must be positive'):
            build(xyz, np.ones(5), 0, 4, block_points=block_points)
    with pytest.raises(ValueError, match=r'solution must have shape \(25,\)'):
        ga.lstsq.PostFit.of_potentials(np.zeros(24), xyz, np.ones(5), 0, 4)
    bound = ga.lstsq.ArcParameters(ga.lstsq.arc_basis([0, 3], 5, degree=0), [0, 3])
    with pytest.raises(ValueError, match=r'potentials must have shape \(M,\)'):
        bound.from_potentials(xyz, np.ones((5, 1)), 0, 4)
    with pytest.raises(ValueError, match=r'the arc basis must have shape \(4, u\)'):
        bound.from_potentials(xyz[:4], np.ones(4), 0, 4)


def test_python_checks_of_pairs():
    a, b = (x[:5] for x in pi.pairs())
    routes = (lambda a, b, **kw: ga.gravityfield.potential_difference_design_matrix(a, b, 0, 4, **kw),
              lambda a, b, **kw: ga.engine.potential_difference_design(4, a, b, pi.GM, pi.R, **kw),
              lambda a, b, **kw: ga.lstsq.NormalEquations.from_potential_differences(a, b, np.ones(a.shape[0]), 0, 4, **kw),
              lambda a, b, **kw: ga.lstsq.PostFit.of_potential_differences(np.zeros(25), a, b, np.ones(a.shape[0]), 0, 4, **kw))
    forward = (lambda a, b: _field().potential_difference(a, b),)
    for shape in BAD_SHAPES:
        for route in routes + forward:
            with pytest.raises(ValueError, match=r'positions of the first satellite must have shape \(M, 3\)'):
                route(np.zeros(shape), b)
            with pytest.raises(ValueError, match=r'positions of the second satellite must have shape \(M, 3\)'):
                route(a, np.zeros(shape))
    for route in routes + forward:
        with pytest.raises(ValueError, match='5 positions of the first satellite but 6 of the second'):
            route(a, pi.pairs()[1][:6])
    for route in routes:
        for shape in ((4,), (5, 3), (5, 1), ()):
            with pytest.raises(ValueError, match=r'weights must have shape \(5,\)'):
                route(a, b, weights=np.ones(shape))
        w = np.ones(5)
        w[1] = -0.5
        with pytest.raises(ValueError, match='weights must be finite and not negative'):
            route(a, b, weights=w)
    build = ga.lstsq.NormalEquations.from_potential_differences
    for shape in ((5, 1), (5, 3), ()):
        with pytest.raises(ValueError, match=r'differences must have shape \(M,\)'):
            build(a, b, np.ones(shape), 0, 4)
    with pytest.raises(ValueError, match='5 pairs but 6 differences'):
        build(a, b, np.ones(6), 0, 4)
    with pytest.raises(ValueError, match='min_degree 5 must lie between 0 and max_degree 4'):
        build(a, b, np.ones(5), 5, 4)


def test_time_series_checks_positions_before_the_device():
    fields = [ga.gravityfield.PotentialCoefficients(pi.GM, pi.R, 4) for _ in range(3)]
    for epoch, field in enumerate(fields):
        field.epoch = epoch
    series = ga.gravityfield.TimeSeries(fields)
    a, b = (x[:5] for x in pi.pairs())
    for bad in (np.zeros((2, 5, 3)), np.zeros((5, 2)), np.zeros(5)):
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\) or \(3, M, 3\)'):
            series.gravitational_potential(bad)
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\) or \(3, M, 3\)'):
            series.potential_difference(bad, bad)
    with pytest.raises(ValueError, match='must have the same shape'):
        series.potential_difference(a, np.stack((b, b, b)))
    with pytest.raises(ValueError, match='must have the same shape'):
        series.potential_difference(a, b[:4])


def test_fixture_geometry(golden):
    data = golden('g28_potential')
    xyz, a, b = data['xyz'], data['xyz_a'], data['xyz_b']
    assert xyz.shape == a.shape == b.shape == (20, 3)
    assert np.array_equal(xyz, pi.positions()[0]) and np.array_equal(a, xyz) and np.array_equal(b, pi.pairs()[1])
    sep = np.sqrt(np.sum((b - a) ** 2, axis=1))
    assert np.array_equal(sep == 0.0, pi.separations() == 0.0) and np.count_nonzero(sep == 0.0) == 2
    assert np.array_equal(b[sep == 0.0], a[sep == 0.0])
    assert np.count_nonzero(np.abs(sep - 1e3) < 1e-6) == 2 and np.count_nonzero(np.abs(sep - 1.0) < 1e-8) == 2
    assert np.count_nonzero(np.abs(sep - 220e3) < 1e-6) == 14
    r = pi.radius_of(xyz)
    assert np.count_nonzero((xyz[:, 0] == 0) & (xyz[:, 1] == 0)) >= 4 and np.count_nonzero(r < pi.R) >= 2      # the axis; below R
    heights = pi.radius_of(pi.loop_positions()[0]) - 6378137.0
    assert heights.min() > 349e3 and heights.max() < 551e3 and np.unique(np.round(heights)).size == 8          # eight shells
    assert np.array_equal(data['xyz60'], pi.v60_positions()[0]) and data['V60'].shape == (413,)
    assert pi.loop_arcs().size == 12 and np.array_equal(pi.arc_indicator().sum(axis=0), np.full(12, 50.0))
    assert np.array_equal(pi.arc_indicator(), np.repeat(np.eye(12), 50, axis=0))


def test_fixture_min_degree_is_a_column_slice(golden):
    data = golden('g28_potential')
    zero = pi.separations() == 0.0
    for N in pi.DEGREES:
        for kind in ('pot', 'dif'):
            A, A2 = data['A_{0}{1}'.format(kind, N)], data['A_{0}{1}_min2'.format(kind, N)]
            assert A.shape == (20, (N + 1) ** 2) and np.all(np.isfinite(A))
            assert np.array_equal(A2, A[:, 4:])
        assert np.all(data['A_dif{0}'.format(N)][zero] == 0.0) and np.all(np.abs(data['A_dif{0}'.format(N)][~zero]).max(axis=1) > 0)
        assert float(data['pot_scale{0}'.format(N)]) >= np.abs(data['A_pot{0}'.format(N)]).max() > 0


def test_fixture_matches_the_restatement(golden):
    """the recorded scalars are what this machine computes; the bounds on the GPU stay at the project's 5e-14 and 1e-13 because the
    restatement is within a quarter of them (recorded: 1.2e-15 of max|A_pot|, 1.9e-15 and 1.2e-15 of max|V|)"""
    data = golden('g28_potential')
    a, b = data['xyz_a'], data['xyz_b']
    far = pi.separations() > 100e3
    worst = 0.0
    for N in pi.DEGREES:
        scale = float(data['pot_scale{0}'.format(N)])
        for kind, A in (('pot', pi.restatement(a, 0, N)), ('dif', pi.difference_restatement(a, b, 0, N))):
            ref = data['A_{0}{1}'.format(kind, N)]
            err = np.abs(A - ref).max() / scale
            print('d/o {0} {1}: restatement {2:.2e} of max|A_pot|{3}'.format(
                N, kind, err, '' if kind == 'pot' else ', {0:.2e} of max|A_dif| at 220 km'.format(np.abs(A - ref)[far].max() / np.abs(ref[far]).max())))
            assert err <= TOL
            worst = max(worst, err)
        assert np.array_equal(pi.restatement(a, 2, N), pi.restatement(a, 0, N)[:, 4:])
        assert np.array_equal(pi.difference_restatement(a, b, 2, N), pi.difference_restatement(a, b, 0, N)[:, 4:])
        assert np.array_equal(pi.difference_restatement(b, a, 0, N), -pi.difference_restatement(a, b, 0, N))
    assert worst <= 2 * float(data['restatement_err']) and float(data['restatement_err']) <= TOL / 4
    forward_err = np.abs(pi.forward(data['xyz60'], pi.v60_field()) - data['V60']).max() / float(data['V60_scale'])
    print('forward restatement: {0:.2e} of max|V|'.format(forward_err))
    assert forward_err <= 2 * float(data['forward_err']) and float(data['forward_err']) <= TOL / 4
    assert float(data['ax_err']) <= TOL_AX / 4
    assert data['host_rel_err'].shape == data['loop_cond'].shape == (3,)
    assert np.all(data['host_rel_err'] <= 1e-8) and np.all(data['loop_cond'] <= 1e4)


def test_fixture_times_coefficients_is_v60(golden):
    """A @ x = V60 of the reference with A the restatement at d/o 60 (the fixture does not hold a 413 x 3721 matrix)"""
    data = golden('g28_potential')
    N = pi.V60[0]
    xyz, anm = data['xyz60'], pi.v60_field()
    x = di.ravel(anm, 0, N)
    err = np.abs(pi.restatement(xyz, 0, N) @ x - data['V60']).max() / float(data['V60_scale'])
    print('restatement @ x against V60: {0:.2e} of max|V|'.format(err))
    assert err <= TOL_AX
    x2 = di.ravel(anm, 2, N)                                                            # the field has nothing below degree 2
    assert np.abs(pi.restatement(xyz, 2, N) @ x2 - data['V60']).max() <= TOL_AX * float(data['V60_scale'])
    assert np.array_equal(x2, ga.utilities.ravel_coefficients(anm, 2, N))
