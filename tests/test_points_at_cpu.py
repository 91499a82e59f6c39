"""
CPU checks of the point functionals of time-variable fields with every point at its own epoch: the six shg_*_points_at entry points
and the workspace limit reject bad arguments before any HIP call, the Python layers reject bad shapes, epochs and constituents before
anything reaches the device, the window and weight arithmetic of TimeSeries, Trend and Oscillation agrees with the fixture
g32_points_at.npz and with interpolate_to / evaluate_at of the package, and engine.points_at_plan builds the runs the C ABI takes.
"""
import ctypes
import datetime

import numpy as np
import pytest

import grates_amd as ga
import points_at_inputs as pi

STEMS = ('shg_acceleration_points_at', 'shg_potential_points_at', 'shg_gravitational_gradients_points_at')


def _error(lib):
    return lib.shg_last_error().decode()


def _ints(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


def _calls(lib):
    """the six entry points behind one signature (N, xyz, M, fields, B, Bpad, run_first, run_begin, runs, weights, W, GM, R, out); the
    reference layout has no Bpad"""
    out = []
    for stem in STEMS:
        out.append((stem, False, lambda N, x, M, c, B, Bpad, rf, rb, runs, w, W, GM, R, o, f=getattr(lib, stem):
                    f(N, x, M, c, B, rf, rb, runs, w, W, GM, R, o, None)))
        out.append((stem + '_om', True, lambda N, x, M, c, B, Bpad, rf, rb, runs, w, W, GM, R, o, f=getattr(lib, stem + '_om'):
                    f(N, x, M, c, B, Bpad, rf, rb, runs, w, W, GM, R, o, None)))
    return out


def test_entry_points_reject_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    GM, R = pi.GM, pi.R
    keep_first, first = _ints([0, 2])                               # (the arrays must outlive their addresses)
    keep_begin, begin = _ints([0, 4, 10])
    for name, om, call in _calls(lib):
        def good(N=4, x=dummy, M=10, c=dummy, B=4, Bpad=32, rf=first, rb=begin, runs=2, w=dummy, W=2, gm=GM, r=R, o=dummy):
            return call(N, x, M, c, B, Bpad, rf, rb, runs, w, W, gm, r, o)
        for kw in (dict(N=-1), dict(M=-1), dict(B=-1)):
            assert good(**kw) == -1
            assert name + ': negative size' in _error(lib)
        for W in (0, -1, 17):
            assert good(W=W, B=20) == -1
            assert 'window of {0} fields, expected 1 .. 16'.format(W) in _error(lib)
        assert good(B=2, W=3) == -1
        assert '2 fields, fewer than the window of 3' in _error(lib)
        assert good(runs=-1) == -1
        assert 'negative number of runs' in _error(lib)
        for gm, r in ((float('nan'), R), (float('inf'), R), (GM, 0.0), (GM, -R), (GM, float('inf')), (GM, float('nan'))):
            assert good(gm=gm, r=r) == -1
            assert 'GM and R must be finite and R positive' in _error(lib)
        if om:
            assert good(Bpad=3) == -1
            assert 'Bpad 3 below B 4' in _error(lib)
        for kw in (dict(x=None), dict(c=None), dict(rf=None), dict(rb=None), dict(w=None), dict(o=None)):
            assert good(**kw) == -1
            assert name + ': NULL pointer' in _error(lib)
        # the run tables
        for table, message in (([1, 4, 10], 'run_begin[0] is 1, not 0'), ([0, 4, 4], 'run_begin must increase strictly'),
                               ([0, 5, 4], 'run_begin must increase strictly'), ([0, 4, 11], 'run_begin must increase strictly'),
                               ([0, 4, 9], 'the runs end at point 9, not at M 10')):
            keep, rb = _ints(table)
            assert good(rb=rb) == -1
            assert message in _error(lib), table
        assert good(runs=0) == -1                                    # no run covers the 10 points
        assert 'the runs end at point 0, not at M 10' in _error(lib)
        for table in ([-1, 2], [0, 3], [3, 0]):
            keep, rf = _ints(table)
            assert good(rf=rf) == -1
            assert 'outside 0 .. B - W = 2' in _error(lib), table
        # nothing to do: no pointer is looked at and no HIP call is made
        assert call(4, None, 0, None, 4, 32, None, None, 0, None, 2, GM, R, None) == 0
        assert call(4, None, 0, None, 4, 32, None, None, 5, None, 2, GM, R, None) == 0
    # (the rule of at most 2^40 output values cannot fail while M is an int: 9 * 2^31 < 2^40)
    # the gradients' degree rule: one pass of the combined coefficients must be indexable by int
    for name, om, call in _calls(lib):
        if 'gradients' in name:
            assert call(10000, dummy, 10, dummy, 4, 32, first, begin, 2, dummy, 2, GM, R, dummy) == -1
            assert 'degree 10000 is too large' in _error(lib)
    with pytest.raises(_lib.ShgError, match='window of 0 fields'):
        _lib.call('shg_potential_points_at', 4, dummy, 10, dummy, 4, first, begin, 2, dummy, 0, GM, R, dummy, None)


def test_workspace_limit_is_checked_at_call_time():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)
    keep_first, first = _ints([0, 2])                               # (the arrays must outlive their addresses)
    keep_begin, begin = _ints([0, 4, 10])
    assert lib.shg_points_at_set_workspace_limit(-1) == -1
    assert 'negative limit -1' in _error(lib)
    with pytest.raises(_lib.ShgError, match='negative limit'):
        ga.engine.points_at_set_workspace_limit(-5)
    # one field of the acceleration at d/o 4 holds packed(5) * 6 = 126 doubles: a window of 2 needs 2016 bytes
    try:
        assert lib.shg_points_at_set_workspace_limit(2015) == 0
        for name, om, call in _calls(lib):
            if name.startswith('shg_acceleration'):
                assert call(4, dummy, 10, dummy, 4, 32, first, begin, 2, dummy, 2, pi.GM, pi.R, dummy) == -1
                assert 'the workspace limit of 2015 bytes is below one window of 2 fields (2016 bytes)' in _error(lib)
                assert call(4, None, 0, None, 4, 32, None, None, 0, None, 2, pi.GM, pi.R, None) == 0           # nothing to do comes first
    finally:
        assert lib.shg_points_at_set_workspace_limit(0) == 0


def test_points_at_plan():
    plan = ga.engine.points_at_plan
    order, first, begin = plan(np.array([0, 0, 0, 2, 2, 5]))
    assert order is None and first.dtype == np.int32 and begin.dtype == np.int32
    assert first.tolist() == [0, 2, 5] and begin.tolist() == [0, 3, 5, 6]
    order, first, begin = plan(np.array([3, 0, 3, 1, 0, 3]))
    assert order.tolist() == [1, 4, 3, 0, 2, 5]                     # stable: equal starts keep their order
    assert first.tolist() == [0, 1, 3] and begin.tolist() == [0, 2, 3, 6]
    order, first, begin = plan(np.array([7]))
    assert order is None and first.tolist() == [7] and begin.tolist() == [0, 1]
    order, first, begin = plan(np.zeros(0, dtype=np.int64))
    assert order is None and first.tolist() == [] and begin.tolist() == [0]
    # scatter: row i of the call's output belongs to point order[i]
    rng = np.random.default_rng(5)
    start = rng.integers(0, 9, 1000)
    order, first, begin = plan(start)
    assert np.all(np.diff(first) > 0) and begin[0] == 0 and begin[-1] == 1000 and np.all(np.diff(begin) > 0)
    expanded = np.repeat(first, np.diff(begin))
    back = np.empty(1000, dtype=np.int64)
    back[order] = expanded
    assert np.array_equal(back, start)


def test_engine_rejects_bad_arguments_before_the_device():
    xyz = pi.positions('model31')[:6]
    anm = pi.series_coefficients('model31')[:4]
    first = np.array([0, 0, 1, 1, 2, 2])
    weights = np.ones((6, 2))
    for function in (ga.engine.acceleration_points_at, ga.engine.potential_points_at, ga.engine.gravitational_gradients_points_at):
        def call(x=xyz, c=anm, f=first, w=weights, N=31, GM=pi.GM, R=pi.R):
            return function(N, x, c, f, w, GM, R)
        with pytest.raises(ValueError, match=r'must have shape \(M, 3\)'):
            call(x=xyz[:, :2])
        with pytest.raises(ValueError, match='coefficient batch must have shape'):
            call(N=30)
        with pytest.raises(ValueError, match='coefficient batch must have shape'):
            call(c=anm[0])
        with pytest.raises(ValueError, match='first must be an integer array'):
            call(f=first[:5])
        with pytest.raises(ValueError, match='first must be an integer array'):
            call(f=first.astype(float))
        with pytest.raises(ValueError, match=r'weights must have shape \(6, W\)'):
            call(w=weights[:5])
        with pytest.raises(ValueError, match=r'weights must have shape \(6, W\)'):
            call(w=np.ones((6, 0)))
        with pytest.raises(ValueError, match='a window of 5 fields, but only 4 fields'):
            call(w=np.ones((6, 5)))
        with pytest.raises(ValueError, match=r'first\[4\] is 3, outside 0 .. 2'):
            call(f=np.array([0, 0, 1, 1, 3, 4]))
        with pytest.raises(ValueError, match=r'first\[1\] is -1'):
            call(f=np.array([0, -1, 1, 1, 2, 2]))
        for bad in (np.nan, np.inf):
            w = weights.copy()
            w[3, 1] = bad
            with pytest.raises(ValueError, match='weights must be finite'):
                call(w=w)
        with pytest.raises(ValueError, match='GM and R must be finite and R positive'):
            call(R=0.0)
    series = ga.engine.OrderMajorSeries(None, 31, 4)                 # looked at for its degree and length only
    with pytest.raises(ValueError, match='the series holds degrees up to 31, not 30'):
        ga.engine.acceleration_points_at(30, xyz, series, first, weights, pi.GM, pi.R)
    with pytest.raises(ValueError, match=r'first\[4\] is 3'):
        ga.engine.acceleration_points_at(31, xyz, series, first + 1, weights, pi.GM, pi.R)


def _datetimes(iso):
    return [datetime.datetime.fromisoformat(str(s)) for s in iso]


@pytest.mark.parametrize('tag', list(pi.CASES))
def test_windows_and_weights_match_fixture(golden, tag):
    data = golden('g32_points_at')
    epochs = _datetimes(data['iso_' + tag])
    assert epochs == pi.epochs(tag)
    assert np.array_equal(data['mjd_' + tag], np.array([ga.utilities._mjd(e) for e in epochs]))
    parts = pi.constituents(tag)
    series = parts[-1]
    first, weights = series.interpolation_windows(epochs)
    assert np.array_equal(first, data['first_' + tag])
    ref = data['weights_' + tag]
    assert weights.dtype == np.float64 and np.array_equal(weights, ref[:, -2:])       # the reference's expressions: the same bits
    # the epochs the fixture must hold: both ends, interior nodes, 5 microseconds behind a node, unsorted
    nodes = series.epochs()
    assert epochs[0] == nodes[-1] and first[0] == len(nodes) - 2 and weights[0].tolist() == [0.0, 1.0]
    assert epochs[1] == nodes[0] and first[1] == 0 and weights[1].tolist() == [1.0, 0.0]
    assert epochs[2] == nodes[3] and first[2] == 2 and weights[2].tolist() == [0.0, 1.0]
    assert epochs[4] - nodes[2] == datetime.timedelta(microseconds=5) and first[4] == 2 and 0 < weights[4, 1] < 1e-9
    assert any(b < a for a, b in zip(epochs, epochs[1:]))
    # modified Julian dates: the same windows (the 5 microseconds are dropped: that epoch is the node), weights within the
    # resolution of a date of 5e4 days, 2^-37 days of the 0.125 days between two nodes
    first_mjd, weights_mjd = series.interpolation_windows(data['mjd_' + tag])
    keep = np.arange(len(epochs)) != 4
    assert np.array_equal(first_mjd[keep], first[keep]) and first_mjd[4] == 1 and weights_mjd[4].tolist() == [0.0, 1.0]
    assert np.abs(weights_mjd[keep] - weights[keep]).max() <= 2 * 2.0 ** -37 / 0.125                  # numerator and denominator
    if pi.CASES[tag][2]:
        columns = np.concatenate([c.weights_at(epochs) for c in parts[:-1]], axis=1)
        assert columns.shape == (len(epochs), 5)
        assert np.all(np.abs(columns - ref[:, :5]) <= np.spacing(np.abs(ref[:, :5])))                 # 1 ulp
        columns_mjd = np.concatenate([c.weights_at(data['mjd_' + tag]) for c in parts[:-1]], axis=1)
        # tau of 3 years to 2^-37 days of 365.25; the phase 2 pi tau of the semi-annual cycle moves twice as fast as the annual one's
        assert np.abs(columns_mjd - columns).max() <= 4 * np.pi * 2.0 ** -36 / 182.625 + 5e-6 / 86400 / 182.625 * 4 * np.pi


@pytest.mark.parametrize('tag', list(pi.CASES))
def test_weights_match_evaluate_at(tag):
    """the blend of the weights is the field evaluate_at / interpolate_to return: coefficients within 1 ulp of each term's rounding"""
    epochs = pi.epochs(tag)[:12]
    parts = pi.constituents(tag)
    series = parts[-1]
    first, weights = series.interpolation_windows(epochs)
    anm = pi.series_coefficients(tag)
    for k, epoch in enumerate(epochs):
        blend = anm[first[k]] * weights[k, 0] + anm[first[k] + 1] * weights[k, 1]
        assert np.array_equal(blend, series.interpolate_to(epoch).anm), k
    if pi.CASES[tag][2]:
        model = pi.model_coefficients(tag)
        trend, annual = parts[0], parts[1]
        for k, epoch in enumerate(epochs):
            w = trend.weights_at([epoch])[0]
            assert np.array_equal(model[0] * w[0], trend.evaluate_at(epoch).anm)
            w = annual.weights_at([epoch])[0]
            got, ref = model[1] * w[0] + model[2] * w[1], annual.evaluate_at(epoch).anm
            assert np.all(np.abs(got - ref) <= 2 * np.spacing(np.abs(model[1]) + np.abs(model[2])))    # cos and sin within 1 ulp


def test_public_methods_reject_bad_arguments_before_the_device():
    tag = 'model31'
    parts = pi.constituents(tag)
    series, trend, annual = parts[-1], parts[0], parts[1]
    tv = ga.gravityfield.TimeVariableGravityField(parts)
    xyz = pi.positions(tag)[:8]
    epochs = pi.epochs(tag)[:8]
    mjd = np.array([pi.mjd(e) for e in epochs])
    nodes = pi.series_epochs()
    for target in (series, trend, annual, tv):
        for method in (target.gravitational_acceleration_at, target.gravitational_gradients_at, target.gravitational_potential_at):
            with pytest.raises(ValueError, match=r'must have shape \(M, 3\)'):
                method(xyz.T, epochs)
            with pytest.raises(ValueError, match='7 epochs for 8 points'):
                method(xyz, epochs[:7])
            with pytest.raises(ValueError, match='7 epochs for 8 points'):
                method(xyz, mjd[:7])
            with pytest.raises(ValueError, match='float64 array of shape'):
                method(xyz, mjd.astype(np.float32))
            with pytest.raises(ValueError, match='epoch 2 is 5'):
                method(xyz, epochs[:2] + [5] + epochs[3:])
            bad = mjd.copy()
            bad[3] = np.nan
            with pytest.raises(ValueError, match='epoch 3 is not finite'):
                method(xyz, bad)
        for method in (target.line_of_sight_acceleration_at, target.potential_difference_at):
            with pytest.raises(ValueError, match='8 positions of the first satellite but 7 of the second'):
                method(xyz, xyz[:7], epochs)
            with pytest.raises(ValueError, match='7 epochs for 8 points'):
                method(xyz, xyz + 1.0, epochs[:7])
        with pytest.raises(ValueError, match='same position'):
            target.line_of_sight_acceleration_at(xyz, xyz.copy(), epochs)
        with pytest.raises(ValueError, match=r'directions must have shape \(8, 3\)'):
            target.line_of_sight_acceleration_at(xyz, xyz + 1.0, epochs, directions=np.ones((7, 3)))
    # no extrapolation, by datetime and by date
    late = nodes[-1] + datetime.timedelta(microseconds=1)
    early = nodes[0] - datetime.timedelta(seconds=1)
    for target in (series, tv):
        with pytest.raises(ValueError, match='epoch 5 .* lies outside the series'):
            target.gravitational_acceleration_at(xyz, epochs[:5] + [late] + epochs[6:])
        with pytest.raises(ValueError, match='epoch 2 .* lies outside the series'):
            target.gravitational_potential_at(xyz, epochs[:2] + [early, late] + epochs[4:])
        bad = mjd.copy()
        bad[6] = pi.mjd(nodes[-1]) + 1e-6
        with pytest.raises(ValueError, match='epoch 6 .* lies outside the series'):
            target.gravitational_gradients_at(xyz, bad)
    one = ga.gravityfield.TimeSeries([pi.field(pi.series_coefficients(tag)[0], nodes[0])])
    with pytest.raises(ValueError, match='at least two data points'):
        one.gravitational_acceleration_at(xyz, [nodes[0]] * 8)
    mixed = [pi.field(a, e) for a, e in zip(pi.series_coefficients(tag)[:3], nodes)]
    mixed[1].GM *= 1.0 + 1e-9
    with pytest.raises(ValueError, match='common GM and R'):
        ga.gravityfield.TimeSeries(mixed).gravitational_acceleration_at(xyz, [nodes[0]] * 8)
    cosine, sine = pi.field(pi.model_coefficients(tag)[1]), pi.field(pi.model_coefficients(tag)[2])
    sine.R += 1.0
    with pytest.raises(ValueError, match='common GM and R'):
        ga.gravityfield.Oscillation(cosine, sine, 365.25, pi.REFERENCE_EPOCH).gravitational_potential_at(xyz, epochs)

    class Other:
        def copy(self):
            return self
    with pytest.raises(TypeError, match='need PotentialCoefficients, not Other'):
        ga.gravityfield.Trend(Other(), pi.REFERENCE_EPOCH).gravitational_acceleration_at(xyz, epochs)
    with pytest.raises(TypeError, match='need PotentialCoefficients, not Other'):
        ga.gravityfield.Oscillation(cosine, Other(), 365.25, pi.REFERENCE_EPOCH).gravitational_gradients_at(xyz, epochs)

    class Constant:
        def evaluate_at(self, epoch):
            return cosine
    with pytest.raises(TypeError, match='constituent .*Constant.* has no functionals at epochs'):
        ga.gravityfield.TimeVariableGravityField([trend, Constant(), series]).gravitational_acceleration_at(xyz, epochs)
    with pytest.raises(ValueError, match='without constituents'):
        ga.gravityfield.TimeVariableGravityField([]).gravitational_acceleration_at(xyz, epochs)


def test_adjacent_trends_and_cycles_are_merged():
    """[Trend, Oscillation, Oscillation, TimeSeries] is two calls: W = 5 on the stacked model fields, then the series' W = 2; a lower
    degree is zero-padded, another GM is not merged"""
    tag = 'model31'
    parts = pi.constituents(tag)
    epochs = pi.epochs(tag)[:10]
    calls = ga.gravityfield.TimeVariableGravityField(parts)._at_calls(epochs)
    assert [c.weights.shape for c in calls] == [(10, 5), (10, 2)] and [c.fixed for c in calls] == [True, False]
    assert np.array_equal(calls[0].coefficients, pi.model_coefficients(tag)) and not calls[0].first.any()
    assert np.array_equal(calls[0].weights, np.concatenate([c.weights_at(epochs) for c in parts[:3]], axis=1))
    assert np.array_equal(calls[1].coefficients, pi.series_coefficients(tag))
    low = pi.field(pi.model_coefficients(tag)[0][:11, :11])
    calls = ga.gravityfield.TimeVariableGravityField([ga.gravityfield.Trend(low, pi.REFERENCE_EPOCH), parts[1]])._at_calls(epochs)
    assert len(calls) == 1 and calls[0].max_degree == 31 and calls[0].coefficients.shape == (3, 32, 32)
    assert np.array_equal(calls[0].coefficients[0, :11, :11], low.anm) and not calls[0].coefficients[0, 11:].any() \
        and not calls[0].coefficients[0, :, 11:].any()
    other = pi.field(pi.model_coefficients(tag)[0])
    other.GM *= 2.0
    calls = ga.gravityfield.TimeVariableGravityField([ga.gravityfield.Trend(other, pi.REFERENCE_EPOCH), parts[1], parts[-1], parts[2]])._at_calls(epochs)
    assert [c.weights.shape[1] for c in calls] == [1, 2, 2, 2]
