"""
CPU checks of the observation leverages and the Huber reweighting: shg_leverages rejects bad arguments before any HIP call,
robust_least_squares has the reference's signature, the new functions and methods have the listed signatures, every ValueError of
PostFit.leverages fires on the host, huber_factors matches hand-made arrays, and the fixture g32_robust.npz and the host oracle of
tests/golden/leverage_inputs.py are what the GPU tests take them for.
"""
import ctypes
import inspect

import numpy as np
import pytest

import grates_amd as ga
import leverage_inputs as lev
import test_api_signatures as api


def _error(lib):
    return lib.shg_last_error().decode()


def test_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first

    def call(n=7, cols=10, Ui=dummy, ldu=7, X=dummy, ldx=10, out=dummy):
        return lib.shg_leverages(n, cols, Ui, ldu, X, ldx, out, None)
    for bad in (dict(n=-1, ldu=0), dict(cols=-1, ldx=0)):
        assert call(**bad) == -1
        assert 'shg_leverages: negative size' in _error(lib)
    assert call(ldu=6) == -1
    assert 'ldu 6 below n 7' in _error(lib)
    assert call(ldx=9) == -1
    assert 'ldx 9 below the 10 columns' in _error(lib)
    assert call(n=1 << 20, ldu=(1 << 20) + 1) == -1                                               # more than 2^40 values of Ui
    assert 'is too large' in _error(lib)
    assert call(n=1 << 11, ldu=1 << 11, cols=1 << 29, ldx=(1 << 29) + 1) == -1                     # ... of X
    assert 'is too large' in _error(lib)
    for missing in ('Ui', 'X', 'out'):
        assert call(**{missing: None}) == -1
        assert 'shg_leverages: NULL pointer' in _error(lib)
    assert call(n=0, ldu=0, Ui=None, X=None, out=None) == -1                                      # an empty sum still writes its zeros
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(cols=0, ldx=0, Ui=None, X=None, out=None) == 0
    with pytest.raises(_lib.ShgError, match='ldu 3 below n 7'):
        _lib.call('shg_leverages', 7, 10, dummy, 3, dummy, 10, dummy, None)
    assert _lib.PROTOTYPES['shg_leverages'] == [ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong,
                                                ctypes.c_void_p, ctypes.c_void_p]


def test_robust_least_squares_has_the_reference_signature():
    record = api.API['modules']['lstsq']['robust_least_squares']
    assert record['kind'] == 'function'
    assert api.compatible(record['signature'], api.params_of(ga.lstsq.robust_least_squares)) is None
    assert api.params_of(ga.lstsq.robust_least_squares) == record['signature']                    # nothing appended either


def test_signatures():
    def names(function):
        return list(inspect.signature(function).parameters)

    def defaults(function):
        return {name: prm.default for name, prm in inspect.signature(function).parameters.items() if prm.default is not inspect.Parameter.empty}
    lstsq, fit = ga.lstsq, ga.lstsq.PostFit
    assert names(ga.engine.leverages) == ['Ui', 'X', 'out'] and defaults(ga.engine.leverages) == dict(out=None)
    assert names(fit.leverages) == ['self', 'normals', 'elimination'] and defaults(fit.leverages) == dict(elimination=None)
    assert names(fit.redundancies) == ['self', 'normals', 'elimination'] and defaults(fit.redundancies) == dict(elimination=None)
    assert names(fit.standardised) == ['self', 'normals', 'sigma', 'factors', 'elimination']
    assert defaults(fit.standardised) == dict(sigma=None, factors=None, elimination=None)
    huber = dict(threshold=2.5, downweight_power=1.5, redundancy_threshold=1e-4)
    assert names(lstsq.huber_factors) == ['standardised', 'redundancies', 'factors', 'threshold', 'downweight_power', 'redundancy_threshold']
    assert defaults(lstsq.huber_factors) == dict(factors=None, **huber)
    assert names(lstsq.huber_iterate) == ['system', 'post_fit', 'weights', 'threshold', 'downweight_power', 'redundancy_threshold', 'max_iter']
    assert defaults(lstsq.huber_iterate) == dict(max_iter=10, **huber)
    assert names(lstsq.robust_least_squares) == ['l', 'A', 'threshold', 'downweight_power', 'redundancy_threshold', 'max_iter']
    assert defaults(lstsq.robust_least_squares) == dict(max_iter=10, **huber)


# ---- the checks of PostFit.leverages, without a device --------------------------------------------------------------------------------------
M, MIN_DEGREE, MAX_DEGREE = 12, 2, 4
P = (MAX_DEGREE + 1) ** 2 - MIN_DEGREE ** 2


def _bound_fit(model=None, temporal=False, setup=None):
    """a PostFit bound to checked observations as its pass binds it, nothing uploaded"""
    xyz = lev.sphere_positions(M, 4280)
    observations = ga.lstsq._observations('accelerations', dict(xyz=xyz, g=np.zeros((M, 3)), weights=None),
                                          ga.engine.Band(MIN_DEGREE, MAX_DEGREE, lev.GM, lev.R))
    fit = ga.lstsq.PostFit(np.zeros(P), None, model, xyz)
    fit._bind(observations, ga.lstsq._StochasticModel.of(model), 256, setup, temporal)
    return fit


def _system(parameters=P, blocks=1, status='cholesky_factor'):
    index = [parameters * i for i in range(blocks + 1)]
    ne = ga.lstsq.NormalEquations(ga.lstsq.BlockMatrix(index, index), np.zeros((parameters * blocks, 1)), 0.0, 3 * M)
    ne.status = status
    return ne


def test_leverages_refuse_on_the_host():
    """every ValueError fires before anything reaches the device: on a machine without a GPU the first upload would raise a RuntimeError
    instead"""
    fit = _bound_fit()
    for method in (fit.leverages, fit.redundancies, fit.standardised):
        with pytest.raises(ValueError, match='TemporalParameters.*out of scope'):
            method(_system(blocks=3))
        with pytest.raises(ValueError, match='holds normal_matrix: solve the system first'):
            method(_system(status='normal_matrix'))
        with pytest.raises(ValueError, match='holds covariance_matrix'):
            method(_system(status='covariance_matrix'))
        with pytest.raises(ValueError, match='the system has 16 x 16 parameters, the observations 21'):
            method(_system(parameters=16))
    with pytest.raises(ValueError, match='TemporalParameters.*out of scope'):
        _bound_fit(temporal=True).leverages(_system())
    with pytest.raises(ValueError, match='need the pass of an of_\\* call'):
        ga.lstsq.PostFit(np.zeros(P), None, None, None).leverages(_system())
    # under ArcParameters: no elimination at all (a combined system), and one without kept columns
    model = ga.lstsq.ArcParameters(ga.lstsq.arc_basis([0, 6], M, degree=1), [0, 6])
    arc_fit = _bound_fit(model)
    with pytest.raises(ValueError, match='pass elimination=ne.arc_elimination'):
        arc_fit.leverages(_system())
    dropped = ga.lstsq.ArcElimination(np.full((2, 3), 2), np.zeros((2, 3, 2, 2)), np.zeros((2, 3, 2)), True, None)
    with pytest.raises(ValueError, match=r'ArcParameters\(keep=True\)'):
        arc_fit.leverages(_system(), dropped)
    own = _system()
    own.arc_elimination = dropped
    with pytest.raises(ValueError, match=r'ArcParameters\(keep=True\)'):
        arc_fit.standardised(own)
    assert dropped._columns() is None


# ---- huber_factors ------------------------------------------------------------------------------------------------------------------------
def test_huber_factors_on_hand_made_arrays():
    t = np.array([[1.0, 5.0, np.nan], [2.5, np.inf, 10.0], [25.0, 3.0, 2.6]])
    r = np.array([[0.9, 0.5, 0.9], [0.9, 0.9, 1e-5], [0.9, 1e-4, 0.2]])
    factors, outliers = ga.lstsq.huber_factors(t, r)
    assert outliers.dtype == bool and np.array_equal(outliers, [[False, True, False], [False, False, False], [True, False, True]])
    expected = np.ones((3, 3))
    expected[0, 1], expected[2, 0], expected[2, 2] = 0.5 ** 3, 0.1 ** 3, (2.5 / 2.6) ** 3
    assert np.allclose(factors, expected, rtol=4 * 2.0 ** -53, atol=0) and np.all(factors[~outliers] == 1.0)
    # nan, inf, t at the threshold, r at its threshold: not flagged; the earlier factor stays, as in the reference
    earlier = np.full((3, 3), 0.25)
    again, flags = ga.lstsq.huber_factors(t, r, earlier)
    assert np.array_equal(flags, outliers) and np.all(again[~outliers] == 0.25) and np.array_equal(again[outliers], factors[outliers])
    # the reference's std_dev = (t / threshold)^power, applied as 1 / std_dev^2, with other keywords
    f, o = ga.lstsq.huber_factors(np.array([8.0, 1.0]), np.array([0.5, 0.5]), threshold=2.0, downweight_power=1.0, redundancy_threshold=0.4)
    assert np.array_equal(o, [True, False]) and np.array_equal(f, [1.0 / 16.0, 1.0])
    assert not ga.lstsq.huber_factors(np.array([8.0]), np.array([0.5]), redundancy_threshold=0.5)[1][0]
    # per-point factors: the smallest over the components
    point, flags = ga.lstsq.huber_factors(t, r, np.array([1.0, 0.5, 1.0]))
    assert point.shape == (3,) and np.array_equal(flags, outliers)
    assert np.allclose(point, [0.125, 0.5, 0.001], rtol=4 * 2.0 ** -53, atol=0)
    for bad in (dict(factors=np.ones((2, 3))), dict(threshold=0.0), dict(downweight_power=-1.0)):
        with pytest.raises(ValueError, match='huber_factors'):
            ga.lstsq.huber_factors(t, r, **bad)
    with pytest.raises(ValueError, match='one shape'):
        ga.lstsq.huber_factors(t, r[:2])
    assert np.array_equal(lev.huber_factors(t, r, np.ones((3, 3)), 2.5, 1.5, 1e-4)[0], factors)     # the oracle's own statement


# ---- the fixture and the oracle --------------------------------------------------------------------------------------------------------------
def test_fixture_and_oracle(golden):
    """the reference flags exactly the planted five at max_iter=1 on orthonormal columns, where its formulas are the textbook ones: the
    host IRLS of the tests gives the same solution, covariance and flags there; and on the general problem it flags exactly the
    planted five in all ten iterations while sigma0 falls from 4.04 to 0.88"""
    data = golden('g32_robust')
    l, A, truth, planted = lev.robust_problem(True)
    assert np.array_equal(data['l'], l) and np.array_equal(data['A'], A) and np.array_equal(data['planted'], planted)
    assert np.array_equal(np.flatnonzero(data['outlier_flag']), planted) and data['outlier_flag'].dtype == bool
    assert np.abs(A.T @ A - np.eye(6)).max() <= 8 * 2.0 ** -53
    first = lev.irls(l, A, max_iter=1)[0]
    assert np.array_equal(first['flags'], data['outlier_flag'])
    assert np.abs(first['x'] - data['x_hat']).max() <= 1e-13 * np.abs(data['x_hat']).max()
    assert np.abs(first['sigma0'] ** 2 * np.linalg.inv(A.T @ A) - data['C']).max() <= 1e-13 * np.abs(data['C']).max()
    l, A, truth, planted = lev.robust_problem(False)
    history = lev.irls(l, A)
    assert len(history) == 10 and all(np.array_equal(np.flatnonzero(step['flags']), planted) for step in history)
    assert abs(history[0]['sigma0'] - 4.04) < 0.01 and abs(history[-1]['sigma0'] - 0.88) < 0.01
    assert np.linalg.norm(history[-1]['x'] - truth) < 0.2 * np.linalg.norm(np.linalg.lstsq(A, l, rcond=None)[0] - truth)


def test_host_hat_routes_agree():
    """A self-check of the oracles, not of the feature (it passes without it): the two host routes of the GPU tests, normals and QR, on
    a small problem with arc columns give the same diagonal, in 0 .. 1, with the sum P + rank of the arc columns"""
    rng = np.random.default_rng(4281)
    A, B = rng.standard_normal((60, 7)), np.zeros((60, 4))
    B[:30, 0], B[:30, 1], B[30:, 2], B[30:, 3] = 1.0, np.linspace(-1, 1, 30), 1.0, np.linspace(-1, 1, 30)
    Q = lev.orthonormal_arc_columns([B[:, :2], B[:, 2:]])
    reduced = A - Q @ (Q.T @ A)
    factor = np.linalg.cholesky(reduced.T @ reduced).T
    first, bound = lev.hat_by_normals(A, factor, Q, 30)
    second, rank = lev.hat_by_qr(np.hstack((A, B)))
    assert rank == 11 and np.abs(first - second).max() <= 1e-13 and abs(first.sum() - 11) <= 1e-12
    assert first.min() >= 0 and first.max() <= 1 and np.all(bound > 0) and bound.max() < 1e-11
