"""
CPU checks of noise given by a covariance function: lstsq.CovarianceFunction.taps() against the AR models the reference derives from
the same lags (tests/golden/g27_whitening.npz, g33_covariance_noise.npz) and against inv(cholesky(Toeplitz)) in np.longdouble at long
orders, every ValueError before anything reaches the device, the unchanged errors of AR sequences, the signatures of the new names
and the argument checks of shg_whiten_rows_long before any HIP call.
"""
import ctypes
import inspect
import time

import numpy as np
import pytest

import covariance_noise_inputs as ci
import design_inputs as di
import grates_amd as ga
import whitening_inputs as wi

U = 2.0 ** -53


def _reference_taps(coefficients, variances):
    """the table of whitening_taps from recorded coefficients [q + 1, q] and variances [q + 1]"""
    sigma = np.sqrt(variances)
    return np.hstack(((1.0 / sigma)[:, None], -coefficients / sigma[:, None]))


def _route_deviation(c):
    """(W64, W80, deviation): inv(cholesky(Toeplitz(c))) in float64 and in np.longdouble and their largest difference over max|W|"""
    W64, W80 = ci.inverse_cholesky(ci.toeplitz(c)), ci.inverse_cholesky(ci.toeplitz(c, np.longdouble))
    return W64, W80, float(np.abs(W64 - W80).max() / np.abs(W80).max())


# ---- taps ------------------------------------------------------------------------------------------------------------------------------
# tolerance of the three comparisons: 10 times the deviation of the float64 Cholesky route from the np.longdouble one (two correct
# routes that differ by the conditioning of the Toeplitz matrix), floor 1e-13, of max|W|
@pytest.mark.parametrize('name', sorted(wi.PROCESSES))
def test_taps_against_the_models_of_the_reference(golden, name):
    data = golden('g27_whitening')
    p = wi.order(name)
    function = wi.covariance_function(name)
    model = ga.lstsq.CovarianceFunction(function)                                  # [1, 1] lags, as from_covariance_function takes them
    assert model.maximum_order == p and model.dimension == 1
    taps = model.taps()
    assert taps.shape == (p + 1, p + 1) and taps.dtype == np.float64 and np.array_equal(taps, np.tril(taps)) and np.all(taps[:, 0] > 0)
    assert np.array_equal(ga.lstsq.CovarianceFunction(np.array([lag[0, 0] for lag in function])).taps(), taps)      # a 1-D array
    sequence = wi.sequence(data, name, ga.lstsq)
    expected = ga.lstsq.whitening_taps(sequence)[0]
    deviation = _route_deviation(wi.covariance(name, p + 1))[2]
    tolerance = max(10 * deviation, 1e-13) * np.abs(expected).max()
    print('{0}: taps differ by {1:.2e}, Cholesky routes by {2:.2e} of max|W|'.format(name, np.abs(taps - expected).max() / np.abs(expected).max(), deviation))
    assert np.abs(taps - expected).max() <= tolerance
    assert np.array_equal(ga.lstsq.whitening_taps(model), taps[None])


def test_taps_against_the_new_fixture(golden):
    data = golden('g33_covariance_noise')
    q = ci.ORDER
    assert np.array_equal(data['covariance'], ci.covariance(q + 1))
    taps = ga.lstsq.CovarianceFunction(data['covariance']).taps()
    expected = _reference_taps(data['coefficients'], data['variances'])
    deviation = _route_deviation(data['covariance'])[2]
    scale = np.abs(expected).max()
    tolerance = max(10 * deviation, 1e-13)
    print('q 40: taps differ by {0:.2e}, Cholesky routes by {1:.2e} of max|W|'.format(np.abs(taps - expected).max() / scale, deviation))
    assert np.abs(taps - expected).max() <= tolerance * scale
    for L in ci.LENGTHS:                                                            # W^T W is the reference's normal_equations(L)
        W = ci.dense_filter(taps, ga.lstsq.arc_stages(None, L, q))
        reference = data['normals{0}'.format(L)]
        assert reference.shape == (L, L) and not np.any(np.tril(reference, -1))
        # the dot-product bound of tests/test_whitening_cpu.py, and |dW|^T |W| + |W|^T |dW| for taps within the tolerance above
        bound = 2 * (q + 4) * U * np.abs(reference).max() + 2 * tolerance * scale * np.abs(W).sum(axis=0).max()
        err = np.abs(np.triu(W.T @ W) - reference).max()
        print('    normals of {0} epochs: {1:.2e} of the bound'.format(L, err / bound))
        assert err <= bound


@pytest.mark.parametrize('q', [300, 2047])
def test_one_arc_filter_is_the_inverse_cholesky_factor_at_long_order(q):
    """the condition number of the Toeplitz matrix is 303 at q = 300 and 411 at q = 2047: the white floor of 0.1 bounds it"""
    c = ci.covariance(q + 1)
    started = time.perf_counter()
    taps = ga.lstsq.CovarianceFunction(c).taps()
    seconds = time.perf_counter() - started
    W = ci.dense_filter(taps, np.arange(q + 1))
    _, W80, deviation = _route_deviation(c)
    err = float(np.abs(W - W80).max() / np.abs(W80).max())
    print('q {0}: W from the taps {1:.2e}, float64 Cholesky {2:.2e} of max|W| off np.longdouble; taps in {3:.2f} s'.format(q, err, deviation, seconds))
    assert 0.0 < deviation and err <= max(10 * deviation, 1e-13)


def test_the_largest_table_builds_in_seconds():
    q = ga.lstsq.MAX_COVARIANCE_ORDER
    assert q == 4095
    started = time.perf_counter()
    taps = ga.lstsq.whitening_taps(ga.lstsq.CovarianceFunction(ci.covariance(q + 1)))
    seconds = time.perf_counter() - started
    print('q 4095: {0:.2f} s'.format(seconds))
    assert taps.shape == (1, q + 1, q + 1) and np.all(np.isfinite(taps)) and seconds < 30.0
    stage = ga.lstsq.arc_stages([0, 5000], 9000, q)                                 # stage = min(t - arc start, q) with the new q
    assert stage[4999] == q and stage[5000] == 0 and stage[8999] == 3999


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_covariance_function_checks():
    make = ga.lstsq.CovarianceFunction
    assert make([2.0]).taps().tolist() == [[1.0 / np.sqrt(2.0)]] and make([2.0]).maximum_order == 0
    assert make(np.array([[[1.0]], [[0.5]]])).maximum_order == 1
    for bad in ([1.0, np.nan], [np.inf, 0.5], [1.0, -np.inf]):
        with pytest.raises(ValueError, match='not finite'):
            make(bad)
    for bad in ([0.0, 0.0], [-1.0, 0.5]):
        with pytest.raises(ValueError, match='c_0'):
            make(bad)
    with pytest.raises(ValueError, match='order 1 .*not positive definite'):
        make([1.0, 1.5])
    with pytest.raises(ValueError, match='order 2 .*not positive definite'):
        make([1.0, 0.9, 0.2])
    with pytest.raises(ValueError, match='maximum order 4096 of the covariance function above 4095'):
        make(np.ones(4097))
    with pytest.raises(ValueError, match='dimension 2'):
        make([np.eye(2), 0.5 * np.eye(2)])
    for bad in (None, 5, [], np.ones((3, 2)), 'abc'):
        with pytest.raises(ValueError, match='covariance_function must hold'):
            make(bad)


def test_whitening_taps_accepts_functions_and_keeps_its_errors(golden):
    taps = ga.lstsq.whitening_taps
    three, five = ga.lstsq.CovarianceFunction(ci.covariance(4)), ga.lstsq.CovarianceFunction(ci.covariance(6))
    long = ga.lstsq.CovarianceFunction(ci.covariance(130))
    assert taps(long).shape == (1, 130, 130) and taps([five, five, five]).shape == (3, 6, 6) and np.array_equal(taps((five,))[0], five.taps())
    with pytest.raises(ValueError, match='differ in their maximum order'):
        taps([three, five])
    sequence = wi.sequence(golden('g27_whitening'), 'ar5', ga.lstsq)
    for mixed in ([five, sequence], [sequence, five], [five, None]):
        with pytest.raises(ValueError, match='noise_model must be'):
            taps(mixed)
    for bad in (None, 5, [], 'ar5'):
        with pytest.raises(ValueError, match='noise_model must be'):
            taps(bad)
    models = [ga.lstsq.AutoregressiveModel([0.1 / (k + 1) * np.eye(1) for k in range(s)], np.eye(1)) for s in range(130)]
    with pytest.raises(ValueError, match='maximum order 129 of the noise model above 128'):
        taps(ga.lstsq.AutoregressiveModelSequence(models))
    assert taps(ga.lstsq.AutoregressiveModelSequence(models[:129])).shape == (1, 129, 129)
    with pytest.raises(ValueError, match='maximum_lag must be an integer in 0 .. 128'):
        ga.lstsq.PostFit.covariance_function(None, 129)


def test_every_surface_checks_the_model_before_the_device():
    """every ValueError below is raised without a GPU"""
    ls = ga.lstsq
    xyz = di.positions()[:5]
    long = ls.CovarianceFunction(ci.covariance(300))
    other = ls.CovarianceFunction(ci.covariance(6))
    assert ls.ColouredNoise(long, [0, 3]).noise_model is long
    assert ls.ArcParameters(ls.arc_basis([0, 3], 5, degree=0), [0, 3], noise_model=long).noise_model is long
    with pytest.raises(ValueError, match='differ in their maximum order'):
        ls.ColouredNoise([long, other, other])
    with pytest.raises(ValueError, match='differ in their maximum order'):
        ls.ArcParameters(ls.arc_basis([0, 3], 5, degree=0), [0, 3], noise_model=[long, other, other])
    with pytest.raises(ValueError, match='arcs must'):
        ls.NormalEquations.from_accelerations(xyz, np.ones((5, 3)), 0, 4, noise_model=long, arcs=[0, 5])
    with pytest.raises(ValueError, match='arcs must'):
        ls.ColouredNoise(long, [1, 2]).from_accelerations(xyz, np.ones((5, 3)), 0, 4)
    with pytest.raises(ValueError, match='2 noise models for 3 components'):
        ls.ColouredNoise([long, long]).from_accelerations(xyz, np.ones((5, 3)), 0, 4)
    with pytest.raises(ValueError, match='2 noise models for 3 components'):
        ls.decorrelate(np.ones((5, 3)), [long, long])
    with pytest.raises(ValueError, match='arcs must'):
        ls.decorrelate(np.ones(5), long, arcs=[0, 7])
    with pytest.raises(ValueError, match='arcs must'):
        ls.PostFit.of_accelerations(np.zeros(25), xyz, np.ones((5, 3)), 0, 4, model=ls.ColouredNoise(long, [0, 9]))


def test_signatures():
    assert list(inspect.signature(ga.lstsq.CovarianceFunction).parameters) == ['covariance_function']
    assert list(inspect.signature(ga.lstsq.CovarianceFunction.taps).parameters) == ['self']
    assert isinstance(ga.lstsq.CovarianceFunction.maximum_order, property) and isinstance(ga.lstsq.CovarianceFunction.dimension, property)
    assert ga.lstsq.MAX_COVARIANCE_ORDER == 4095 and ga.lstsq.MAX_WHITENING_ORDER == 128
    assert list(inspect.signature(ga.lstsq.whitening_taps).parameters) == ['noise_model']
    assert list(inspect.signature(ga.engine.whiten_rows).parameters) == ['X', 'taps', 'stage', 'channels', 'skip', 'out']
    from grates_amd import _lib
    assert _lib.PROTOTYPES['shg_whiten_rows_long'] == _lib.PROTOTYPES['shg_whiten_rows']


# ---- the C entry point ------------------------------------------------------------------------------------------------------------------
def test_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    call = lib.shg_whiten_rows_long
    X, Y, stage, taps = (ctypes.c_void_p(address) for address in (0x10000000, 0x20000000, 0x30000000, 0x30010000))   # never dereferenced

    def error():
        return lib.shg_last_error().decode()
    #    rows channels M  X  ldx stage taps q skip Y ldy stream
    for rows, M, ldx, ldy in ((-1, 10, 10, 10), (6, -1, 10, 10), (6, 10, -1, 10), (6, 10, 10, -1)):
        assert call(rows, 3, M, X, ldx, stage, taps, 5, 0, Y, ldy, None) == -1
        assert 'shg_whiten_rows_long: negative size' in error()
    for channels in (0, -3):
        assert call(6, channels, 10, X, 10, stage, taps, 5, 0, Y, 10, None) == -1
        assert 'channels {0} below 1'.format(channels) in error()
    assert call(7, 3, 10, X, 10, stage, taps, 5, 0, Y, 10, None) == -1
    assert 'rows 7 are not a multiple of channels 3' in error()
    for q in (-1, 4096):
        assert call(6, 3, 10, X, 10, stage, taps, q, 0, Y, 10, None) == -1
        assert 'shg_whiten_rows_long: order q {0} outside 0 .. 4095'.format(q) in error()
    for skip in (-1, 11):
        assert call(6, 3, 10, X, 10, stage, taps, 500, skip, Y, 10, None) == -1
        assert 'skip {0} outside 0 .. M 10'.format(skip) in error()
    assert call(6, 3, 10, X, 9, stage, taps, 500, 0, Y, 10, None) == -1
    assert 'ldx 9 below M 10' in error()
    assert call(6, 3, 10, X, 10, stage, taps, 500, 4, Y, 5, None) == -1
    assert 'ldy 5 below M - skip 6' in error()
    for pointers in ((None, stage, taps, Y), (X, None, taps, Y), (X, stage, None, Y), (X, stage, taps, None)):
        assert call(6, 3, 10, pointers[0], 10, pointers[1], pointers[2], 500, 0, pointers[3], 10, None) == -1
        assert 'shg_whiten_rows_long: NULL pointer' in error()
    assert call((1 << 20) + 1, 1, 1 << 20, X, 1 << 20, stage, taps, 500, 0, Y, 1 << 20, None) == -1        # 2^40 + 2^20 values
    assert 'are too large' in error()
    assert call(1 << 20, 1, 4, X, 4, stage, taps, 500, 0, Y, (1 << 20) + 1, None) == -1                     # ... of Y alone
    assert 'are too large' in error()
    base, span = 0x10000000, 8 * (5 * 704 + 700)
    for y in (base, base + 8, base + span - 8, base - span + 8, base + 8 * 704):
        assert call(6, 3, 700, ctypes.c_void_p(base), 704, stage, taps, 500, 0, ctypes.c_void_p(y), 704, None) == -1, hex(y)
        assert 'X and Y overlap' in error()
    assert call(6, 3, 700, ctypes.c_void_p(base), 704, stage, taps, 500, 5, ctypes.c_void_p(base + 40), 704, None) == -1
    assert 'X and Y overlap' in error()
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(0, 3, 10, None, 10, None, None, 500, 0, None, 10, None) == 0
    assert call(6, 3, 10, None, 10, None, None, 500, 10, None, 0, None) == 0
    assert call(6, 3, 0, None, 0, None, None, 0, 0, None, 0, None) == 0
    with pytest.raises(_lib.ShgError, match='rows 7 are not a multiple of channels 3'):
        _lib.call('shg_whiten_rows_long', 7, 3, 10, X, 10, stage, taps, 500, 0, Y, 10, None)
