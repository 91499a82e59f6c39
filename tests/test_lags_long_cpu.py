"""
CPU checks of the covariance functions of any lag: the argument checks of shg_segment_lag_products_long before any HIP call, its
host rules under a sanitizer (tools/lags_long_host_check.cpp, a stand-alone program), the constants it reports, the signatures of the new
Python names, the checks of PostFit.covariance_lags and covariance_model before anything reaches the device, and the lag windows.
"""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import grates_amd as ga
import lags_long_inputs as ll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C entry points --------------------------------------------------------------------------------------------------------------
def test_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    call = lib.shg_segment_lag_products_long
    assert _lib.PROTOTYPES['shg_segment_lag_products_long'] == _lib.PROTOTYPES['shg_segment_lag_products']
    X, seg, S = (ctypes.c_void_p(address) for address in (0x10000000, 0x30000000, 0x40000000))   # never dereferenced

    def error():
        return lib.shg_last_error().decode()
    #    rows M X ldx lags nseg seg S stream
    for rows, M, ldx in ((-1, 10, 10), (6, -1, 10), (6, 10, -1)):
        assert call(rows, M, X, ldx, 5, 2, seg, S, None) == -1
        assert 'shg_segment_lag_products_long: negative size' in error()
    for lags in (-1, 4096, 1 << 20):
        assert call(6, 10, X, 10, lags, 2, seg, S, None) == -1
        assert 'lags {0} outside 0 .. 4095'.format(lags) in error()
    assert call(6, 10, X, 10, 5, -1, seg, S, None) == -1
    assert 'nseg -1 is negative' in error()
    assert call(6, 10, X, 9, 5, 2, seg, S, None) == -1
    assert 'ldx 9 below M 10' in error()
    for pointers in ((None, seg, S), (X, None, S), (X, seg, None)):
        assert call(6, 10, pointers[0], 10, 5, 2, pointers[1], pointers[2], None) == -1
        assert 'shg_segment_lag_products_long: NULL pointer' in error()
    assert call((1 << 20) + 1, 1 << 20, X, 1 << 20, 5, 2, seg, S, None) == -1                              # 2^40 + 2^20 values of X
    assert 'values of X are too large' in error()
    assert call(1 << 20, 4, X, 4, 15, (1 << 16) + 1, seg, S, None) == -1                                    # ... of S alone
    assert 'values of S are too large' in error()
    assert call(1 << 20, 4, X, 4, 15, 1 << 15, seg, S, None) == -1                                          # ... of the workspace alone: 256 sums per slot
    assert 'of the workspace are too large' in error()
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(0, 10, None, 10, 5, 2, None, None, None) == 0
    assert call(6, 10, None, 10, 4095, 0, None, None, None) == 0
    assert call(6, 10, X, 10, 4096, 0, seg, S, None) == -1                                                 # the checks come before the early return
    with pytest.raises(_lib.ShgError, match='lags 4096 outside 0 .. 4095'):
        _lib.call('shg_segment_lag_products_long', 6, 10, X, 10, 4096, 2, seg, S, None)


def test_info():
    info = ga.engine.segment_lag_long_info()
    assert sorted(info) == ['chunk', 'max_lags', 'tile_lags']
    assert info['max_lags'] == 4095 == ga.lstsq.MAX_COVARIANCE_ORDER
    assert info['tile_lags'] > 0 and 4096 % info['tile_lags'] == 0 and info['chunk'] > 0
    from grates_amd import _lib
    assert _lib.load().shg_segment_lag_long_info(None, None, None) == 0                                    # NULL pointers are skipped


def test_host_rules_run_clean_under_a_sanitizer(tmp_path):
    """the argument rules, the work items and every index of the kernels as a stand-alone CPU program with its own main, built with
    -fsanitize=address,undefined: nothing of it is loaded into Python"""
    compiler = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert compiler, 'a host C++ compiler is needed'
    program = str(tmp_path / 'lags_long_host_check')
    subprocess.run([compiler, '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tools', 'lags_long_host_check.cpp'), '-o', program], check=True)
    done = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and done.stdout.strip() == 'ok', done.stdout


# ---- the Python names ----------------------------------------------------------------------------------------------------------------
def test_signatures():
    def listed(function):
        return [(prm.name, prm.default) for prm in inspect.signature(function).parameters.values()]
    empty = inspect.Parameter.empty
    assert listed(ga.engine.segment_lag_products_long) == listed(ga.engine.segment_lag_products) == \
        [('X', empty), ('seg', empty), ('lags', empty), ('out', None)]
    assert listed(ga.lstsq.PostFit.covariance_lags) == listed(ga.lstsq.PostFit.covariance_function) == \
        [('self', empty), ('maximum_lag', empty), ('per_component', False), ('biased', True)]
    assert listed(ga.lstsq.PostFit.covariance_model) == [('self', empty), ('maximum_lag', empty), ('per_component', False), ('window', None)]
    assert ga.lstsq.MAX_WHITENING_ORDER == 128 and ga.lstsq.MAX_COVARIANCE_ORDER == 4095


class _NoDevice:
    """stands where the residuals on the device are: any use beyond the shape is an error"""

    def __init__(self, K, count):
        self.shape = (K, count)

    def __getattr__(self, name):
        raise AssertionError('the device was touched: ' + name)


def _bare_fit(arcs, count, K=2):
    """a PostFit with the state covariance_lags and covariance_model check before they touch the device"""
    fit = ga.lstsq.PostFit(None, None, None, None)
    fit.arcs = np.asarray(arcs)
    fit._PostFit__rows, fit._PostFit__seg = _NoDevice(K, count), _NoDevice(1, len(arcs) + 1)
    return fit


def test_every_error_comes_before_the_device():
    fit = _bare_fit([0, 1, 4, 300], 700)
    for lag in (-1, 4096, 2.5, 1 << 20):
        with pytest.raises(ValueError, match='maximum_lag must be an integer in 0 .. 4095'):
            fit.covariance_lags(lag)
        with pytest.raises(ValueError, match='maximum_lag must be an integer in 0 .. 4095'):
            fit.covariance_model(lag)
        with pytest.raises(ValueError, match='maximum_lag must be an integer in 0 .. 4095'):
            fit.covariance_model(lag, window='no such window')                                      # the lag first
    with pytest.raises(ValueError, match='maximum_lag must be an integer in 0 .. 128'):             # unchanged
        fit.covariance_function(129)
    short = _bare_fit([0, 3, 7], 10)
    with pytest.raises(ValueError, match='no arc is longer than 4 points: no pair at lag 4'):
        short.covariance_lags(5, biased=False)
    with pytest.raises(ValueError, match='no arc is longer than 400 points: no pair at lag 400'):
        fit.covariance_lags(700, per_component=True, biased=False)
    for window in ('hann', 'Parzen', '', np.ones(5), np.ones(302), np.ones((301, 1)), 0.5 * np.ones(301), np.full(301, np.nan), [1.0, 'a'], 3.0, object()):
        with pytest.raises(ValueError, match='window must be None'):
            fit.covariance_model(300, window=window)
    infinite = np.ones(301)
    infinite[7] = np.inf
    with pytest.raises(ValueError, match='window must be None'):
        fit.covariance_model(300, per_component=True, window=infinite)


# ---- the windows -----------------------------------------------------------------------------------------------------------------------
def _toeplitz(c):
    index = np.arange(len(c))
    return c[np.abs(index[:, None] - index[None, :])]


@pytest.mark.parametrize('q', [0, 1, 2, 63, 300])
def test_windows(q):
    k = np.arange(q + 1)
    bartlett, parzen = ga.lstsq.lag_window('bartlett', q), ga.lstsq.lag_window('parzen', q)
    assert np.array_equal(ga.lstsq.lag_window(None, q), np.ones(q + 1))
    assert np.allclose(bartlett, 1 - k / (q + 1), rtol=4e-16, atol=0)
    x = k / (q + 1)
    assert np.allclose(parzen, np.where(2 * k <= q + 1, 1 - 6 * x ** 2 + 6 * x ** 3, 2 * (1 - x) ** 3), rtol=1e-14, atol=0)
    for w in (bartlett, parzen):
        assert w.shape == (q + 1,) and w[0] == 1.0 and np.all(np.diff(w) < 0) and np.all(w > 0)
    given = np.linspace(1.0, 0.25, q + 1)
    assert np.array_equal(ga.lstsq.lag_window(given, q), given) and np.array_equal(ga.lstsq.lag_window(list(given), q), given)


def test_windows_are_positive_semi_definite():
    for name in ('bartlett', 'parzen'):
        lowest = np.linalg.eigvalsh(_toeplitz(ga.lstsq.lag_window(name, 63))).min()
        print('{0}: smallest eigenvalue of Toeplitz(w) at q = 63: {1:.3e}'.format(name, lowest))
        assert lowest >= -1e-12


@pytest.mark.parametrize('window', ['bartlett', 'parzen'])
def test_a_tapered_estimate_still_builds_a_covariance_function(window):
    """the biased estimate of a sample is positive semi-definite, and so is its product with a positive semi-definite window"""
    q = 63
    noise = ll.coloured_noise(200, 1, 40, 3670)[0]
    estimate = ll.covariance(noise, [0, 90], q, True)[2]
    assert np.linalg.eigvalsh(_toeplitz(estimate)).min() >= -1e-12 * estimate[0]
    model = ga.lstsq.CovarianceFunction(estimate * ga.lstsq.lag_window(window, q))
    assert model.maximum_order == q and np.all(np.isfinite(model.taps())) and np.all(model.taps()[:, 0] > 0)
    rough = estimate.copy()
    rough[1] = 1.5 * estimate[0]                                                                    # |c_1| w_1 > c_0: no window rescues this
    with pytest.raises(ValueError, match='not positive definite'):
        ga.lstsq.CovarianceFunction(rough * ga.lstsq.lag_window(window, q))
