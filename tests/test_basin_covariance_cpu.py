"""
CPU checks of the basin functionals / basin covariance API: the two new C entry points reject bad arguments before any HIP call, the
Python methods reject bad shapes before anything reaches the device, and the fixture g21_basin_covariance.npz is consistent with itself.
"""
import ctypes
import datetime

import numpy as np
import pytest

import basin_covariance_inputs as ci
import grates_amd as ga


def _error(lib):
    return lib.shg_last_error().decode()


def test_basin_covariance_entry_points_reject_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    for B in (0, 65, -1):
        assert lib.shg_basin_covariance(B, 10, dummy, 10, dummy, 10, dummy, None) == -1
        assert '1 to 64 are supported' in _error(lib)
    assert lib.shg_basin_covariance(4, 0, dummy, 10, dummy, 10, dummy, None) == -1
    assert 'at least 1 expected' in _error(lib)
    for args in ((None, 10, dummy, 10, dummy), (dummy, 10, None, 10, dummy), (dummy, 10, dummy, 10, None)):
        assert lib.shg_basin_covariance(4, 10, args[0], args[1], args[2], args[3], args[4], None) == -1
        assert 'NULL pointer' in _error(lib)
    assert lib.shg_basin_covariance(4, 10, dummy, 9, dummy, 10, dummy, None) == -1
    assert 'leading dimensions' in _error(lib)
    assert lib.shg_basin_covariance(4, 10, dummy, 10, dummy, 3, dummy, None) == -1
    assert 'leading dimensions' in _error(lib)
    with pytest.raises(_lib.ShgError, match='65 masks, 1 to 64 are supported'):
        _lib.call('shg_basin_functionals', None, dummy, 65, dummy, 0, dummy, None)
    with pytest.raises(_lib.ShgError, match='0 masks, 1 to 64 are supported'):
        _lib.call('shg_basin_functionals', None, dummy, 0, dummy, 0, dummy, None)
    with pytest.raises(_lib.ShgError, match='NULL pointer'):
        _lib.call('shg_basin_functionals', None, dummy, 3, dummy, 0, dummy, None)
    with pytest.raises(_lib.ShgError, match='NULL pointer'):
        _lib.call('shg_basin_functionals', dummy, None, 3, dummy, 0, dummy, None)


def test_python_side_errors():
    grid = ga.grid.GeographicGrid(10, 10)
    P = grid.point_count
    ok = np.zeros((2, P), dtype=bool)
    with pytest.raises(ValueError, match='do not fit a grid'):
        grid.basin_functionals(np.zeros((2, P + 1), dtype=bool), 0, 4)
    with pytest.raises(ValueError, match='must be boolean'):
        grid.basin_functionals(np.zeros((2, P)), 0, 4)
    with pytest.raises(ValueError, match='65 masks'):
        grid.basin_functionals(np.zeros((65, P), dtype=bool), 0, 4)
    with pytest.raises(ValueError, match='must be square'):
        grid.basin_covariance(np.zeros((25, 24)), ok, 0, 4)
    with pytest.raises(ValueError, match=r'must have shape \(21, 21\)'):
        grid.basin_covariance(np.zeros((25, 25)), ok, 2, 4)
    with pytest.raises(ValueError, match='65 masks'):
        grid.basin_covariance(np.zeros((25, 25)), np.zeros((65, P), dtype=bool), 0, 4)
    fields = []
    for k, GM in enumerate((3.986004415e14, 3.986004418e14)):
        gf = ga.gravityfield.PotentialCoefficients(GM, 6.3781363e6, 4)
        gf.epoch = datetime.datetime(2010, 1 + k, 15)
        fields.append(gf)
    with pytest.raises(ValueError, match='common GM and R'):
        grid.basin_averages(ga.gravityfield.TimeSeries(fields), ok)
    with pytest.raises(TypeError):
        grid.basin_averages(np.zeros((2, 5, 5)).tolist(), ok)


def test_fixture_is_consistent(golden):
    g = golden('g21_basin_covariance')
    for case in ci.CASES:
        t = ci.tag(*case)
        L, d = ci.covariance(case[2])
        F = g['F_' + t]
        assert F.shape == (4, (ci.MAX_DEGREE + 1) ** 2 - case[2] ** 2)
        assert np.all(np.isnan(F[3])) and np.all(np.isfinite(F[:3]))
        C = (F @ L) @ (F @ L).T + (F * d) @ F.T
        ref = g['C_' + t]
        scale = np.abs(ref[:3, :3]).max()
        assert np.abs(C[:3, :3] - ref[:3, :3]).max() <= 1e-12 * scale, t
        if case in ci.FILTERED:
            FW = g['FW_' + t]
            CW = (FW @ L) @ (FW @ L).T + (FW * d) @ FW.T
            assert np.abs(CW[:3, :3] - g['CW_' + t][:3, :3]).max() <= 1e-12 * np.abs(g['CW_' + t][:3, :3]).max(), t
