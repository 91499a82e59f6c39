"""
CPU checks of the gravitational acceleration at points: the two C entry points reject bad arguments before any HIP call, the Python
methods reject bad position shapes before anything reaches the device, and the host path (as_tensor=False) reproduces the reference
fixture g22_acceleration.npz.
"""
import ctypes

import numpy as np
import pytest

import acceleration_inputs as ai
import grates_amd as ga


def _error(lib):
    return lib.shg_last_error().decode()


def test_acceleration_entry_points_reject_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    GM, R = ai.GM, ai.R
    for N, M, B in ((-1, 10, 1), (4, -1, 1), (4, 10, -2)):
        assert lib.shg_acceleration_points(N, dummy, M, 0, dummy, B, GM, R, dummy, None) == -1
        assert 'negative size' in _error(lib)
    for layout in (-1, 2):
        assert lib.shg_acceleration_points(4, dummy, 10, layout, dummy, 1, GM, R, dummy, None) == -1
        assert 'layout {0}, expected 0 (shared points) or 1 (points per epoch)'.format(layout) in _error(lib)
    for gm, r in ((float('nan'), R), (GM, 0.0), (GM, -R), (GM, float('inf'))):
        assert lib.shg_acceleration_points(4, dummy, 10, 0, dummy, 1, gm, r, dummy, None) == -1
        assert 'GM and R must be finite and R positive' in _error(lib)
    for xyz, anm, g in ((None, dummy, dummy), (dummy, None, dummy), (dummy, dummy, None)):
        assert lib.shg_acceleration_points(4, xyz, 10, 1, anm, 3, GM, R, g, None) == -1
        assert 'shg_acceleration_points: NULL pointer' in _error(lib)
    assert lib.shg_acceleration_points(4, dummy, 1 << 30, 0, dummy, 1 << 12, GM, R, dummy, None) == -1
    assert 'is too large' in _error(lib)
    # nothing to do: no pointer is looked at and no HIP call is made
    assert lib.shg_acceleration_points(4, None, 0, 0, None, 3, GM, R, None, None) == 0
    assert lib.shg_acceleration_points(4, None, 10, 1, None, 0, GM, R, None, None) == 0
    with pytest.raises(_lib.ShgError, match='Bpad 3 below B 4'):
        _lib.call('shg_acceleration_points_om', 4, dummy, 10, 0, dummy, 4, 3, GM, R, dummy, None)
    with pytest.raises(_lib.ShgError, match='shg_acceleration_points_om: NULL pointer'):
        _lib.call('shg_acceleration_points_om', 4, dummy, 10, 0, None, 4, 32, GM, R, dummy, None)
    with pytest.raises(_lib.ShgError, match='shg_acceleration_points_om: layout 5'):
        _lib.call('shg_acceleration_points_om', 4, dummy, 10, 5, dummy, 4, 32, GM, R, dummy, None)


def _series(count, N=4):
    fields = []
    for k in range(count):
        gf = ga.gravityfield.PotentialCoefficients(max_degree=N)
        gf.anm[0, 0] = 1.0
        gf.epoch = k
        fields.append(gf)
    return ga.gravityfield.TimeSeries(fields)


def test_python_shape_checks():
    gf = ga.gravityfield.PotentialCoefficients(max_degree=4)
    for shape in ((5,), (5, 2), (5, 4), (2, 5, 3)):
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
            gf.gravitational_acceleration(np.zeros(shape), as_tensor=True)
    series = _series(3)
    for shape in ((5,), (5, 2), (2, 5, 3), (4, 5, 3), (3, 5, 2), (1, 3, 5, 3)):
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\) or \(3, M, 3\)'):
            series.gravitational_acceleration(np.zeros(shape))
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\) or \(3, M, 3\)'):
            series.gravitational_acceleration(np.zeros(shape), as_tensor=True)


@pytest.mark.parametrize('tag', list(ai.CASES))
def test_host_path_matches_reference(golden, tag):
    """the host path of the port against the reference, bit for bit (as_tensor=False must stay exactly this)"""
    data = golden('g22_acceleration')
    N, kind, seed, _ = ai.CASES[tag]
    gf = ga.gravityfield.PotentialCoefficients(ai.GM, ai.R)
    gf.anm = ai.coefficients(N, kind, seed)
    xyz, ref = data['xyz_' + tag], data['g_' + tag]
    g = gf.gravitational_acceleration(xyz)
    assert isinstance(g, np.ndarray) and g.shape == ref.shape and g.dtype == np.float64
    assert np.all(np.isfinite(g))
    assert np.array_equal(g, ref), 'host path differs from the reference by {0:.3e} of max|g|'.format(np.max(np.abs(g - ref)) / np.max(np.abs(ref)))


def test_fixture_cases_cover_the_special_positions(golden):
    data = golden('g22_acceleration')
    for tag in ai.CASES:
        xyz = data['xyz_' + tag]
        r = np.sqrt(np.sum(xyz ** 2, axis=1))
        assert np.any((xyz[:, 0] == 0) & (xyz[:, 1] == 0)), tag                         # exact poles
        assert np.any((xyz[:, 0] < 0) & (xyz[:, 1] == 0) & np.signbit(xyz[:, 1])), tag    # antimeridian, y = -0
        assert np.any((xyz[:, 0] < 0) & (xyz[:, 1] == 0) & ~np.signbit(xyz[:, 1])), tag   # antimeridian, y = +0
        assert np.any(r < ai.R) and np.any(r > ai.R + 400e3), tag
