"""
CPU checks of the gravitational gradient tensor at points: the two C entry points reject bad arguments before any HIP call, the Python
methods reject bad position shapes before anything reaches the device, and the fixture g23_gradients.npz checks itself (closed form of
a point mass, symmetry and trace, central differences of the host acceleration).
"""
import ctypes

import numpy as np
import pytest

import gradient_inputs as gi
import grates_amd as ga

ENTRY = 'shg_gravitational_gradients_points'
ENTRY_OM = 'shg_gravitational_gradients_points_om'


def _error(lib):
    return lib.shg_last_error().decode()


def test_gradient_entry_points_reject_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, ENTRY)
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    GM, R = gi.GM, gi.R
    for N, M, B in ((-1, 10, 1), (4, -1, 1), (4, 10, -2)):
        assert fn(N, dummy, M, 0, dummy, B, GM, R, dummy, None) == -1
        assert ENTRY + ': negative size' in _error(lib)
    for layout in (-1, 2):
        assert fn(4, dummy, 10, layout, dummy, 1, GM, R, dummy, None) == -1
        assert 'layout {0}, expected 0 (shared points) or 1 (points per epoch)'.format(layout) in _error(lib)
    for gm, r in ((float('nan'), R), (float('inf'), R), (GM, 0.0), (GM, -R), (GM, float('inf')), (GM, float('nan'))):
        assert fn(4, dummy, 10, 0, dummy, 1, gm, r, dummy, None) == -1
        assert 'GM and R must be finite and R positive' in _error(lib)
    for xyz, anm, T in ((None, dummy, dummy), (dummy, None, dummy), (dummy, dummy, None)):
        assert fn(4, xyz, 10, 1, anm, 3, GM, R, T, None) == -1
        assert ENTRY + ': NULL pointer' in _error(lib)
    assert fn(4, dummy, 1 << 29, 0, dummy, 1 << 12, GM, R, dummy, None) == -1
    assert 'output of {0} values is too large'.format(9 * (1 << 29) * (1 << 12)) in _error(lib)
    assert fn(10000, dummy, 10, 0, dummy, 1, GM, R, dummy, None) == -1     # one pass of Q: 48 * 10003 * 10004 / 2 values > 2^31 - 1
    assert 'degree 10000 is too large' in _error(lib)
    # nothing to do: no pointer is looked at and no HIP call is made
    assert fn(4, None, 0, 0, None, 3, GM, R, None, None) == 0
    assert fn(4, None, 10, 1, None, 0, GM, R, None, None) == 0
    assert fn(9000, None, 0, 0, None, 3, GM, R, None, None) == 0


def test_gradient_om_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)
    GM, R = gi.GM, gi.R
    with pytest.raises(_lib.ShgError, match=ENTRY_OM + ': negative size'):
        _lib.call(ENTRY_OM, 4, dummy, -1, 0, dummy, 4, 4, GM, R, dummy, None)
    with pytest.raises(_lib.ShgError, match='Bpad 3 below B 4'):
        _lib.call(ENTRY_OM, 4, dummy, 10, 0, dummy, 4, 3, GM, R, dummy, None)
    with pytest.raises(_lib.ShgError, match=ENTRY_OM + ': NULL pointer'):
        _lib.call(ENTRY_OM, 4, dummy, 10, 0, None, 4, 32, GM, R, dummy, None)
    with pytest.raises(_lib.ShgError, match=ENTRY_OM + ': layout 5'):
        _lib.call(ENTRY_OM, 4, dummy, 10, 5, dummy, 4, 32, GM, R, dummy, None)
    with pytest.raises(_lib.ShgError, match='GM and R must be finite and R positive'):
        _lib.call(ENTRY_OM, 4, dummy, 10, 0, dummy, 4, 32, GM, float('nan'), dummy, None)
    with pytest.raises(_lib.ShgError, match='is too large'):
        _lib.call(ENTRY_OM, 4, dummy, 1 << 29, 0, dummy, 1 << 12, 1 << 12, GM, R, dummy, None)
    assert getattr(lib, ENTRY_OM)(4, None, 0, 0, None, 4, 4, GM, R, None, None) == 0
    assert getattr(lib, ENTRY_OM)(4, None, 10, 0, None, 0, 0, GM, R, None, None) == 0


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
    for shape in ((5,), (5, 2), (5, 4), (2, 5, 3), (3,)):
        for as_tensor in (False, True):
            with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
                gf.gravitational_gradients(np.zeros(shape), as_tensor=as_tensor)
    series = _series(3)
    for shape in ((5,), (5, 2), (2, 5, 3), (4, 5, 3), (3, 5, 2), (1, 3, 5, 3)):
        for as_tensor in (False, True):
            with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\) or \(3, M, 3\)'):
                series.gravitational_gradients(np.zeros(shape), as_tensor=as_tensor)


def test_fixture_cases_cover_the_special_positions(golden):
    data = golden('g23_gradients')
    for tag in gi.CASES:
        xyz, T = data['xyz_' + tag], data['T_' + tag]
        assert T.shape == (xyz.shape[0], 3, 3) and np.all(np.isfinite(T)), tag
        r = np.sqrt(np.sum(xyz ** 2, axis=1))
        assert np.any((xyz[:, 0] == 0) & (xyz[:, 1] == 0)), tag                         # exact poles
        assert np.any((xyz[:, 0] < 0) & (xyz[:, 1] == 0) & np.signbit(xyz[:, 1])), tag    # antimeridian, y = -0
        assert np.any((xyz[:, 0] < 0) & (xyz[:, 1] == 0) & ~np.signbit(xyz[:, 1])), tag   # antimeridian, y = +0
        assert np.any((xyz[:, 2] == 0) & (xyz[:, 0] > 0)), tag                          # equator
        assert np.any(r < gi.R) and np.any(r > gi.R + 400e3), tag
        assert np.array_equal(xyz, gi.positions(tag)), tag                              # the fixture's positions are the seeded ones


def test_fixture_point_mass_closed_form(golden):
    data = golden('g23_gradients')
    xyz, T = data['xyz_point_mass'], data['T_point_mass']
    ref = gi.point_mass_tensor(xyz)
    err = np.abs(T - ref).max() / np.abs(ref).max()
    assert err <= 1e-14, err


@pytest.mark.parametrize('tag', list(gi.CASES))
def test_fixture_symmetric_and_trace_free(golden, tag):
    T = golden('g23_gradients')['T_' + tag]
    scale = np.abs(T).max()
    assert np.abs(T - T.transpose(0, 2, 1)).max() == 0.0                            # off-diagonals are stored twice
    assert np.abs(np.trace(T, axis1=1, axis2=2)).max() <= 1e-14 * scale              # Laplace's equation outside the masses


def _host_field(tag):
    N, kind, seed, _ = gi.CASES[tag]
    gf = ga.gravityfield.PotentialCoefficients(gi.GM, gi.R)
    gf.anm = gi.coefficients(N, kind, seed)
    return gf


@pytest.mark.parametrize('tag', [t for t in gi.CASES if gi.CASES[t][0] <= 60])
def test_fixture_matches_differences_of_host_acceleration(golden, tag):
    """4th-order central differences of the host acceleration at h = 4 km.  Truncation: h^4 / 30 |g^(5)|, with |g^(5)| ~ 5! |T| / r^4
    for degree 0: 4 (h / r)^4 ~ 5e-13 of max|T|; degree 60 (at most 1e-6 of max|T|) adds (60 h / r)^4 ~ 1e-6 of that.  Rounding:
    a few 1e-16 of |g| / h ~ 1e-12 of max|T|.  The host path forms s = sqrt(1 - t^2): near the poles s has a relative error of about
    1e-16 / colatitude^2, which the steps off the axis turn into 2e-11 of max|T| at 4 km (and 1e-9 at 1 km, hence the large step);
    within 1.5e-8 rad of the axis s is 0 and g_x vanishes, so at the point 1 mm off the pole T_xz = 3 GM x z / r^5 (2.3e-10 of
    max|T|) is missed.  Hence 1e-9."""
    data = golden('g23_gradients')
    xyz, ref = data['xyz_' + tag], data['T_' + tag]
    gf = _host_field(tag)
    h = 4e3
    T = np.empty_like(ref)
    for d in range(3):
        e = np.zeros(3)
        e[d] = h
        g = [gf.gravitational_acceleration(xyz + s * e) for s in (-2, -1, 1, 2)]
        T[:, :, d] = (g[0] - 8 * g[1] + 8 * g[2] - g[3]) / (12 * h)
    err = np.abs(T - ref).max() / np.abs(ref).max()
    assert err <= 1e-9, '{0}: {1:.3e} of max|T|'.format(tag, err)
