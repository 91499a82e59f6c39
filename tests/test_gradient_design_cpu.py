"""
CPU checks of the gradient-tensor design matrix and of NormalEquations.from_gradients: both C entry points reject bad arguments
before any HIP call, the host-only table of shg_gradient_design_terms reproduces the mp-oracle fixture g25_gradient_design.npz when it
is evaluated in NumPy, and the Python functions reject bad shapes, components, frames, weights and degrees before anything reaches
the device.
"""
import ctypes
import inspect

import numpy as np
import pytest

import gradient_design_inputs as gdi
import grates_amd as ga

GM, R = gdi.GM, gdi.R


def _error(lib):
    return lib.shg_last_error().decode()


def _tolerance(data):
    """5e-14 of max|A| (the bound of the acceleration's design matrix) while the recorded restatement error leaves it a factor of
    four; otherwise four times the recorded value"""
    recorded = float(data['restatement_err'])
    return 5e-14 if recorded <= 5e-14 / 4 else 4 * recorded


def _terms(N, min_degree):
    from grates_amd import _lib
    P = gdi.parameter_count(min_degree, N)
    slot, factor = np.full((P, 6, 4), 7, dtype=np.int32), np.full((P, 6, 4), np.nan)
    _lib.call('shg_gradient_design_terms', N, min_degree, slot.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_void_p(factor.ctypes.data),
              slot.size)
    return slot, factor


def test_design_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    call = lib.shg_gradient_design
    for N, nmin, M in ((-1, 0, 10), (4, -1, 10), (4, 0, -1)):
        assert call(N, nmin, dummy, M, None, 63, None, 0, GM, R, dummy, max(M, 0), None) == -1
        assert 'shg_gradient_design: negative size' in _error(lib)
    assert call(4, 5, dummy, 10, None, 63, None, 0, GM, R, dummy, 10, None) == -1
    assert 'min_degree 5 above N 4' in _error(lib)
    assert call(32766, 0, dummy, 10, None, 63, None, 0, GM, R, dummy, 10, None) == -1
    assert 'N 32766 is too large' in _error(lib)
    for components in (0, 64, -1, 127):
        assert call(4, 0, dummy, 10, None, components, None, 0, GM, R, dummy, 10, None) == -1
        assert 'components {0}, expected a set of SHG_GRAD_XX ... SHG_GRAD_ZZ (1 .. 63)'.format(components) in _error(lib)
    for layout in (-1, 3):
        assert call(4, 0, dummy, 10, None, 63, dummy, layout, GM, R, dummy, 10, None) == -1
        assert 'weight layout {0}, expected 0 (none), 1 (per point) or 2 (per component)'.format(layout) in _error(lib)
    for gm, r in ((float('nan'), R), (GM, 0.0), (GM, -R), (GM, float('inf'))):
        assert call(4, 0, dummy, 10, None, 63, None, 0, gm, r, dummy, 10, None) == -1
        assert 'GM and R must be finite and R positive' in _error(lib)
    assert call(4, 0, dummy, 10, None, 63, None, 0, GM, R, dummy, 9, None) == -1
    assert 'ldt 9 below M 10' in _error(lib)
    for xyz, w, layout, At in ((None, None, 0, dummy), (dummy, None, 0, None), (dummy, None, 1, dummy), (dummy, None, 2, dummy)):
        assert call(4, 0, xyz, 10, dummy, 9, w, layout, GM, R, At, 10, None) == -1
        assert 'shg_gradient_design: NULL pointer' in _error(lib)
    # 2^40 values: 4e6 rows x K x 2^20 points is too large for every K; 1024 rows x 2^30 points only from K = 2 on
    assert call(2000, 0, dummy, 1 << 20, None, 32, None, 0, GM, R, dummy, 1 << 20, None) == -1
    assert 'is too large' in _error(lib)
    assert call(31, 0, dummy, 1 << 30, None, 3, None, 0, GM, R, dummy, 1 << 30, None) == -1
    assert 'output of 1024 x 2 x 1073741824 values is too large' in _error(lib)
    assert call(32765, 0, dummy, 1 << 30, None, 63, None, 0, GM, R, dummy, (1 << 31) - 1, None) == -1       # no overflow of the product
    assert 'is too large' in _error(lib)
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(4, 2, None, 0, None, 63, None, 0, GM, R, None, 0, None) == 0
    assert call(4, 2, None, 0, None, 1, None, 2, GM, R, None, 5, None) == 0
    with pytest.raises(_lib.ShgError, match='min_degree 3 above N 2'):
        _lib.call('shg_gradient_design', 2, 3, dummy, 10, None, 63, None, 0, GM, R, dummy, 10, None)


def test_terms_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    slot, factor = np.zeros(24 * 9, dtype=np.int32), np.zeros(24 * 9)
    sp, fp = slot.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_void_p(factor.ctypes.data)
    call = lib.shg_gradient_design_terms
    for N, nmin in ((-1, 0), (2, -1)):
        assert call(N, nmin, sp, fp, 216) == -1
        assert 'shg_gradient_design_terms: negative size' in _error(lib)
    assert call(2, 3, sp, fp, 216) == -1
    assert 'min_degree 3 above N 2' in _error(lib)
    assert call(32766, 32766, sp, fp, 1 << 40) == -1
    assert 'N 32766 is too large' in _error(lib)
    assert call(2, 0, sp, fp, 215) == -1
    assert 'capacity 215 below the 216 entries of the table' in _error(lib)
    for s, f in ((None, fp), (sp, None)):
        assert call(2, 0, s, f, 216) == -1
        assert 'shg_gradient_design_terms: NULL pointer' in _error(lib)
    assert not slot.any() and not factor.any()           # nothing was written by the refused calls
    assert call(2, 0, sp, fp, 216) == 0 and call(2, 2, sp, fp, 216) == 0 and call(2, 2, sp, fp, 120) == 0


@pytest.mark.parametrize('N,min_degree', [(8, 0), (8, 2), (2, 0), (0, 0)])
def test_terms_reproduce_the_fixture(golden, N, min_degree):
    data = golden('g25_gradient_design')
    xyz = data['xyz']
    # a column does not depend on the other columns: (N, min_degree) is a column slice of the d/o 8 (or d/o 2) matrix
    ref = data['A8' if N == 8 else 'A2'][:, min_degree ** 2:(N + 1) ** 2]
    slot, factor = _terms(N, min_degree)
    P = gdi.parameter_count(min_degree, N)
    assert slot.shape == (P, 6, 4) and np.all(np.isfinite(factor))
    present = slot >= 0
    assert np.all((slot == -1) | present) and np.all(factor[~present] == 0.0)
    assert present.sum(axis=2).max() <= 4 and np.all(present[:, 5].sum(axis=1) == 1)                  # zz is one term
    N2 = N + 2
    assert slot.max() < (N2 + 1) * (N2 + 2)                                                          # 2 packed_count(N + 2)
    for row in range(P):                                                                             # merged: no slot twice in an entry
        for comp in range(6):
            used = slot[row, comp][present[row, comp]]
            assert len(set(used.tolist())) == used.size
            assert np.all(present[row, comp][:used.size])                                            # terms first, then the -1 entries
    A = gdi.evaluate_table(slot, factor, gdi.solid_harmonics(xyz, N2))
    assert A.shape == ref.shape
    err = np.abs(A - ref).max() / np.abs(ref).max()
    print('d/o {0} from {1}: table on the restated harmonics {2:.2e} of max|A|'.format(N, min_degree, err))
    assert err <= _tolerance(data)
    trace = A.reshape(-1, 6, P)[:, [0, 3, 5]].sum(axis=1)
    print('trace: {0:.2e} of max|A|'.format(np.abs(trace).max() / np.abs(A).max()))
    assert np.abs(trace).max() <= 1e-13 * np.abs(A).max()
    if min_degree:                                                                                   # min_degree is a row slice
        slot0, factor0 = _terms(N, 0)
        assert np.array_equal(slot, slot0[min_degree ** 2:]) and np.array_equal(factor, factor0[min_degree ** 2:])


def test_terms_match_the_python_table():
    """the restatement's own table holds the same terms (as sets per entry: the order of merged terms is the builder's)"""
    for N, min_degree in ((8, 0), (5, 3), (0, 0)):
        slot, factor = _terms(N, min_degree)
        pslot, pfactor = gdi.table(min_degree, N)
        for row in range(slot.shape[0]):
            for comp in range(6):
                got = {int(s): f for s, f in zip(slot[row, comp], factor[row, comp]) if s >= 0}
                expected = {int(s): f for s, f in zip(pslot[row, comp], pfactor[row, comp]) if s >= 0}
                assert got.keys() == expected.keys()
                for s in got:
                    assert abs(got[s] - expected[s]) <= 4e-16 * abs(expected[s]) + 1e-300, (row, comp, s)


def test_fixture_is_consistent(golden):
    data = golden('g25_gradient_design')
    xyz, frames = data['xyz'], data['frames']
    assert np.array_equal(xyz, gdi.positions()) and xyz.shape == (20, 3)
    assert np.array_equal(frames, gdi.frames(20)) and np.array_equal(frames[0], np.eye(3))
    assert np.abs(np.einsum('iac,ibc->iab', frames, frames) - np.eye(3)).max() <= 1e-14
    assert np.all(np.abs(np.linalg.det(frames) - 1.0) <= 1e-14)
    worst = 0.0
    for N in gdi.DEGREES:
        A = data['A{0}'.format(N)]
        assert A.shape == (120, (N + 1) ** 2) and np.all(np.isfinite(A))
        worst = max(worst, np.abs(gdi.restatement(xyz, 0, N) - A).max() / np.abs(A).max())
        assert np.array_equal(gdi.restatement(xyz, 2, N), gdi.restatement(xyz, 0, N)[:, 4:])
        trace = A.reshape(20, 6, -1)[:, [0, 3, 5]].sum(axis=1)
        assert np.abs(trace).max() <= 1e-13 * np.abs(A).max()
    assert np.array_equal(data['A2'], data['A8'][:, :9])                                  # a column does not depend on N
    assert worst <= 2 * float(data['restatement_err']) and float(data['restatement_err']) <= 5e-14 / 4
    assert float(data['ax_err']) <= 1e-13 / 4
    for name in gdi.LOOP_SETS:
        assert float(data['host_rel_err_' + name]) <= 1e-8 and float(data['loop_cond_' + name]) <= 1e4
    # the rotation helper: identity frames and the Earth-fixed rows, a subset and its rows of the full set
    A = data['A2']
    assert np.array_equal(gdi.rotate_rows(A), A)
    assert np.array_equal(gdi.rotate_rows(A, np.tile(np.eye(3), (20, 1, 1))), A)
    rotated = gdi.rotate_rows(A, frames)
    assert np.array_equal(gdi.rotate_rows(A, frames, ('zz', 'xx')), rotated.reshape(20, 6, -1)[:, [0, 5]].reshape(40, -1))
    trace = rotated.reshape(20, 6, -1)[:, [0, 3, 5]].sum(axis=1)                          # the trace is invariant
    assert np.abs(trace).max() <= 1e-13 * np.abs(A).max()


BAD_SHAPES = ((5,), (5, 2), (5, 4), (2, 5, 3))


def test_signatures():
    def names(function):
        return list(inspect.signature(function).parameters)
    assert names(ga.engine.gradient_design) == ['max_degree', 'xyz', 'GM', 'R', 'min_degree', 'frames', 'components', 'weights']
    assert names(ga.gravityfield.gradient_design_matrix) == ['xyz', 'min_degree', 'max_degree', 'GM', 'R', 'frames', 'components', 'weights',
                                                              'as_tensor']
    assert names(ga.lstsq.NormalEquations.from_gradients) == ['xyz', 'gradients', 'min_degree', 'max_degree', 'GM', 'R', 'frames', 'components',
                                                              'weights', 'block_points']
    reference = inspect.signature(ga.gravityfield.acceleration_design_matrix).parameters
    for function in (ga.gravityfield.gradient_design_matrix, ga.lstsq.NormalEquations.from_gradients):
        parameters = inspect.signature(function).parameters
        assert parameters['GM'].default == reference['GM'].default and parameters['R'].default == reference['R'].default
    assert ga.engine.GRADIENT_COMPONENTS == gdi.COMPONENTS
    # the weight check keeps its results for the acceleration's callers
    assert names(ga.engine.check_observation_weights)[:2] == ['weights', 'points']
    assert ga.engine.check_observation_weights(np.ones((5, 3)), 5) == 2 and ga.engine.check_observation_weights(np.ones(5), 5) == 1
    assert ga.engine.check_observation_weights(None, 5) == 0
    with pytest.raises(ValueError, match=r'weights must have shape \(5,\) or \(5, 3\)'):
        ga.engine.check_observation_weights(np.ones((5, 4)), 5)


def test_components_are_parsed():
    parse = ga.engine.gradient_components
    assert parse(None) == [0, 1, 2, 3, 4, 5]
    assert parse(('xz', 'zz', 'xx', 'yy')) == [0, 2, 3, 5] and parse(['xy']) == [1] and parse('zz') == [5]
    with pytest.raises(ValueError, match="unknown gradient component 'yx'"):
        parse(('xx', 'yx'))
    with pytest.raises(ValueError, match='gradient components must be distinct'):
        parse(('xx', 'zz', 'xx'))
    with pytest.raises(ValueError, match='at least one gradient component'):
        parse(())


def test_design_matrix_python_checks():
    design = ga.gravityfield.gradient_design_matrix
    for shape in BAD_SHAPES:
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
            design(np.zeros(shape), 0, 4)
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
            ga.engine.gradient_design(4, np.zeros(shape), GM, R)
    xyz = gdi.positions()[:5]
    with pytest.raises(ValueError, match='min_degree 5 must lie between 0 and max_degree 4'):
        design(xyz, 5, 4)
    with pytest.raises(ValueError, match='min_degree -1'):
        design(xyz, -1, 4)
    with pytest.raises(ValueError, match="unknown gradient component 'zx'"):
        design(xyz, 0, 4, components=('zx',))
    with pytest.raises(ValueError, match='gradient components must be distinct'):
        design(xyz, 0, 4, components=('zz', 'zz'))
    for shape in ((4,), (5, 2), (5, 3), (5, 6, 1), (6, 5), ()):
        with pytest.raises(ValueError, match=r'weights must have shape \(5,\) or \(5, 6\)'):
            design(xyz, 0, 4, weights=np.ones(shape))
    with pytest.raises(ValueError, match=r'weights must have shape \(5,\) or \(5, 4\)'):
        design(xyz, 0, 4, components=('xx', 'yy', 'zz', 'xz'), weights=np.ones((5, 6)))
    for bad in (-1.0, np.nan, np.inf):
        for shape in ((5,), (5, 6)):
            w = np.ones(shape)
            w[2] = bad
            with pytest.raises(ValueError, match='weights must be finite and not negative'):
                design(xyz, 0, 4, weights=w)
    frames = gdi.frames(5)
    for shape in ((5, 3), (4, 3, 3), (5, 9), (3, 3)):
        with pytest.raises(ValueError, match=r'frames must have shape \(5, 3, 3\)'):
            design(xyz, 0, 4, frames=np.zeros(shape))
    for defect in (1e-11, 1e-3):
        bad = frames.copy()
        bad[3, 1] *= 1.0 + defect                                                       # row 1 is no longer of unit length
        with pytest.raises(ValueError, match='frames must have orthonormal rows'):
            design(xyz, 0, 4, frames=bad)
    bad = frames.copy()
    bad[2, 0, 0] = np.nan
    with pytest.raises(ValueError, match='frames must have orthonormal rows'):
        design(xyz, 0, 4, frames=bad)
    ga.engine.check_frames(frames, 5)                                                    # seeded rotations pass
    skewed = frames.copy()
    skewed[4, 2] += 1e-14 * skewed[4, 0]                                                 # within the tolerance
    ga.engine.check_frames(skewed, 5)


def test_from_gradients_python_checks():
    build = ga.lstsq.NormalEquations.from_gradients
    good, obs = np.ones((5, 3)), np.ones((5, 6))
    for shape in BAD_SHAPES:
        with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
            build(np.zeros(shape), obs, 0, 4)
    for shape in ((5,), (5, 5), (5, 3), (5, 3, 2), (5, 2, 3, 3)):
        with pytest.raises(ValueError, match=r'gradients must have shape \(M, 6\) or \(M, 3, 3\)'):
            build(good, np.zeros(shape), 0, 4)
    with pytest.raises(ValueError, match=r'gradients must have shape \(M, 4\) or \(M, 3, 3\)'):
        build(good, obs, 0, 4, components=('xx', 'yy', 'zz', 'xz'))
    for other in (np.ones((6, 6)), np.ones((6, 3, 3))):
        with pytest.raises(ValueError, match='5 positions but 6 gradients'):
            build(good, other, 0, 4)
    with pytest.raises(ValueError, match='min_degree 5 must lie between 0 and max_degree 4'):
        build(good, obs, 5, 4)
    with pytest.raises(ValueError, match='gradient components must be distinct'):
        build(good, obs, 0, 4, components=('xx', 'xx'))
    with pytest.raises(ValueError, match=r'weights must have shape \(5,\) or \(5, 6\)'):
        build(good, obs, 0, 4, weights=np.ones((5, 3)))
    with pytest.raises(ValueError, match='weights must be finite and not negative'):
        build(good, obs, 0, 4, weights=np.array([1.0, 1.0, -0.5, 1.0, 1.0]))
    with pytest.raises(ValueError, match=r'frames must have shape \(5, 3, 3\)'):
        build(good, obs, 0, 4, frames=np.zeros((5, 3)))
    with pytest.raises(ValueError, match='frames must have orthonormal rows'):
        build(good, obs, 0, 4, frames=np.ones((5, 3, 3)))
    with pytest.raises(ValueError, match='block_points must be positive'):
        build(good, obs, 0, 4, block_points=0)


def test_default_block_is_a_multiple_of_256_within_the_budget():
    """the rule of from_gradients' default block_points, restated: At [P, K Mb] of a block stays within DESIGN_BLOCK_BYTES"""
    budget = ga.lstsq.NormalEquations.DESIGN_BLOCK_BYTES
    for N, nmin, K, expected in ((96, 2, 6, 512), (96, 2, 4, 768), (60, 2, 6, 1280), (8, 2, 4, 108800), (720, 0, 6, 256)):
        P = gdi.parameter_count(nmin, N)
        block = max(budget // (8 * K * P) // 256 * 256, 256)
        assert block == expected and block % 256 == 0
        assert block == 256 or (8 * K * P * block <= budget < 8 * K * P * (block + 256))
