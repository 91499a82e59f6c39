"""
CPU checks of the decorrelation of coloured observation noise: lstsq.whitening_taps against the normals of the reference's
AutoregressiveModelSequence (tests/golden/g27_whitening.npz) and against the inverse Cholesky factor of the process covariance,
lstsq.arc_stages, the Python checks of noise_model= / arcs= before anything reaches the device, and the argument checks of
shg_whiten_rows before any HIP call.
"""
import ctypes

import numpy as np
import pytest

import design_inputs as di
import grates_amd as ga
import los_inputs as li
import whitening_inputs as wi

U = 2.0 ** -53
NAMES = sorted(wi.PROCESSES)


def _sequence(golden, name):
    return wi.sequence(golden('g27_whitening'), name, ga.lstsq)


def test_models_accessor(golden):
    for name in NAMES:
        sequence = _sequence(golden, name)
        p = wi.order(name)
        assert sequence.maximum_order == p and sequence.dimension == 1
        assert isinstance(sequence.models, tuple) and [model.order for model in sequence.models] == list(range(p + 1))
        assert sequence.models[p].white_noise_covariance.shape == (1, 1)


# ---- 1: taps against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_taps_give_the_normals_of_the_reference(golden, name):
    """W^T W of the dense one-arc W against normal_equations(L) of the reference (its upper triangle), L = p + 1 and 12.  An entry is a
    dot product of at most p + 1 products of two taps on either side: summation (p + 1) u sum|a b|, and 3 u sum|a b| for the square
    root, the division and the product behind every term; sum|a b| <= sqrt(N_ii N_jj) <= max|entry| (N is positive definite, so its
    largest entry is on the diagonal).  Both sides together: 2 (p + 1 + 3) u max|entry|."""
    data = golden('g27_whitening')
    p = wi.order(name)
    taps = ga.lstsq.whitening_taps(_sequence(golden, name))
    assert taps.shape == (1, p + 1, p + 1) and taps.dtype == np.float64
    assert np.array_equal(taps[0], np.tril(taps[0])) and np.all(np.diag(taps[0]) != 0) and np.all(taps[0, :, 0] > 0)
    assert np.array_equal(taps[0, :, 0], 1.0 / np.sqrt(data[name + '_Q']))
    for L in (p + 1, wi.LENGTHS):
        stage = ga.lstsq.arc_stages([0], L, p)
        assert stage.dtype == np.int32 and np.array_equal(stage, np.minimum(np.arange(L), p))
        W = wi.dense_filter(taps[0], stage)
        reference = data['{0}_normals{1}'.format(name, L)]
        assert reference.shape == (L, L) and not np.any(np.tril(reference, -1))
        bound = 2 * (p + 1 + 3) * U * np.abs(reference).max()
        err = np.abs(np.triu(W.T @ W) - reference).max()
        print('{0}, L {1}: {2:.2f} of the bound'.format(name, L, err / bound))
        assert err <= bound


# ---- 2: the one-arc W is the inverse Cholesky factor -------------------------------------------------------------------------------
def _levinson(gamma):
    """W [L, L] of the covariance function gamma_0 .. gamma_(L-1) by the Levinson-Durbin recursion in float64: row s holds the
    prediction-error filter of order s over its standard deviation (independent of whitening_taps and of the fixture's models)"""
    L = len(gamma)
    W = np.zeros((L, L))
    phi, variance = np.zeros(0), gamma[0]
    W[0, 0] = 1.0 / np.sqrt(variance)
    for s in range(1, L):
        reflection = (gamma[s] - np.dot(phi, gamma[s - 1:0:-1])) / variance
        phi = np.concatenate((phi - reflection * phi[::-1], [reflection]))
        variance = variance * (1.0 - reflection * reflection)
        W[s, s] = 1.0 / np.sqrt(variance)
        W[s, :s] = -phi[::-1] / np.sqrt(variance)
    return W


# deviation of _levinson from inv(cholesky(Sigma_L)), of max|entry|, measured on the CPU this was written on (the test measures it
# again and allows 10 times what it finds: the two routes differ by the conditioning of Sigma_L only, cond 44 .. 1600)
LEVINSON_DEVIATION = {('ar2', 3): 2.7e-16, ('ar2', 40): 2.5e-15, ('ar5', 3): 1.0e-15, ('ar5', 40): 7.3e-15}      # W itself: 8.1e-16, 3.8e-15, 2.8e-15, 9.4e-15


@pytest.mark.parametrize('L', [3, 40])
@pytest.mark.parametrize('name', NAMES)
def test_one_arc_filter_is_the_inverse_cholesky_factor(golden, name, L):
    """Sigma_L = C C^T, W = C^-1 (lower triangular with a positive diagonal: unique).  L = 3 never reaches the stationary model of
    ar5; at L = 40 the rows from p on are the stationary row (the process is AR(p), so the higher orders add nothing)."""
    p = wi.order(name)
    oracle = np.linalg.inv(np.linalg.cholesky(wi.toeplitz(name, L)))
    scale = np.abs(oracle).max()
    measured = np.abs(_levinson(wi.covariance(name, L)) - oracle).max() / scale
    taps = ga.lstsq.whitening_taps(_sequence(golden, name))
    W = wi.dense_filter(taps[0], ga.lstsq.arc_stages(None, L, p))
    err = np.abs(W - oracle).max() / scale
    print('{0}, L {1}: W {2:.2e}, Levinson {3:.2e} (recorded {4:.1e}) of max|entry|'.format(name, L, err, measured, LEVINSON_DEVIATION[name, L]))
    assert 0.0 < measured <= 10 * LEVINSON_DEVIATION[name, L]
    assert err <= 10 * measured


# ---- 3: stages and the Python checks ---------------------------------------------------------------------------------------------------
def test_arc_stages():
    stage = ga.lstsq.arc_stages([0, 1, 4, 300], 700, 5)
    assert stage.dtype == np.int32 and stage.shape == (700,)
    expected = np.concatenate(([0], [0, 1, 2], np.minimum(np.arange(296), 5), np.minimum(np.arange(400), 5)))
    assert np.array_equal(stage, expected)
    assert np.array_equal(ga.lstsq.arc_stages(np.array([0, 1, 4, 300]), 700, 5), expected)
    assert np.array_equal(ga.lstsq.arc_stages(None, 4, 2), [0, 1, 2, 2]) and np.array_equal(ga.lstsq.arc_stages([0], 4, 0), [0, 0, 0, 0])
    assert np.array_equal(ga.lstsq.arc_stages([0, 699], 700, 128)[-3:], [128, 128, 0])
    assert ga.lstsq.arc_stages(None, 0, 5).shape == (0,)
    for arcs in ([0, 5, 3], [0, 3, 3], [1, 5], [0, 700], [0, 1000], [-1, 5], [], [[0, 5]], [0.5, 2.0]):
        with pytest.raises(ValueError, match='arcs must'):
            ga.lstsq.arc_stages(arcs, 700, 5)
    with pytest.raises(ValueError, match='arcs must'):
        ga.lstsq.arc_stages([0], 0, 5)
    with pytest.raises(ValueError, match='must not be negative'):
        ga.lstsq.arc_stages([0], 5, -1)


def _model(order, variance=1.0, dimension=1):
    return ga.lstsq.AutoregressiveModel([0.1 / (k + 1) * np.eye(dimension) for k in range(order)], variance * np.eye(dimension))


def _plain_sequence(q, **kwargs):
    return ga.lstsq.AutoregressiveModelSequence([_model(s, **kwargs) for s in range(q + 1)])


def test_whitening_taps_checks(golden):
    taps = ga.lstsq.whitening_taps
    two, five = _sequence(golden, 'ar2'), _sequence(golden, 'ar5')
    assert taps([five, _plain_sequence(5), five]).shape == (3, 6, 6)
    assert np.array_equal(taps([five, five])[1], taps(five)[0])
    assert taps(_plain_sequence(0, variance=4.0)).tolist() == [[[0.5]]]
    assert taps(_plain_sequence(128)).shape == (1, 129, 129)
    with pytest.raises(ValueError, match='dimension 2'):
        taps(_plain_sequence(2, dimension=2))
    with pytest.raises(ValueError, match='differ in their maximum order'):
        taps([two, five])
    with pytest.raises(ValueError, match='maximum order 129 of the noise model above 128'):
        taps(_plain_sequence(129))
    for variance in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='not finite and positive'):
            taps(ga.lstsq.AutoregressiveModelSequence([_model(0), _model(1, variance=variance), _model(2)]))
    with pytest.raises(ValueError, match='expected the orders 0, 1, ..., 2'):
        taps(ga.lstsq.AutoregressiveModelSequence([_model(0), _model(2), _model(2)]))
    for bad in (None, 5, [], [five, None], 'ar5'):
        with pytest.raises(ValueError, match='noise_model must be'):
            taps(bad)


def _constructors():
    """components: the from_* call on five valid points under ColouredNoise(noise_model, arcs); 'keywords' (3 components): the
    noise_model= / arcs= keywords of from_accelerations itself"""
    xyz = di.positions()[:5]
    a, b = (x[:5] for x in li.pairs())
    noise = ga.lstsq.ColouredNoise
    return {'keywords': lambda noise_model=None, arcs=None, **kw: ga.lstsq.NormalEquations.from_accelerations(
                xyz, np.ones((5, 3)), 0, 4, noise_model=noise_model, arcs=arcs, **kw),
            3: lambda noise_model, arcs=None, **kw: noise(noise_model, arcs).from_accelerations(xyz, np.ones((5, 3)), 0, 4, **kw),
            4: lambda noise_model, arcs=None, **kw: noise(noise_model, arcs).from_gradients(xyz, np.ones((5, 4)), 0, 4,
                                                                                           components=('xx', 'yy', 'zz', 'xz'), **kw),
            1: lambda noise_model, arcs=None, **kw: noise(noise_model, arcs).from_line_of_sight(a, b, np.ones(5), 0, 4, **kw)}


def test_constructors_check_the_noise_arguments_before_the_device(golden):
    """every ValueError below is raised without a GPU: the checks precede require_gpu (on a machine with a GPU they precede the
    first upload just the same)"""
    two, five = _sequence(golden, 'ar2'), _sequence(golden, 'ar5')
    keywords = _constructors()['keywords']
    with pytest.raises(ValueError, match='arcs are those of the noise model'):
        keywords(arcs=[0])
    with pytest.raises(ValueError, match='arcs are those of the noise model'):
        keywords(arcs=[0, 2], block_points=2)
    with pytest.raises(ValueError, match='noise_model must be'):
        ga.lstsq.ColouredNoise(None, arcs=[0])
    for components, build in _constructors().items():
        components = 3 if components == 'keywords' else components
        with pytest.raises(ValueError, match='arcs must'):
            build(noise_model=five, arcs=[0, 5])
        with pytest.raises(ValueError, match='arcs must'):
            build(noise_model=five, arcs=[1, 2])
        with pytest.raises(ValueError, match='differ in their maximum order'):
            build(noise_model=[two, five])
        with pytest.raises(ValueError, match='dimension 3'):
            build(noise_model=_plain_sequence(1, dimension=3))
        with pytest.raises(ValueError, match='{0} noise models for {1} components'.format(components + 1, components)):
            build(noise_model=[two] * (components + 1))
    for values in (np.ones(5), np.ones((5, 3))):
        with pytest.raises(ValueError, match='arcs must'):
            ga.lstsq.decorrelate(values, five, arcs=[0, 7])
    with pytest.raises(ValueError, match='2 noise models for 3 components'):
        ga.lstsq.decorrelate(np.ones((5, 3)), [two, two])
    with pytest.raises(ValueError, match=r'values must have shape \(M,\) or \(M, K\)'):
        ga.lstsq.decorrelate(np.ones((5, 3, 1)), two)


def test_constructor_signatures():
    import inspect
    parameters = list(inspect.signature(ga.lstsq.NormalEquations.from_accelerations).parameters.values())
    assert [prm.name for prm in parameters[-3:]] == ['block_points', 'noise_model', 'arcs'] and all(prm.default is None for prm in parameters[-3:])
    assert list(inspect.signature(ga.lstsq.ColouredNoise).parameters) == ['noise_model', 'arcs']
    for name in ('from_accelerations', 'from_gradients', 'from_line_of_sight'):             # the arguments of the classmethod of the same name
        bound = [(prm.name, prm.default) for prm in list(inspect.signature(getattr(ga.lstsq.ColouredNoise, name)).parameters.values())[1:]]
        plain = [(prm.name, prm.default) for prm in inspect.signature(getattr(ga.lstsq.NormalEquations, name)).parameters.values()]
        assert bound == [item for item in plain if item[0] not in ('noise_model', 'arcs')]
    assert list(inspect.signature(ga.engine.whiten_rows).parameters)[:5] == ['X', 'taps', 'stage', 'channels', 'skip']
    assert list(inspect.signature(ga.lstsq.decorrelate).parameters) == ['values', 'noise_model', 'arcs']


# ---- 4: the C entry point ---------------------------------------------------------------------------------------------------------------
def test_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    call = lib.shg_whiten_rows
    X, Y, stage, taps = (ctypes.c_void_p(address) for address in (0x10000000, 0x20000000, 0x30000000, 0x30010000))   # never dereferenced

    def error():
        return lib.shg_last_error().decode()
    #    rows channels M  X  ldx stage taps q skip Y ldy stream
    for rows, M, ldx, ldy in ((-1, 10, 10, 10), (6, -1, 10, 10), (6, 10, -1, 10), (6, 10, 10, -1)):
        assert call(rows, 3, M, X, ldx, stage, taps, 5, 0, Y, ldy, None) == -1
        assert 'shg_whiten_rows: negative size' in error()
    for channels in (0, -3):
        assert call(6, channels, 10, X, 10, stage, taps, 5, 0, Y, 10, None) == -1
        assert 'channels {0} below 1'.format(channels) in error()
    assert call(7, 3, 10, X, 10, stage, taps, 5, 0, Y, 10, None) == -1
    assert 'rows 7 are not a multiple of channels 3' in error()
    for q in (-1, 129):
        assert call(6, 3, 10, X, 10, stage, taps, q, 0, Y, 10, None) == -1
        assert 'order q {0} outside 0 .. 128'.format(q) in error()
    for skip in (-1, 11):
        assert call(6, 3, 10, X, 10, stage, taps, 5, skip, Y, 10, None) == -1
        assert 'skip {0} outside 0 .. M 10'.format(skip) in error()
    assert call(6, 3, 10, X, 9, stage, taps, 5, 0, Y, 10, None) == -1
    assert 'ldx 9 below M 10' in error()
    assert call(6, 3, 10, X, 10, stage, taps, 5, 4, Y, 5, None) == -1
    assert 'ldy 5 below M - skip 6' in error()
    for pointers in ((None, stage, taps, Y), (X, None, taps, Y), (X, stage, None, Y), (X, stage, taps, None)):
        assert call(6, 3, 10, pointers[0], 10, pointers[1], pointers[2], 5, 0, pointers[3], 10, None) == -1
        assert 'shg_whiten_rows: NULL pointer' in error()
    assert call((1 << 20) + 1, 1, 1 << 20, X, 1 << 20, stage, taps, 5, 0, Y, 1 << 20, None) == -1         # 2^40 + 2^20 values
    assert 'are too large' in error()
    assert call(1 << 20, 1, 4, X, 4, stage, taps, 5, 0, Y, (1 << 20) + 1, None) == -1                      # ... of Y alone
    assert 'are too large' in error()
    # X [6][704] with 700 columns in use and Y [6][704]: the ranges end 8 (5 * 704 + 700) bytes after their first address
    base, span = 0x10000000, 8 * (5 * 704 + 700)
    for y in (base, base + 8, base + span - 8, base - span + 8, base + 8 * 704):
        assert call(6, 3, 700, ctypes.c_void_p(base), 704, stage, taps, 5, 0, ctypes.c_void_p(y), 704, None) == -1, hex(y)
        assert 'X and Y overlap' in error()
    # Y starts 5 columns into X and is written from column 5 on (skip = 5): in place in all but name
    assert call(6, 3, 700, ctypes.c_void_p(base), 704, stage, taps, 5, 5, ctypes.c_void_p(base + 40), 704, None) == -1
    assert 'X and Y overlap' in error()
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(0, 3, 10, None, 10, None, None, 5, 0, None, 10, None) == 0
    assert call(6, 3, 10, None, 10, None, None, 5, 10, None, 0, None) == 0
    assert call(6, 3, 0, None, 0, None, None, 0, 0, None, 0, None) == 0
    with pytest.raises(_lib.ShgError, match='rows 7 are not a multiple of channels 3'):
        _lib.call('shg_whiten_rows', 7, 3, 10, X, 10, stage, taps, 5, 0, Y, 10, None)
