"""
CPU checks of vector noise models: lstsq.VectorNoise.taps against the inverse Cholesky factor of the block
Toeplitz covariance of known VAR processes (which settles the transpose convention of the lags), its ValueErrors and those of the
routing through every constructor before anything reaches the device, lstsq.component_basis, and the argument checks of
shg_whiten_rows_vector and shg_segment_cross_lag_products before any HIP call.
"""
import ctypes

import numpy as np
import pytest

import design_inputs as di
import grates_amd as ga
import los_inputs as li
import vector_noise_reference as vr

ARCS, L = [0, 1, 4, 30], 40


# ---- 1: the filter whitens the process ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K, q', [(3, 2), (2, 2), (6, 2), (3, 4)])
def test_filter_whitens_every_arc(K, q):
    """W_a Sigma_La W_a^T = I for every arc, W dense from taps() and arc_stages.  The tolerance is measured, not fixed: the same product
    with W = inv(cholesky(Sigma_La)) of numpy.linalg deviates from I by its own rounding, and 10 times that is allowed.  With
    Sigma_k = E[x_t x_(t-k)^T] in place of E[x_t x_(t+k)^T] the deviation is of order 1: this test settles the convention."""
    B1, B2, Q = vr.process(K)
    Sigma = vr.covariance_function([B1, B2], Q, max(q, L))
    noise = ga.lstsq.VectorNoise(vr.sequence(ga.lstsq, Sigma, q))
    assert noise.dimension == K and noise.maximum_order == q
    taps = noise.taps()
    assert taps.shape == (q + 1, q + 1, K, K) and taps.dtype == np.float64
    for s in range(q + 1):
        assert np.array_equal(taps[s, 0], np.tril(taps[s, 0])) and np.all(np.diag(taps[s, 0]) > 0) and not np.any(taps[s, s + 1:])
    stage = ga.lstsq.arc_stages(ARCS, L, q)
    W = vr.dense_filter(taps, stage)
    assert not np.any(np.triu(W, 1)[np.triu(np.ones_like(W), K) > 0])                       # block lower triangular
    bounds = ARCS + [L]
    for a in range(len(ARCS)):
        rows = slice(bounds[a] * K, bounds[a + 1] * K)
        assert not np.any(W[rows, :bounds[a] * K])                                          # nothing crosses the start of an arc
        Wa, cov = W[rows, rows], vr.block_toeplitz(Sigma, bounds[a + 1] - bounds[a])
        oracle = np.linalg.inv(np.linalg.cholesky(cov))
        eye = np.eye(cov.shape[0])
        measured, err = np.abs(oracle @ cov @ oracle.T - eye).max(), np.abs(Wa @ cov @ Wa.T - eye).max()
        print('K {0}, q {1}, arc of {2}: W {3:.2e}, inv(cholesky) {4:.2e}'.format(K, q, bounds[a + 1] - bounds[a], err, measured))
        assert measured > 0.0 and err <= 10 * measured
        flipped = vr.block_toeplitz([lag.T for lag in Sigma], bounds[a + 1] - bounds[a])
        if bounds[a + 1] - bounds[a] > 1:
            assert np.abs(Wa @ flipped @ Wa.T - eye).max() > 1e-3                           # the other convention does not whiten


def test_taps_give_the_normals_of_the_reference(golden):
    """W^T W of the dense one-arc W against normal_equations(L) of the reference's sequence of the K = 3 process (its upper blocks,
    tests/golden/g35_vector_noise.npz), L = 3 and 12, from the models the reference formed.  An entry is a dot product of at most
    K (p + 1) products of two taps on either side.  A tap is an entry of R^-T or of R^-T B: a triangular solve and a product of K
    terms, 2 K u cond(R) |R^-T| |B| of relative error norm-wise, on both factors of a product and on both sides of the comparison,
    beside the K (p + 1) u of the summation; cond(R) = sqrt(cond(Q_s)) at most.  sum |a b| <= max|entry| as in
    tests/test_whitening_cpu.py (N is positive definite): 2 (K (p + 1) + 4 K cond(R)) u max|entry|."""
    data = golden('g35_vector_noise')
    K, p = 3, 2
    B1, B2, Q = vr.process(K)
    assert np.array_equal(data['covariance'], np.array(vr.covariance_function([B1, B2], Q, p)))           # the fixture is of this process
    models = [ga.lstsq.AutoregressiveModel([data['coefficients'][s, k] for k in range(s)], data['Q'][s]) for s in range(p + 1)]
    taps = ga.lstsq.VectorNoise(ga.lstsq.AutoregressiveModelSequence(models)).taps()
    cond = max(np.sqrt(np.linalg.cond(data['Q'][s])) for s in range(p + 1))
    for L in (3, 12):
        W = vr.dense_filter(taps, ga.lstsq.arc_stages([0], L, p))
        reference = data['normals{0}'.format(L)]
        upper = np.arange(K * L)[:, None] // K <= np.arange(K * L)[None, :] // K                         # the reference keeps the upper blocks, whole
        assert reference.shape == (K * L, K * L) and not np.any(reference[~upper])
        bound = 2 * (K * (p + 1) + 4 * K * cond) * vr.U * np.abs(reference).max()
        err = np.abs(np.where(upper, W.T @ W, 0.0) - reference).max()
        print('L {0}: {1:.3f} of the bound (cond(R) {2:.1f})'.format(L, err / bound, cond))
        assert err <= bound
    # the NumPy Yule-Walker solve of the helpers gives the reference's models
    for s in range(p + 1):
        B, Qs = vr.yule_walker(list(data['covariance']), s)
        assert np.allclose(Qs, data['Q'][s], rtol=0, atol=1e-13 * np.abs(data['Q'][0]).max())
        assert all(np.allclose(B[k], data['coefficients'][s, k], rtol=0, atol=1e-13) for k in range(s))


def test_taps_are_the_models():
    """H[s][0] = R_s^-T with R_s^T R_s = Q_s, R_s upper triangular, and H[s][k] = -R_s^-T B_k"""
    sequence = vr.synthetic_sequence(ga.lstsq, 3, 4, 2911)
    taps = ga.lstsq.VectorNoise(sequence).taps()
    for s, model in enumerate(sequence.models):
        R = np.linalg.cholesky(model.white_noise_covariance).T
        assert np.allclose(taps[s, 0], np.linalg.inv(R).T, rtol=1e-13, atol=0)
        for k in range(1, s + 1):
            assert np.allclose(taps[s, k], -np.linalg.inv(R).T @ model.coefficients[k - 1], rtol=1e-13, atol=1e-16)


# ---- 2: the checks of VectorNoise ------------------------------------------------------------------------------------------------------
def _model(order, K, covariance=None):
    return ga.lstsq.AutoregressiveModel([0.1 / (k + 1) * np.eye(K) for k in range(order)], np.eye(K) if covariance is None else covariance)


def _plain(q, K):
    return ga.lstsq.AutoregressiveModelSequence([_model(s, K) for s in range(q + 1)])


def test_vector_noise_checks():
    noise, sequence = ga.lstsq.VectorNoise, ga.lstsq.AutoregressiveModelSequence
    assert noise(_plain(128, 2)).taps().shape == (129, 129, 2, 2) and noise(_plain(0, 6)).taps().shape == (1, 1, 6, 6)
    for K in (1, 7):
        with pytest.raises(ValueError, match='dimension {0}: expected 2 .. 6'.format(K)):
            noise(_plain(2, K))
    with pytest.raises(ValueError, match='maximum order 129 of the noise model above 128'):
        noise(_plain(129, 2))
    with pytest.raises(ValueError, match='expected the orders 0, 1, ..., 2'):
        noise(sequence([_model(0, 3), _model(2, 3), _model(2, 3)]))
    with pytest.raises(ValueError, match='without AR models'):
        noise(sequence([]))
    for bad in (None, [_plain(2, 3)], 'var', vr.process(3)):
        with pytest.raises(ValueError, match='takes one AutoregressiveModelSequence'):
            noise(bad)
    indefinite = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match='order 1 is not positive definite'):
        noise(sequence([_model(0, 3), _model(1, 3, indefinite), _model(2, 3)]))
    skewed = np.eye(3)
    skewed[0, 1] = 0.5
    with pytest.raises(ValueError, match='order 2 is not a finite symmetric'):
        noise(sequence([_model(0, 3), _model(1, 3), _model(2, 3, skewed)]))
    with pytest.raises(ValueError, match='order 0 is not a finite symmetric'):
        noise(sequence([_model(0, 3, np.full((3, 3), np.nan)), _model(1, 3)]))
    with pytest.raises(ValueError, match='order 1 is not a finite symmetric'):
        noise(sequence([_model(0, 3), _model(1, 3, np.eye(2))]))
    for coefficient in (np.full((3, 3), np.inf), np.eye(2), np.ones(3)):
        with pytest.raises(ValueError, match='coefficient 1 of the model of order 1 is not a finite'):
            noise(sequence([_model(0, 3), ga.lstsq.AutoregressiveModel([coefficient], np.eye(3))]))


def test_a_bare_sequence_of_dimension_k_still_raises():
    for K in (2, 3):
        with pytest.raises(ValueError, match='dimension {0}'.format(K)):
            ga.lstsq.whitening_taps(_plain(2, K))
        with pytest.raises(ValueError, match='dimension {0}'.format(K)):
            ga.lstsq.ColouredNoise(_plain(2, K))
        with pytest.raises(ValueError, match='dimension {0}'.format(K)):
            ga.lstsq.decorrelate(np.ones((5, K)), _plain(2, K))
    with pytest.raises(ValueError, match='dimension 2'):
        ga.lstsq.CovarianceFunction([np.eye(2), 0.1 * np.eye(2)])


# ---- 3: the routing, before the device -----------------------------------------------------------------------------------------------------
def _constructors():
    """components: the from_* call on five valid points under ColouredNoise(noise_model, arcs); 'keywords' (3 components): the
    noise_model= / arcs= keywords of from_accelerations itself; 'arc' (3): under ArcParameters with a general basis; 'temporal' (3):
    TemporalParameters(model=)"""
    xyz = di.positions()[:5]
    a, b = (x[:5] for x in li.pairs())
    noise = ga.lstsq.ColouredNoise
    general = np.ones((5, 3, 2))
    epochs = np.linspace(58000.0, 58010.0, 5)
    return {'keywords': lambda noise_model, arcs=None, **kw: ga.lstsq.NormalEquations.from_accelerations(
                xyz, np.ones((5, 3)), 0, 4, noise_model=noise_model, arcs=arcs, **kw),
            3: lambda noise_model, arcs=None, **kw: noise(noise_model, arcs).from_accelerations(xyz, np.ones((5, 3)), 0, 4, **kw),
            4: lambda noise_model, arcs=None, **kw: noise(noise_model, arcs).from_gradients(xyz, np.ones((5, 4)), 0, 4,
                                                                                           components=('xx', 'yy', 'zz', 'xz'), **kw),
            1: lambda noise_model, arcs=None, **kw: noise(noise_model, arcs).from_line_of_sight(a, b, np.ones(5), 0, 4, **kw),
            'arc': lambda noise_model, arcs=None, **kw: ga.lstsq.ArcParameters(general, arcs, noise_model).from_accelerations(
                xyz, np.ones((5, 3)), 0, 4, **kw),
            'temporal': lambda noise_model, arcs=None, **kw: ga.lstsq.TemporalParameters.linear(
                np.array([58000.0, 58010.0]), epochs, model=noise(noise_model, arcs)).from_accelerations(xyz, np.ones((5, 3)), 0, 4, **kw),
            'post fit': lambda noise_model, arcs=None, **kw: ga.lstsq.PostFit.of_accelerations(
                np.zeros(25), xyz, np.ones((5, 3)), 0, 4, model=noise(noise_model, arcs), **kw)}


def test_constructors_check_the_vector_model_before_the_device():
    """every ValueError below is raised without a GPU: the checks precede require_gpu"""
    two, three, five = (ga.lstsq.VectorNoise(_plain(2, K)) for K in (2, 3, 5))
    for components, build in _constructors().items():
        K = components if isinstance(components, int) else 3
        wrong = two if K != 2 else three
        with pytest.raises(ValueError, match='VectorNoise of dimension {0} for observations of {1} component'.format(wrong.dimension, K)):
            build(wrong)
        with pytest.raises(ValueError, match='VectorNoise of dimension 5 for observations of {0} component'.format(K)):
            build(five, arcs=[0, 2])
        with pytest.raises(ValueError, match='pass it alone'):
            build([three] * K)
        if K == 3:
            with pytest.raises(ValueError, match='arcs must'):
                build(three, arcs=[0, 5])
            with pytest.raises(ValueError, match='pass it alone'):
                build([three, _plain(2, 1), _plain(2, 1)])
    with pytest.raises(ValueError, match='VectorNoise of dimension 3 for observations of 1 component'):
        ga.lstsq.decorrelate(np.ones(5), three)
    with pytest.raises(ValueError, match='VectorNoise of dimension 3 for observations of 2 components'):
        ga.lstsq.decorrelate(np.ones((5, 2)), three)
    with pytest.raises(ValueError, match='arcs must'):
        ga.lstsq.decorrelate(np.ones((5, 3)), three, arcs=[0, 7])
    with pytest.raises(ValueError, match='pass it alone'):
        ga.lstsq.decorrelate(np.ones((5, 3)), [three, three, three])
    with pytest.raises(ValueError, match='pass it alone'):
        ga.lstsq.whitening_taps([three])
    with pytest.raises(ValueError, match='noise_model must be'):
        ga.lstsq.whitening_taps(three)                                                     # the scalar table has no vector form


def test_shared_arc_basis_is_refused_under_a_vector_model():
    three = ga.lstsq.VectorNoise(_plain(2, 3))
    shared = ga.lstsq.arc_basis(None, 5, degree=1)
    with pytest.raises(ValueError, match=r'lstsq\.component_basis\(basis, 3\)'):
        ga.lstsq.ArcParameters(shared, noise_model=three)
    assert ga.lstsq.ArcParameters(shared, noise_model=_plain(2, 1)).basis.shape == (5, 2)                  # the scalar model keeps the shared form
    general = ga.lstsq.ArcParameters(ga.lstsq.component_basis(shared, 3), noise_model=three)
    assert general.basis.shape == (5, 3, 6) and general.noise_model is three


def test_component_basis():
    basis = ga.lstsq.arc_basis([0, 4], 9, degree=1, periods=(5.0,))
    M, u = basis.shape
    for K in (1, 3, 4):
        general = ga.lstsq.component_basis(basis, K)
        assert general.shape == (M, K, K * u) and general.dtype == np.float64
        for c in range(K):
            assert np.array_equal(general[:, c, c * u:(c + 1) * u], basis)                                 # parameter index c u + j
            outside = np.delete(general[:, c], np.s_[c * u:(c + 1) * u], axis=1)
            assert not np.any(outside)
    assert ga.lstsq.component_basis(np.ones((5, 4)), 4).shape == (5, 4, 16)
    with pytest.raises(ValueError, match='17 columns|18 columns|20 columns'):
        ga.lstsq.component_basis(np.ones((5, 4)), 5)
    with pytest.raises(ValueError, match='18 columns of the component basis: expected at most 16'):
        ga.lstsq.component_basis(np.ones((5, 6)), 3)
    with pytest.raises(ValueError, match=r'basis must have shape \(M, u\)'):
        ga.lstsq.component_basis(np.ones((5, 3, 2)), 3)
    with pytest.raises(ValueError, match='components must be positive'):
        ga.lstsq.component_basis(np.ones((5, 2)), 0)


def test_signatures():
    import inspect
    assert list(inspect.signature(ga.lstsq.VectorNoise).parameters) == ['sequence']
    assert list(inspect.signature(ga.lstsq.component_basis).parameters) == ['basis', 'components']
    assert list(inspect.signature(ga.engine.whiten_rows_vector).parameters) == ['X', 'taps', 'stage', 'skip', 'out']
    assert list(inspect.signature(ga.engine.segment_cross_lag_products).parameters) == ['X', 'seg', 'lags', 'out']
    assert list(inspect.signature(ga.lstsq.PostFit.cross_covariance_function).parameters) == ['self', 'maximum_lag', 'biased']
    assert list(inspect.signature(ga.lstsq.PostFit.vector_noise).parameters) == ['self', 'maximum_lag', 'window']
    assert ga.engine.whiten_vector_info(2) == ga.engine.whiten_vector_info(3) == {'tile_columns': 1024}
    assert ga.engine.whiten_vector_info(4) == ga.engine.whiten_vector_info(6) == {'tile_columns': 512}


# ---- 4: the C entry points --------------------------------------------------------------------------------------------------------------
def test_whiten_rows_vector_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    call = lib.shg_whiten_rows_vector
    X, Y, stage, taps = (ctypes.c_void_p(address) for address in (0x10000000, 0x20000000, 0x30000000, 0x30010000))   # never dereferenced

    def error():
        return lib.shg_last_error().decode()
    #    groups K M  X  ldx stage taps q skip Y ldy stream
    for groups, M, ldx, ldy in ((-1, 10, 10, 10), (2, -1, 10, 10), (2, 10, -1, 10), (2, 10, 10, -1)):
        assert call(groups, 3, M, X, ldx, stage, taps, 5, 0, Y, ldy, None) == -1
        assert 'shg_whiten_rows_vector: negative size' in error()
    for K in (-1, 0, 1, 7):
        assert call(2, K, 10, X, 10, stage, taps, 5, 0, Y, 10, None) == -1
        assert 'dimension K {0} outside 2 .. 6'.format(K) in error()
    for q in (-1, 129):
        assert call(2, 3, 10, X, 10, stage, taps, q, 0, Y, 10, None) == -1
        assert 'order q {0} outside 0 .. 128'.format(q) in error()
    for skip in (-1, 11):
        assert call(2, 3, 10, X, 10, stage, taps, 5, skip, Y, 10, None) == -1
        assert 'skip {0} outside 0 .. M 10'.format(skip) in error()
    assert call(2, 3, 10, X, 9, stage, taps, 5, 0, Y, 10, None) == -1
    assert 'ldx 9 below M 10' in error()
    assert call(2, 3, 10, X, 10, stage, taps, 5, 4, Y, 5, None) == -1
    assert 'ldy 5 below M - skip 6' in error()
    for pointers in ((None, stage, taps, Y), (X, None, taps, Y), (X, stage, None, Y), (X, stage, taps, None)):
        assert call(2, 3, 10, pointers[0], 10, pointers[1], pointers[2], 5, 0, pointers[3], 10, None) == -1
        assert 'shg_whiten_rows_vector: NULL pointer' in error()
    assert call((1 << 19) + 1, 2, 1 << 20, X, 1 << 20, stage, taps, 5, 0, Y, 1 << 20, None) == -1          # 2^40 + 2^21 values
    assert 'are too large' in error()
    assert call(1 << 19, 2, 4, X, 4, stage, taps, 5, 0, Y, (1 << 20) + 1, None) == -1                       # ... of Y alone
    assert 'are too large' in error()
    assert call(1 << 62, 6, 4, X, 4, stage, taps, 5, 0, Y, 4, None) == -1                                   # groups x K past 64 bits
    assert 'are too large' in error()
    base, span = 0x10000000, 8 * (5 * 704 + 700)                  # X [6][704] with 700 columns in use and Y [6][704]
    for y in (base, base + 8, base + span - 8, base - span + 8, base + 8 * 704):
        assert call(2, 3, 700, ctypes.c_void_p(base), 704, stage, taps, 5, 0, ctypes.c_void_p(y), 704, None) == -1, hex(y)
        assert 'X and Y overlap' in error()
    assert call(2, 3, 700, ctypes.c_void_p(base), 704, stage, taps, 5, 5, ctypes.c_void_p(base + 40), 704, None) == -1
    assert 'X and Y overlap' in error()
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(0, 3, 10, None, 10, None, None, 5, 0, None, 10, None) == 0
    assert call(2, 3, 10, None, 10, None, None, 5, 10, None, 0, None) == 0
    assert call(2, 3, 0, None, 0, None, None, 0, 0, None, 0, None) == 0
    with pytest.raises(_lib.ShgError, match='dimension K 7 outside 2 .. 6'):
        _lib.call('shg_whiten_rows_vector', 2, 7, 10, X, 10, stage, taps, 5, 0, Y, 10, None)
    tile = ctypes.c_int(-1)
    assert lib.shg_whiten_vector_info(3, ctypes.byref(tile)) == 0 and tile.value == 1024
    assert lib.shg_whiten_vector_info(5, None) == 0
    for K in (1, 7):
        assert lib.shg_whiten_vector_info(K, ctypes.byref(tile)) == -1 and 'outside 2 .. 6' in error() and tile.value == 1024


def test_segment_cross_lag_products_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    call = lib.shg_segment_cross_lag_products
    X, seg, S = (ctypes.c_void_p(address) for address in (0x10000000, 0x20000000, 0x30000000))             # never dereferenced

    def error():
        return lib.shg_last_error().decode()
    #    K M  X ldx lags nseg seg S stream
    for M, ldx in ((-1, 10), (10, -1)):
        assert call(3, M, X, ldx, 5, 2, seg, S, None) == -1
        assert 'shg_segment_cross_lag_products: negative size' in error()
    for K in (-1, 0, 7):
        assert call(K, 10, X, 10, 5, 2, seg, S, None) == -1
        assert 'dimension K {0} outside 1 .. 6'.format(K) in error()
    for lags in (-1, 129):
        assert call(3, 10, X, 10, lags, 2, seg, S, None) == -1
        assert 'lags {0} outside 0 .. 128'.format(lags) in error()
    assert call(3, 10, X, 10, 5, -1, seg, S, None) == -1
    assert 'nseg -1 is negative' in error()
    assert call(3, 10, X, 9, 5, 2, seg, S, None) == -1
    assert 'ldx 9 below M 10' in error()
    assert call(6, 10, X, 1 << 38, 5, 2, seg, S, None) == -1
    assert 'are too large' in error()
    assert call(3, 10, X, 10, 5, (1 << 24) + 1, seg, S, None) == -1
    assert 'are too large' in error()
    for pointers in ((None, seg, S), (X, None, S), (X, seg, None)):
        assert call(3, 10, pointers[0], 10, 5, 2, pointers[1], pointers[2], None) == -1
        assert 'shg_segment_cross_lag_products: NULL pointer' in error()
    assert call(3, 10, None, 10, 5, 0, None, None, None) == 0                                              # no segment: nothing to do
    with pytest.raises(_lib.ShgError, match='lags 129 outside 0 .. 128'):
        _lib.call('shg_segment_cross_lag_products', 3, 10, X, 10, 129, 2, seg, S, None)
