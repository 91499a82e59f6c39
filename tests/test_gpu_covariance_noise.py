"""
Coloured noise given by a covariance function on the GPU: the kernel of shg_whiten_rows_long against the dense filter in
np.longdouble at every seam of its tiling (also below q = 128, where engine.whiten_rows does not send it), repeated calls bitwise,
blocks with their halo against the whole, and lstsq.CovarianceFunction through decorrelate and the from_* / of_* calls against NumPy
products with W_a = inv(cholesky(Toeplitz(c)[:n_a, :n_a])) per arc, built without the taps code.
"""
import functools

import numpy as np
import pytest

import acceleration_inputs as ai
import covariance_noise_inputs as ci
import design_inputs as di
import gradient_design_inputs as gdi
import grates_amd as ga

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ARCS = [0, 1, 4, 300]                 # arcs of 1, 3, 296 and 400 points
SENTINEL = -7.25


def _host(t):
    return t if isinstance(t, np.ndarray) else ga.engine.to_host(t)


def _padded(values, ld, fill):
    """device matrix [rows, ld] filled with `fill`, `values` in its first columns; returns the matrix and the view of the values"""
    import torch
    rows, M = values.shape
    full = torch.full((rows, ld), fill, dtype=torch.float64, device=ga.engine.device())
    full[:, :M] = ga.engine.to_device(values)
    return full, full[:, :M]


def _call(name, X, taps_d, stage_d, channels, skip, Y):
    """the C entry `name` on two-dimensional views with unit column stride"""
    from grates_amd import _lib
    rows, M = (int(size) for size in X.shape)
    assert X.stride(1) == 1 and tuple(Y.shape) == (rows, M - skip) and (Y.shape[1] == 0 or Y.stride(1) == 1)
    _lib.call(name, rows, channels, M, ga.engine._ptr(X), int(X.stride(0)), ga.engine._ptr(stage_d), ga.engine._ptr(taps_d), int(taps_d.shape[-1]) - 1,
              skip, ga.engine._ptr(Y), int(Y.stride(0)), ga.engine._stream())
    return Y


def _clamped(stage, q):
    return np.minimum(np.minimum(np.maximum(stage, 0), q), np.arange(len(stage)))


# ---- the kernel against the dense filter ----------------------------------------------------------------------------------------------
#  q, rows per channel, M, arcs, skip: every q, row count, M, skip and arc structure of the list once, the large M with few rows
KERNEL_CASES = [(0, 1, 1, None, 0), (1, 127, 127, None, 1), (15, 128, 128, None, 0), (16, 129, 129, None, 1), (17, 1, 700, ARCS, 129),
                (128, 2, 700, ARCS, 0), (129, 3, 700, ARCS, 300), (300, 2, 1500, ARCS, 300), (300, 129, 129, None, 0),
                (1023, 1, 1500, None, 129), (1023, 2, 700, None, 0), (300, 128, 127, None, 1), (129, 127, 300, [0, 1, 4], 0)]
CHANNELS = 3


@functools.lru_cache(maxsize=None)
def _kernel_case(q, rpc, M, arcs, skip, wrong=False):
    """(taps, stage as handed to the kernel, X, reference in np.longdouble, bound) on the host; wrong: the stage table holds -5 and
    10^6 at a few columns"""
    arcs = None if arcs is None else list(arcs)
    taps = ci.random_taps(CHANNELS, q, 3301 + q)
    stage = ga.lstsq.arc_stages(arcs, M, q)
    if wrong:
        stage = stage.copy()
        stage[[0, 2, M // 2, M - 1]] = 10 ** 6, -5, -5, 10 ** 6
        stage[M // 3] = 10 ** 6
    X = np.random.default_rng(3302 + q + M).standard_normal((rpc * CHANNELS, M))
    n = _clamped(stage, q)
    reference, magnitude = ci.long_filter(taps, n, X, CHANNELS)
    return taps, stage, X, reference, (n[np.newaxis, :] + 2) * U * magnitude


def _run_kernel(case, name='shg_whiten_rows_long'):
    """Y on the host from the padded buffers (ld = M + 4, NaN behind X, a sentinel behind Y), and the padding checks"""
    import torch
    taps, stage, X = case[:3]
    skip, M = case[5], X.shape[1]
    X_full, X_view = _padded(X, M + 4, float('nan'))
    Y_full, _ = _padded(np.full((X.shape[0], M - skip), SENTINEL), M - skip + 4, SENTINEL)
    taps_d, stage_d = ga.engine.to_device(taps), torch.from_numpy(stage).to(ga.engine.device())
    _call(name, X_view, taps_d, stage_d, CHANNELS, skip, Y_full[:, :M - skip])
    torch.cuda.synchronize()
    assert bool((Y_full[:, M - skip:] == SENTINEL).all()) and bool(X_full[:, M:].isnan().all())
    return _host(Y_full[:, :M - skip])


@pytest.mark.parametrize('q, rpc, M, arcs, skip', KERNEL_CASES)
def test_kernel_against_the_dense_filter(q, rpc, M, arcs, skip):
    """entry-wise within (n + 2) u sum_k |h_k| |x[t-k]|, which holds for any order of the n + 1 products and their sums (the zeros of
    the band add nothing); the np.longdouble reference is 2^-11 of it off"""
    case = _kernel_case(q, rpc, M, None if arcs is None else tuple(arcs), skip)
    reference, bound = case[3][:, skip:], case[4][:, skip:]
    Y = _run_kernel(case + (skip,))
    assert Y.shape == reference.shape and np.all(np.isfinite(Y))
    ratio = np.abs(Y - reference) / bound
    print('q {0}, {1} rows per channel, M {2}, skip {3}: {4:.3f} of the bound'.format(q, rpc, M, skip, float(ratio.max())))
    assert np.all(np.abs(Y - reference) <= bound)
    assert np.array_equal(_run_kernel(case + (skip,)), Y)                                           # two calls are bitwise equal
    if q <= 128:
        chain = _run_kernel(case + (skip,), 'shg_whiten_rows')
        print('    against shg_whiten_rows: {0:.3f} of the bound'.format(float((np.abs(Y - chain) / bound).max())))
        assert np.all(np.abs(Y - chain) <= 2 * bound)


@pytest.mark.parametrize('q, rpc, M, arcs', [(17, 2, 700, ARCS), (300, 2, 700, ARCS), (129, 1, 129, None)])
def test_stage_is_clamped(q, rpc, M, arcs):
    """-5 is order 0, 10^6 is cut to q and to the column: wrong numbers for a wrong table, the bound against the clamped table holds"""
    case = _kernel_case(q, rpc, M, None if arcs is None else tuple(arcs), 0, True)
    Y = _run_kernel(case + (0,))
    ratio = np.abs(Y - case[3]) / case[4]
    print('q {0}: {1:.3f} of the bound under a wrong stage table'.format(q, float(ratio.max())))
    assert np.all(np.isfinite(Y)) and np.all(np.abs(Y - case[3]) <= case[4])


@pytest.mark.parametrize('first', [1, 3, 4, 256, 299, 300, 301, 512])
def test_block_with_halo_is_the_whole_within_the_bound(first):
    """the same products in another order: both sides are within the bound of the exact value"""
    import torch
    q, M = 300, 700
    case = _kernel_case(q, 2, M, tuple(ARCS), 0)
    taps, stage, X, _, bound = case
    whole = _run_kernel(case + (0,))
    h = int(stage[first])
    X_d, taps_d, stage_d = ga.engine.to_device(X), ga.engine.to_device(taps), torch.from_numpy(stage).to(ga.engine.device())
    block = ga.engine.whiten_rows(X_d[:, first - h:], taps_d, stage_d[first - h:].contiguous(), channels=CHANNELS, skip=h)
    assert tuple(block.shape) == (X.shape[0], M - first)
    ratio = np.abs(_host(block) - whole[:, first:]) / bound[:, first:]
    print('seam {0}, halo {1}: {2:.3f} of the bound'.format(first, h, float(ratio.max())))
    assert np.all(ratio <= 2.0)


def test_skip_of_everything_writes_nothing():
    import torch
    taps, stage, X = _kernel_case(300, 2, 700, tuple(ARCS), 0)[:3]
    Y_full, _ = _padded(np.full_like(X, SENTINEL), 704, SENTINEL)
    out = ga.engine.whiten_rows(ga.engine.to_device(X), ga.engine.to_device(taps), torch.from_numpy(stage).to(ga.engine.device()), channels=CHANNELS,
                                skip=700, out=Y_full[:, :0])
    assert tuple(out.shape) == (X.shape[0], 0) and bool((Y_full == SENTINEL).all())


# ---- the oracle of the package: W per arc from the Cholesky factor --------------------------------------------------------------------
def _arc_filters(c, arcs, M, from_taps=False):
    """W_a [n_a, n_a] of every arc of a series of M points under the covariance function c_0 .. c_q: inv(cholesky(Toeplitz)) of its
    first min(n_a, q + 1) points and, for a longer arc, the last of these rows shifted along (the AR(q) continuation).
    from_taps: the same from CovarianceFunction.taps(), the second host route"""
    q = len(c) - 1
    starts = list(arcs) + [M]
    head = ci.dense_filter(ga.lstsq.CovarianceFunction(c).taps(), np.arange(q + 1)) if from_taps else np.linalg.inv(np.linalg.cholesky(ci.toeplitz(c)))
    filters = []
    for start, end in zip(starts[:-1], starts[1:]):
        n = end - start
        W = np.zeros((n, n))
        m = min(n, q + 1)
        W[:m, :m] = head[:m, :m]
        for t in range(m, n):
            W[t, t - q:t + 1] = head[q]
        filters.append(W)
    return filters


def _whiten_host(filters, arcs, values):
    """W along the last axis of values [..., M], arc by arc"""
    out = np.empty_like(values)
    for W, start in zip(filters, arcs):
        out[..., start:start + len(W)] = values[..., start:start + len(W)] @ W.T
    return out


def _normals_oracle(c, arcs, At, l, basis=None):
    """(N, n, lPl, bounds) from the plain transposed design matrix At [P, K, M] and observations l [K, M] (host copies of what the
    device holds).  basis [M, u]: parameters per arc and component with these columns are eliminated, by a projection of the whitened
    rows of every arc and component onto the complement of the whitened columns.  Bounds: those of
    tests/test_gpu_whitening.py::_reference_normals for dot products of length K M, plus tenfold the largest difference of the two
    host routes (W from the Cholesky factor, W from the taps), with a floor of 1e-12, both relative to sqrt(N_ii N_jj),
    sqrt(N_ii l^T l) and l^T l: the two routes are both correct and differ by the conditioning of the Toeplitz matrices alone"""
    P, K, M = At.shape
    routes = []
    for from_taps in (False, True):
        filters = _arc_filters(c, arcs, M, from_taps)
        A, b = _whiten_host(filters, arcs, At), _whiten_host(filters, arcs, l)
        if basis is not None:
            B = _whiten_host(filters, arcs, np.ascontiguousarray(basis.T))
            for W, start in zip(filters, arcs):
                arc = slice(start, start + len(W))
                Q = np.linalg.qr(B[:, arc].T)[0]                                                     # [n_a, u], full rank
                A[:, :, arc] -= (A[:, :, arc] @ Q) @ Q.T
                b[:, arc] -= (b[:, arc] @ Q) @ Q.T
        A, b = A.reshape(P, K * M), b.ravel()
        routes.append((A @ A.T, A @ b, float(b @ b), A, b))
    (N, n, lPl, A, b), (N2, n2, lPl2, _, _) = routes
    d = np.sqrt(np.diag(N))
    scale_N, scale_n = np.outer(d, d), d * np.sqrt(lPl)
    routes_differ = max(float((np.abs(N - N2) / scale_N).max()), float((np.abs(n - n2) / scale_n).max()), abs(lPl - lPl2) / lPl)
    slack = 2 * K * M * U + max(10 * routes_differ, 1e-12)
    print('    the host routes differ by {0:.2e}: tolerance {1:.2e} of sqrt(N_ii N_jj)'.format(routes_differ, slack))
    return N, n, lPl, slack * scale_N, slack * scale_n, slack * lPl, A, b


def _check(ne, oracle, label, count):
    N, n, lPl, bound_N, bound_n, bound_l = oracle[:6]
    got_N, got_n, got_l, got_count = ne.to_array()
    assert got_N.shape == N.shape and got_n.shape == (N.shape[0], 1) and got_count == count
    if len(ne.matrix.shape) == 2 and ne.matrix.shape[0] > 1:                                      # several fields: the upper blocks
        got_N, N = np.triu(got_N), np.triu(N)
    print('{0}: N {1:.3f}, n {2:.3f}, lPl {3:.3f} of their bounds'.format(label, float((np.abs(got_N - N) / bound_N).max()),
                                                                          float((np.abs(got_n[:, 0] - n) / bound_n).max()), abs(got_l - lPl) / bound_l))
    assert np.all(np.abs(got_N - N) <= bound_N) and np.all(np.abs(got_n[:, 0] - n) <= bound_n) and abs(got_l - lPl) <= bound_l
    for block in range(ne.matrix.shape[0]):
        matrix = ne.matrix.device_block(block, block)
        assert bool((matrix == matrix.t()).all())
    return ne


def _same(first, second):
    return (bool((first.matrix.device_block(0, 0) == second.matrix.device_block(0, 0)).all()) and bool((first.right_hand_side == second.right_hand_side).all())
            and first.observation_square_sum == second.observation_square_sum and first.observation_count == second.observation_count)


# ---- decorrelate ------------------------------------------------------------------------------------------------------------------------
def test_decorrelate():
    import torch
    c = ci.covariance(400)
    model = ga.lstsq.CovarianceFunction(c)
    filters = _arc_filters(c, ARCS, 700)
    values = np.random.default_rng(3310).standard_normal((700, 3))
    expected = _whiten_host(filters, ARCS, values.T).T
    scale = _whiten_host([np.abs(W) for W in filters], ARCS, np.abs(values).T).T
    tolerance = 402 * U + 1e-12                                      # the dot-product bound and the floor of the second host route
    for given, columns in ((values, slice(None)), (values[:, 0].copy(), 0)):
        got = ga.lstsq.decorrelate(given, model, arcs=ARCS)
        assert isinstance(got, np.ndarray) and got.shape == given.shape
        ratio = np.abs(got - expected[:, columns]) / scale[:, columns]
        print('decorrelate {0}: {1:.2e} of sum |w| |x| (tolerance {2:.2e})'.format(given.shape, float(ratio.max()), tolerance))
        assert np.all(ratio <= tolerance)
    device = ga.lstsq.decorrelate(ga.engine.to_device(values), [model] * 3, arcs=ARCS)
    assert isinstance(device, torch.Tensor) and device.is_cuda and np.array_equal(_host(device), ga.lstsq.decorrelate(values, model, arcs=ARCS))
    short = ga.lstsq.CovarianceFunction(c[:129])                      # q = 128: the chain of shg_whiten_rows on these taps, bitwise
    taps, stage = ga.lstsq._whitening_tables(short, ARCS, 700, 3)
    X_d = ga.engine.to_device(values.T)
    chain = _call('shg_whiten_rows', X_d, ga.engine.to_device(taps), torch.from_numpy(stage).to(ga.engine.device()), 1, 0, torch.empty_like(X_d))
    assert np.array_equal(ga.lstsq.decorrelate(values, short, arcs=ARCS), _host(chain).T)


# ---- normals from accelerations ---------------------------------------------------------------------------------------------------------
NA, MA = 12, 700


@functools.lru_cache(maxsize=None)
def _acceleration_case(q):
    """700 weighted points, d/o 12; q = 399: every arc under its full covariance matrix, q = 200: the banded continuation on the
    arcs of 296 and 400 points"""
    c = ci.covariance(q + 1)
    xyz = np.vstack((di.positions(), ai.scattered_positions(MA - 20, 3321)))
    rng = np.random.default_rng(3322)
    w = rng.uniform(0.25, 4.0, MA)
    w[rng.choice(MA, 20, replace=False)] = 0.0
    w[[0, 3, 4, 299, 300]] = 0.0
    obs = rng.standard_normal((MA, 3)) * 1e-3
    At = _host(ga.engine.acceleration_design(NA, xyz, di.GM, di.R, 0, weights=w))                     # [P, 3, M], times sqrt(w)
    return xyz, w, obs, c, _normals_oracle(c, ARCS, At, (np.sqrt(w)[:, np.newaxis] * obs).T)


def _build_accelerations(q, block_points):
    xyz, w, obs, c, _ = _acceleration_case(q)
    return ga.lstsq.NormalEquations.from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w, block_points=block_points,
                                                       noise_model=ga.lstsq.CovarianceFunction(c), arcs=ARCS)


@pytest.mark.parametrize('q, block_points', [(399, 256), (399, 100), (399, None), (200, 256)])
def test_normals_of_accelerations(q, block_points):
    xyz, w, obs, c, oracle = _acceleration_case(q)
    ne = _check(_build_accelerations(q, block_points), oracle, 'q {0}, blocks of {1}'.format(q, block_points), 3 * MA)
    assert ne.status == 'normal_matrix' and ne.right_hand_side.is_cuda
    assert _same(_build_accelerations(q, block_points), ne)                                          # two runs are bitwise equal
    bound = ga.lstsq.ColouredNoise(ga.lstsq.CovarianceFunction(c), ARCS).from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w,
                                                                                           block_points=block_points)
    assert _same(bound, ne)


# ---- small cases ------------------------------------------------------------------------------------------------------------------------
NG, MG = 8, 300
TWO_ARCS = [0, 140]
GOCE = ('xx', 'yy', 'zz', 'xz')


def test_normals_of_gradients_with_four_functions():
    """one covariance function per component, q = 159: both arcs (140 and 160 points) under their full matrices; blocks of 128"""
    functions = [ci.covariance(160) * scale + shift * (np.arange(160) == 0) for scale, shift in ((1.0, 0.0), (2.0, 0.1), (0.5, 0.3), (1.5, 0.05))]
    models = [ga.lstsq.CovarianceFunction(c) for c in functions]
    xyz, frames = ai.scattered_positions(MG, 3331), gdi.frames(MG, 3332)
    rng = np.random.default_rng(3333)
    w = rng.uniform(0.25, 4.0, (MG, 4))
    w[rng.choice(MG, 10, replace=False), rng.integers(0, 4, 10)] = 0.0
    obs = rng.standard_normal((MG, 4)) * 1e-9
    At = _host(ga.engine.gradient_design(NG, xyz, gdi.GM, gdi.R, 0, frames=frames, components=GOCE, weights=w))     # [P, 4, M]
    l = (np.sqrt(w) * obs).T
    P = At.shape[0]
    # per component its own filters: the oracle of one function on the rows of that component, sums over the components
    parts = [_normals_oracle(c, TWO_ARCS, At[:, k:k + 1], l[k:k + 1]) for k, c in enumerate(functions)]
    oracle = tuple(sum(part[i] for part in parts) for i in range(6))

    def build():
        return ga.lstsq.ColouredNoise(models, TWO_ARCS).from_gradients(xyz, obs, 0, NG, gdi.GM, gdi.R, frames=frames, components=GOCE, weights=w,
                                                                       block_points=128)
    ne = _check(build(), oracle, 'gradients', 4 * MG)
    assert ne.matrix.device_block(0, 0).shape == (P, P) and _same(build(), ne)


def test_closed_loop_recovers_the_field_under_the_full_covariance(golden):
    """the noise-free loop of tests/test_gpu_whitening.py under the full covariance matrices of two arcs (q = 399 >= 350 - 1):
    consistent observations give the same solution under any positive definite weight matrix, so the bound stays 10 times the host's
    error of the unweighted loop"""
    data = golden('g24_acceleration_design')
    host_rel_err = float(data['host_rel_err'])
    assert float(data['loop_cond']) <= 1e4 and host_rel_err <= 1e-8
    N, min_degree = di.LOOP['N'], di.LOOP['min_degree']
    xyz = ga.engine.to_device(di.loop_positions())
    gf = ga.gravityfield.PotentialCoefficients(di.GM, di.R)
    gf.anm = di.loop_field()
    g = gf.gravitational_acceleration(xyz, as_tensor=True)
    model = ga.lstsq.CovarianceFunction(ci.covariance(400))
    ne = ga.lstsq.NormalEquations.from_accelerations(xyz, g, min_degree, N, di.GM, di.R, noise_model=model, arcs=[0, 250])
    assert ne.observation_count == 1800
    truth = ga.utilities.ravel_coefficients(gf.anm, min_degree, N)
    solution = _host(ne.solve())[:, 0]
    rel = np.linalg.norm(solution - truth) / np.linalg.norm(truth)
    print('closed loop: relative error {0:.2e} (host {1:.2e})'.format(rel, host_rel_err))
    assert rel <= 10 * host_rel_err


def _small_case(seed):
    """300 accelerations at d/o 8 in the arcs [0, 140], weights with zeros, and the covariance function at q = 159"""
    rng = np.random.default_rng(seed)
    xyz = ai.scattered_positions(MG, seed + 1)
    w = rng.uniform(0.25, 4.0, MG)
    w[rng.choice(MG, 10, replace=False)] = 0.0
    return xyz, w, rng.standard_normal((MG, 3)) * 1e-3, ci.covariance(160)


def test_arc_parameters_and_the_post_fit():
    """bias and drift per arc and axis under the full covariance matrices (no weights: the basis keeps its rank); the residual square
    sum of PostFit against l^T P l - n^T x of the normals, within 1e-9 l^T P l: a thousand times the tolerance of the normals, for
    the square sum is stationary in x and the condition of N does not enter at first order"""
    xyz, _, obs, c = _small_case(3340)
    basis = ga.lstsq.arc_basis(TWO_ARCS, MG, degree=1)
    model = ga.lstsq.ArcParameters(basis, TWO_ARCS, noise_model=ga.lstsq.CovarianceFunction(c))
    At = _host(ga.engine.acceleration_design(NG, xyz, di.GM, di.R, 0))
    oracle = _normals_oracle(c, TWO_ARCS, At, obs.T.copy(), basis)
    ne = _check(model.from_accelerations(xyz, obs, 0, NG, di.GM, di.R, block_points=128), oracle, 'arc parameters', 3 * MG - 12)
    got_N, got_n, got_l, _ = ne.to_array()
    solved = ga.lstsq.accumulate_normals([ne], [1.0])                                                # ne keeps its normal matrix
    signs = np.where(np.random.default_rng(3341).integers(0, 2, (got_N.shape[0], 6)) == 1, 1.0, -1.0)
    x = _host(solved.solve(signs=signs))[:, 0]
    fit = ga.lstsq.PostFit.of_accelerations(x, xyz, obs, 0, NG, di.GM, di.R, block_points=128, model=model, vectors=_host(solved.monte_carlo_vectors))
    got, expected = float(np.sum(np.asarray(fit.whitened) ** 2)), got_l - float(got_n[:, 0] @ x)
    print('    residual square sum {0:.6e}, l^T P l - n^T x {1:.6e}: {2:.2e} of l^T P l'.format(got, expected, abs(got - expected) / got_l))
    assert abs(got - expected) <= 1e-9 * got_l
    A, b = oracle[6:]
    e = (b - A.T @ x).reshape(3, MG)
    sums = np.array([np.sum(e[:, :140] ** 2), np.sum(e[:, 140:] ** 2)])
    print('    square sums of the arcs: {0:.2e} off the host'.format(float((np.abs(fit.arc_square_sums - sums) / sums).max())))
    assert np.all(np.abs(fit.arc_square_sums - sums) <= 1e-9 * sums)
    factors = fit.arc_variance_factors()
    redundancies = fit.arc_redundancies()
    print('    redundancies of the arcs {0}, variance factors {1}'.format(redundancies, factors))
    assert factors.shape == (2,) and np.all(np.isfinite(factors)) and np.array_equal(factors, fit.arc_square_sums / redundancies)
    assert np.all(redundancies > 0) and np.all(redundancies <= 3 * np.array([140, 160]) - 6)          # below the rows an arc keeps


def test_temporal_parameters_with_two_nodes():
    """linear interpolation between two fields: the design matrix of field e is f_e(t) A, whitened after the expansion"""
    xyz, w, obs, c = _small_case(3350)
    epochs = np.linspace(0.05, 0.95, MG)
    temporal = ga.lstsq.TemporalParameters.linear(np.array([0.0, 1.0]), epochs, model=ga.lstsq.ColouredNoise(ga.lstsq.CovarianceFunction(c), TWO_ARCS))
    At = _host(ga.engine.acceleration_design(NG, xyz, di.GM, di.R, 0, weights=w))
    expanded = np.concatenate(((1.0 - epochs) * At, epochs * At), axis=0)
    oracle = _normals_oracle(c, TWO_ARCS, expanded, (np.sqrt(w)[:, np.newaxis] * obs).T)
    ne = temporal.from_accelerations(xyz, obs, 0, NG, di.GM, di.R, weights=w, block_points=128)
    assert ne.matrix.shape == (2, 2)
    _check(ne, oracle, 'two nodes in time', 3 * MG)


def test_radial_basis_parameters():
    import rbf_inputs as ri
    xyz, w, obs, c = _small_case(3360)
    lon, lat = ri.scattered_nodes(40, 3361)
    basis = ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat, a=ri.A, f=ri.F), ri.shape_factors(ri.degree_factors(2, NG)), 2, NG,
                                                 ri.GM, ri.R)
    bound = ga.lstsq.RadialBasisParameters(basis, ga.lstsq.ColouredNoise(ga.lstsq.CovarianceFunction(c), TWO_ARCS))
    At = _host(ga.engine.rbf_design('acceleration', basis, xyz, weights=w))                          # [40, 3, M]
    oracle = _normals_oracle(c, TWO_ARCS, At, (np.sqrt(w)[:, np.newaxis] * obs).T)
    ne = _check(bound.from_accelerations(xyz, obs, weights=w, block_points=128), oracle, 'radial basis functions', 3 * MG)
    assert ne.matrix.device_block(0, 0).shape == (40, 40)
