"""
The post-fit pass on the GPU: the kernel of shg_segment_lag_products (engine.segment_lag_products) against exact sums, bitwise wherever
a segment lies and whatever `lags` is, and lstsq.PostFit for the three kinds of observation against NumPy formulations
(tests/golden/postfit_inputs.py) on host copies of the device's design matrices and against what the normal equations already give:
the square sum of the residuals, the parameters of the arcs, the redundancy, the exact trace, ranks, the covariance function and the
loop closed once.
"""
import functools

import numpy as np
import pytest

import acceleration_inputs as ai
import arc_inputs as arc
import design_inputs as di
import gradient_design_inputs as gdi
import grates_amd as ga
import los_inputs as li
import postfit_inputs as pf
import whitening_inputs as wi

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHORT_ARCS = [0, 1, 4, 300]
ARCS = [0, 150, 300]
N, MIN_DEGREE, M = 12, 2, 700
P = (N + 1) ** 2 - MIN_DEGREE ** 2
GOCE = ('xx', 'yy', 'zz', 'xz')


def _host(t):
    return ga.engine.to_host(t) if ga.lstsq._is_tensor(t) else np.asarray(t)


def _int32(values):
    import torch
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=ga.engine.device())


def _padded(values, pad, fill):
    """device tensor with `pad` more columns than `values` [..., M], filled with `fill`; returns the view of the values"""
    import torch
    full = torch.full(values.shape[:-1] + (values.shape[-1] + pad,), fill, dtype=torch.float64, device=ga.engine.device())
    full[..., :values.shape[-1]] = ga.engine.to_device(values)
    return full[..., :values.shape[-1]]


def _lags(X, seg, lags, **kwargs):
    return ga.engine.segment_lag_products(X, _int32(seg), lags, **kwargs)


# ---- 1: the kernel against exact sums ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_case(seg):
    X = np.random.default_rng(2910).standard_normal((6, 700))
    return (X,) + pf.exact_lag_products(X, list(seg), 128)


@pytest.mark.parametrize('seg', [(0, 1, 4, 300, 700), (3, 3, 70, 650)])
@pytest.mark.parametrize('lags', [0, 5, 128])
def test_kernel_against_exact_sums(lags, seg):
    """entry-wise within (n + 1) u sum |x_t x_(t+k)|, n the number of pairs: a chain and the tree round at most n times between them,
    and the exact reference once.  The padding of the rows and every column outside the segments is NaN: a read of it would poison a
    sum.  Entries with no pair are exactly 0."""
    import torch
    X, reference, magnitude, pairs = _exact_case(seg)
    reference, magnitude, pairs = reference[:, :, :lags + 1], magnitude[:, :, :lags + 1], pairs[:, :lags + 1]
    covered = np.zeros(700, dtype=bool)
    for first, last in zip(seg[:-1], seg[1:]):
        covered[first:last] = True
    X_nan = np.where(covered, X, np.nan)
    view = _padded(X_nan, 4, float('nan'))
    S = _lags(view, seg, lags)
    assert tuple(S.shape) == (6, len(seg) - 1, lags + 1) and S.is_contiguous()
    got = _host(S)
    assert np.all(np.isfinite(got))
    bound = (pairs[None] + 1) * U * magnitude
    ratio = np.abs(got - reference) / np.where(bound > 0, bound, 1.0)
    print('lags {0}, seg {1}: {2:.3f} of the bound'.format(lags, seg, ratio.max()))
    assert np.all(np.abs(got - reference) <= bound)
    assert np.all(got[:, pairs == 0] == 0.0)
    # views and outputs: the column slice above, the dense matrix and a given output are bitwise the same
    out = torch.full((6, len(seg) - 1, lags + 1), -7.25, dtype=torch.float64, device=S.device)
    assert _lags(ga.engine.to_device(X_nan), seg, lags, out=out) is out
    assert np.array_equal(_host(out), got)
    assert np.array_equal(_host(_lags(ga.engine.to_device(X_nan).reshape(2, 3, 700), seg, lags)), got.reshape(2, 3, len(seg) - 1, lags + 1))
    assert np.array_equal(_host(_lags(view, seg, lags)), got)                                      # and repeated calls are bitwise equal


# ---- 2: locality, bitwise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('length', [1, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_a_segment_gives_the_same_bits_wherever_it_lies(length):
    """the chains have stride 64, the largest lag is 128 and the kernel of lags > 0 stages tiles of 1024 columns: those and their
    neighbours are the seams.  The data of one segment at offsets 0, 1, 63 and 517 of a longer row, alone and between other segments, in
    a matrix of 1 and of 7 rows (a full group of four rows and a short one), for lags = 0, 5 and 128; and lag k of a call with
    lags = 128 is lag k of a call with lags = k"""
    rng = np.random.default_rng(2920 + length)
    x = rng.standard_normal(length)
    references = {lags: _host(_lags(ga.engine.to_device(x[None]), [0, length], lags)) for lags in (0, 5, 128)}
    assert references[128].shape == (1, 1, 129)
    assert np.array_equal(references[128][..., :1], references[0]) and np.array_equal(references[128][..., :6], references[5])
    for k in (1, 2, 33, 64, 127):
        assert np.array_equal(_host(_lags(ga.engine.to_device(x[None]), [0, length], k))[..., k], references[128][..., k])
    assert np.all(references[128][0, 0, min(length, 129):] == 0.0)
    for offset in (0, 1, 63, 517):
        width = offset + length + 130
        row = rng.standard_normal(width)
        row[offset:offset + length] = x
        X7 = rng.standard_normal((7, width))
        X7[3], X7[6] = row, row
        one, seven = ga.engine.to_device(row[None]), ga.engine.to_device(X7)
        alone, between = [offset, offset + length], [0, offset, offset + length, width - 7, width]
        for lags, reference in references.items():
            assert np.array_equal(_host(_lags(one, alone, lags)), reference)
            assert np.array_equal(_host(_lags(one, between, lags))[:, 1:2], reference)
            many = _host(_lags(seven, between, lags))
            assert np.array_equal(many[3:4, 1:2], reference) and np.array_equal(many[6:7, 1:2], reference)
            assert np.array_equal(_host(_lags(seven, alone, lags))[[3, 6]], np.concatenate((reference, reference)))


# ---- 3: clamping -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lags', [0, 5, 128])
def test_segment_table_is_clamped(lags):
    """a wrong table gives wrong numbers, not a fault: entries are clamped to 0 .. M and made non-decreasing.  With four columns of
    padding even an unclamped read of the table's M + 3 would stay inside the allocation, and at 1e300 it would show"""
    rows, width = 6, 700
    X = np.random.default_rng(2930).standard_normal((rows, width))
    view = _padded(X, 4, 1e300)
    wrong = [-2, 5, 3, width + 3]
    assert arc.clamped(wrong, width).tolist() == [0, 5, 5, width]
    got = _lags(view, wrong, lags)
    expected = _lags(view, arc.clamped(wrong, width), lags)
    assert bool((got == expected).all()) and bool(got.isfinite().all()) and bool((got[:, 1] == 0).all())
    reference, magnitude, pairs = pf.exact_lag_products(X, arc.clamped(wrong, width), lags)
    assert np.all(np.abs(_host(got) - reference) <= (pairs[None] + 1) * U * magnitude)
    extreme = _lags(view, [2 ** 31 - 1, -2 ** 31, 5, 2], lags)
    assert bool((extreme == 0).all())                                                              # everything lies behind the first entry


# ---- the cases of the pass ---------------------------------------------------------------------------------------------------------------
def _device_tables(model, arcs, count):
    import torch
    taps = ga.lstsq.whitening_taps(model)
    return ga.engine.to_device(taps), torch.from_numpy(ga.lstsq.arc_stages(arcs, count, taps.shape[1] - 1)).to(ga.engine.device()), taps.shape[0]


def _transformed(At, l, basis, root, model, arcs):
    """host copies of what the device holds, whitened and not: (A~ [K M, P], l~ [K M], B~ [K, M, u] or None, A, l, B) from the device's
    design matrix At [P, K, M] times sqrt(w), the observations l [M, K] times sqrt(w), basis [M, u'] or [M, K, u] or None, root [M, K]
    or None"""
    parameters, K, count = (int(size) for size in At.shape)
    plain_B = None if basis is None else arc.transformed_basis(basis, root, K).transpose(2, 0, 1)           # [u, K, M]
    plain_l = np.ascontiguousarray(l.T)
    white_A, white_B, white_l = At, plain_B, plain_l
    if model is not None:
        taps, stage, channels = _device_tables(model, arcs, count)
        white_A = ga.engine.whiten_rows(At, taps, stage, channels=channels)
        white_l = _host(ga.engine.whiten_rows(ga.engine.to_device(plain_l), taps, stage, channels=channels))
        if basis is not None:
            white_B = _host(ga.engine.whiten_rows(ga.engine.to_device(plain_B), taps, stage, channels=channels))

    def rows(matrix):
        return _host(matrix).reshape(parameters, K * count).T.copy()

    def columns(B):
        return None if B is None else np.ascontiguousarray(B.transpose(1, 2, 0))
    return rows(white_A), white_l.ravel(), columns(white_B), rows(At), plain_l.ravel(), columns(plain_B)


class Case:
    """one kind of observation with everything the checks need: the bound constructors, the device's design matrix and the inputs"""

    def __init__(self, kind, K, At, obs, root, build, post):
        self.kind, self.K, self.At, self.obs, self.root, self.build, self.post = kind, K, At, obs, root, build, post

    def model(self, basis, arcs, noise):
        if basis is None:
            return None if noise is None else ga.lstsq.ColouredNoise(noise, arcs)
        return ga.lstsq.ArcParameters(basis, arcs, noise)

    def system(self, model, **kwargs):
        """the normal equations under `model`, through the bound constructor or the classmethod"""
        return self.build(ga.lstsq.NormalEquations if model is None else model, **kwargs)


def _weights(count, K, seed, per_component):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 4.0, (count, K) if per_component else count)
    if per_component:
        w[rng.choice(count, 20, replace=False), rng.integers(0, K, 20)] = 0.0
    else:
        w[rng.choice(count, 20, replace=False)] = 0.0
        w[[0, 3, 4, 299, 300]] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _case(kind, degree=N):
    rng = np.random.default_rng(2940)
    if kind == 'accelerations':
        xyz = np.vstack((di.positions(), ai.scattered_positions(M - 20, 2941)))
        w, obs = _weights(M, 3, 2942, False), rng.standard_normal((M, 3)) * 1e-3
        At = ga.engine.acceleration_design(degree, xyz, di.GM, di.R, MIN_DEGREE, weights=w)
        return Case(kind, 3, At, obs, np.sqrt(w)[:, None],
                    lambda owner, **kw: owner.from_accelerations(xyz, obs, MIN_DEGREE, degree, di.GM, di.R, weights=w, **kw),
                    lambda x, **kw: ga.lstsq.PostFit.of_accelerations(x, xyz, obs, MIN_DEGREE, degree, di.GM, di.R, weights=w, **kw))
    if kind == 'frame':                                                                           # weights per component, for the general basis
        xyz = ai.scattered_positions(M, 2943)
        w, obs = _weights(M, 3, 2944, True), rng.standard_normal((M, 3)) * 1e-3
        At = ga.engine.acceleration_design(degree, xyz, di.GM, di.R, MIN_DEGREE, weights=w)
        return Case(kind, 3, At, obs, np.sqrt(w),
                    lambda owner, **kw: owner.from_accelerations(xyz, obs, MIN_DEGREE, degree, di.GM, di.R, weights=w, **kw),
                    lambda x, **kw: ga.lstsq.PostFit.of_accelerations(x, xyz, obs, MIN_DEGREE, degree, di.GM, di.R, weights=w, **kw))
    if kind == 'gradients':
        xyz, frames = ai.scattered_positions(M, 2945), gdi.frames(M, 2946)
        w, obs = _weights(M, 4, 2947, True), rng.standard_normal((M, 4)) * 1e-9
        At = ga.engine.gradient_design(degree, xyz, gdi.GM, gdi.R, MIN_DEGREE, frames=frames, components=GOCE, weights=w)
        return Case(kind, 4, At, obs, np.sqrt(w),
                    lambda owner, **kw: owner.from_gradients(xyz, obs, MIN_DEGREE, degree, gdi.GM, gdi.R, frames=frames, components=GOCE, weights=w, **kw),
                    lambda x, **kw: ga.lstsq.PostFit.of_gradients(x, xyz, obs, MIN_DEGREE, degree, gdi.GM, gdi.R, frames=frames, components=GOCE,
                                                                  weights=w, **kw))
    assert kind == 'line_of_sight'
    a = ai.scattered_positions(M, 2948)
    b = a + li.SEPARATION * li.unit_vectors(M, 2949)
    w, obs = _weights(M, 1, 2950, False), rng.standard_normal(M) * 1e-6
    At = ga.engine.los_design(degree, a, b, li.GM, li.R, MIN_DEGREE, weights=w)[:, None, :]
    return Case(kind, 1, At, obs[:, None], np.sqrt(w)[:, None],
                lambda owner, **kw: owner.from_line_of_sight(a, b, obs, MIN_DEGREE, degree, li.GM, li.R, weights=w, **kw),
                lambda x, **kw: ga.lstsq.PostFit.of_line_of_sight(x, a, b, obs, MIN_DEGREE, degree, li.GM, li.R, weights=w, **kw))


@functools.lru_cache(maxsize=None)
def _noise(K):
    first = wi.sequence(wi.fixture(), 'ar5', ga.lstsq)
    return first if K != 4 else (first, wi.synthetic_sequence(ga.lstsq, 5, 2731), wi.synthetic_sequence(ga.lstsq, 5, 2732), wi.synthetic_sequence(ga.lstsq, 5, 2733))


def _basis(kind, arcs):
    shared = ga.lstsq.arc_basis(arcs, M, degree=1, periods=(93,))                                  # bias + drift + period 93 per axis
    return ga.lstsq.frame_basis(shared, gdi.frames(M, 2951)) if kind == 'frame' else shared


def _signs(parameters, count, seed=2952):
    return np.where(np.random.default_rng(seed).integers(0, 2, (parameters, count)) == 1, 1.0, -1.0)


def _solve(ne, signs):
    """(x [P], vectors [P, S]) of a copy of the system: ne itself keeps its normal matrix for residual_square_sum and redundancy"""
    solved = ga.lstsq.accumulate_normals([ne], [1.0])
    x = _host(solved.solve(signs=signs))
    return x[:, 0], _host(solved.monte_carlo_vectors), solved


@functools.lru_cache(maxsize=None)
def _host_system(kind, arcs, noise, with_basis=True):
    """the host matrices of a case and the units of its arc parameters, whitened and not"""
    case = _case(kind)
    basis = _basis(kind, list(arcs)) if with_basis else None
    white_A, white_l, white_B, plain_A, plain_l, plain_B = _transformed(case.At, case.root * case.obs, basis, case.root, _noise(case.K) if noise else None,
                                                                        list(arcs))
    bounds = arc.bounds_of(arcs, M)
    shared = basis is not None and basis.ndim == 2
    units = [] if basis is None else arc.explicit_columns(white_B, bounds, shared)
    plain_units = [] if basis is None else arc.explicit_columns(plain_B, bounds, shared)
    return white_A, white_l, units, plain_A, plain_l, plain_units


def _entry_bounds(A, l, units, x, y):
    """the dot-product bound of the issue for l - A x - E y, entry-wise: (P + u + 3) u (sum_j |A_ij| |x_j| + |l_i| + sum |E y|)"""
    magnitude = np.abs(A) @ np.abs(x) + (np.abs(l) if l is not None else 0.0)
    width = 0
    if units:
        E = np.hstack(units)
        magnitude = magnitude + np.abs(E) @ np.abs(y.reshape(E.shape[1], -1) if y.ndim > 1 and x.ndim > 1 else y.ravel())
        width = units[0].shape[1]
    return (A.shape[1] + width + 3) * U * magnitude


def _check_entries(fit, kind, arcs, noise, x, Z, with_basis=True, label=''):
    """whitened, residuals and the rows of V against NumPy on the host copies; returns the references and their bounds"""
    white_A, white_l, units, plain_A, plain_l, plain_units = _host_system(kind, tuple(arcs), noise, with_basis)
    K = _case(kind).K
    value = white_l - white_A @ x
    y = pf.parameters(value, units) if units else np.zeros(0)
    reference = pf.project(value, units)
    bound = _entry_bounds(white_A, white_l, units, x, y)
    got = _host(fit.whitened)
    assert got.shape == (M, K)
    ratio = np.abs(got.T.ravel() - reference) / np.where(bound > 0, bound, 1.0)
    plain_reference = plain_l - plain_A @ x - (np.hstack(plain_units) @ y.ravel() if units else 0.0)
    plain_bound = _entry_bounds(plain_A, plain_l, plain_units, x, y)
    plain_got = _host(fit.residuals)
    assert plain_got.shape == (M, K)
    plain_ratio = np.abs(plain_got.T.ravel() - plain_reference) / np.where(plain_bound > 0, plain_bound, 1.0)
    rows = _host(fit.rows)
    assert rows.shape == (1 + Z.shape[1], K, M) and np.array_equal(rows[0].T, got)
    values = white_A @ Z
    parameters = np.stack([pf.parameters(values[:, j], units) for j in range(Z.shape[1])], axis=-1) if units else np.zeros((0, Z.shape[1]))
    vector_reference = pf.project(values, units)
    vector_bound = _entry_bounds(white_A, None, units, Z, parameters)
    vector_ratio = np.abs(rows[1:].reshape(Z.shape[1], K * M).T - vector_reference) / np.where(vector_bound > 0, vector_bound, 1.0)
    print('{0}: whitened {1:.2e}, residuals {2:.2e}, rows of V {3:.2e} of their bounds (largest |V| {4:.2e}, largest deviation {5:.2e})'.format(
        label, ratio.max(), plain_ratio.max(), vector_ratio.max(), np.abs(rows[1:]).max(), np.abs(rows[1:].reshape(Z.shape[1], K * M).T - vector_reference).max()))
    assert ratio.max() <= 1 and plain_ratio.max() <= 1 and vector_ratio.max() <= 1
    return reference, bound, vector_reference, vector_bound, y


def _square_sum_bounds(A, l, x, values, entry_bound):
    """bounds of the two routes to a square sum |l - A x|^2 of projected values.  Normals: N, n and l^T l carry 2 L u sqrt(N_ii N_jj)
    (...) from their dot products of length L, and the quadratic form of length P is evaluated in floating point:
    (2 L + P + 2) u (|l| + sum_i sqrt(N_ii) |x_i|)^2.  Residuals: entries within entry_bound, squared and summed by the kernel:
    2 sum |v| t + sum t^2 + (L + 1) u sum v^2."""
    L = A.shape[0]
    d = np.sqrt(np.einsum('ij,ij->j', A, A))
    normals = (2 * L + A.shape[1] + 2) * U * ((np.sqrt(l @ l) if l is not None else 0.0) + d @ np.abs(x)) ** 2
    residuals = 2 * np.abs(values) @ entry_bound + entry_bound @ entry_bound + (L + 1) * U * (values @ values)
    return normals + residuals


def _check_consistency(fit, ne, solved, kind, arcs, noise, x, Z, entries, label, factor=1.7):
    """what the pass gives against what the normal equations already give, each within the sum of the bounds of the two routes"""
    white_A, white_l, units, _, _, _ = _host_system(kind, tuple(arcs), noise)
    reference, bound, vector_reference, vector_bound, y = entries
    K = _case(kind).K
    # the square sum of the residuals
    got, expected = float(np.sum(_host(fit.whitened) ** 2)), float(ne.residual_square_sum(x[:, None]))
    limit = _square_sum_bounds(white_A, white_l, x, reference, bound)
    assert abs(fit.arc_square_sums.sum() - got) <= (K * M + 1) * U * got
    # the redundancy
    traces = [_square_sum_bounds(white_A, None, Z[:, j], vector_reference[:, j], vector_bound[:, j]) for j in range(Z.shape[1])]
    trace_limit = sum(traces) / Z.shape[1] / factor
    redundancy, expected_redundancy = fit.arc_redundancies(factor).sum(), float(ne.redundancy(solved, factor))
    # the parameters of the arcs: both routes form R R^T (B^T l - C^T x); c = B^T l - C^T x within (len + P + 4) u m each, m_j = sum_t |B_tj| (|l_t| +
    # sum_p |A_tp| |x_p|), the small products with R within (P + 2 u + 2) u |R| |R^T| m each
    expected_y = ne.arc_elimination.parameters(x)
    assert fit.arc_parameters.shape == expected_y.shape
    magnitude = np.abs(white_A) @ np.abs(x) + np.abs(white_l)
    limits = []
    for E in units:
        R = arc.reduction(E.T @ E)[0]
        length = np.count_nonzero(np.any(E != 0.0, axis=1))
        limits.append((2 * length + 4 * P + 4 * E.shape[1] + 12) * U * (np.abs(R) @ np.abs(R.T)) @ (np.abs(E).T @ magnitude))
    y_ratio = np.abs(fit.arc_parameters - expected_y).ravel() / np.concatenate(limits)
    print('{0}: square sum {1:.2e}, redundancy {2:.2e}, parameters {3:.2e} of their bounds'.format(
        label, abs(got - expected) / limit, abs(redundancy - expected_redundancy) / trace_limit, y_ratio.max()))
    assert abs(got - expected) <= limit
    assert abs(redundancy - expected_redundancy) <= trace_limit
    assert y_ratio.max() <= 1
    assert np.allclose(fit.arc_parameters.ravel(), np.asarray(y).ravel(), rtol=0, atol=1e-6 * np.abs(y).max())       # and the host's own, loosely
    assert int(fit.arc_observation_counts.sum()) == ne.observation_count                          # exactly
    assert np.array_equal(fit.ranks, ne.arc_elimination.ranks) and np.array_equal(fit.arcs, arcs)


# ---- 4: entry-wise against NumPy, and against what exists ---------------------------------------------------------------------------------
@pytest.mark.parametrize('noise', [True, False])
@pytest.mark.parametrize('block_points', [256, 100, None])
def test_post_fit_of_accelerations(block_points, noise):
    """blocks of 256 and of 100 cut the arcs [0, 150, 300] of 700 points, the default block holds them all"""
    case = _case('accelerations')
    model = case.model(_basis('accelerations', ARCS), ARCS, _noise(3) if noise else None)
    ne = case.system(model, block_points=block_points)
    x, Z, solved = _solve(ne, _signs(P, 6))
    fit = case.post(x, model=model, vectors=Z, block_points=block_points)
    label = 'accelerations, blocks of {0}, noise {1}'.format(block_points, noise)
    entries = _check_entries(fit, 'accelerations', ARCS, noise, x, Z, label=label)
    _check_consistency(fit, ne, solved, 'accelerations', ARCS, noise, x, Z, entries, label)
    assert isinstance(fit.whitened, np.ndarray) and isinstance(fit.arc_square_sums, np.ndarray) and fit.arc_parameters.shape == (3, 3, 4)
    assert np.array_equal(fit.arc_observation_counts, 3 * np.array([150, 150, 400]) - 12)
    # the parameters do not need the kept columns, the solution may be [P, 1] on the device, and a second run is bitwise the first
    discarded = ga.lstsq.ArcParameters(model.basis, ARCS, model.noise_model, keep=False)
    again = case.post(ga.engine.to_device(x[:, None]), model=discarded, vectors=ga.engine.to_device(Z), block_points=block_points)
    assert np.array_equal(again.whitened, fit.whitened) and np.array_equal(again.residuals, fit.residuals) and bool((again.rows == fit.rows).all())
    assert np.array_equal(again.arc_parameters, fit.arc_parameters) and np.array_equal(again.arc_square_sums, fit.arc_square_sums)
    assert np.array_equal(again.arc_redundancies(), fit.arc_redundancies())
    factors = fit.arc_variance_factors()
    assert factors.shape == (3,) and np.all(np.isfinite(factors)) and np.array_equal(factors, fit.arc_square_sums / fit.arc_redundancies())


@pytest.mark.parametrize('kind', ['gradients', 'line_of_sight', 'frame'])
def test_post_fit_of_the_other_kinds(kind):
    """K = 4 components with a model each and frames; K = 1; and the general basis of frame_basis (u = 12, one set per arc)"""
    case = _case(kind)
    model = case.model(_basis(kind, ARCS), ARCS, _noise(case.K))
    ne = case.system(model, block_points=256)
    x, Z, solved = _solve(ne, _signs(P, 6))
    fit = case.post(x, model=model, vectors=Z, block_points=256)
    entries = _check_entries(fit, kind, ARCS, True, x, Z, label=kind)
    _check_consistency(fit, ne, solved, kind, ARCS, True, x, Z, entries, kind)
    assert fit.arc_parameters.shape == ((3, 12) if kind == 'frame' else (3, case.K, 4))
    assert np.array_equal(fit.arc_observation_counts, case.K * np.array([150, 150, 400]) - (12 if kind == 'frame' else 4 * case.K))


def test_post_fit_without_arc_parameters():
    """ColouredNoise: the arcs of the model, no parameters; no model: one arc, and without weights whitened == residuals, bitwise"""
    case = _case('accelerations')
    model = case.model(None, ARCS, _noise(3))
    ne = case.system(model, block_points=256)
    x, Z, solved = _solve(ne, _signs(P, 6))
    fit = case.post(x, model=model, vectors=Z, block_points=256)
    reference, bound, vector_reference, vector_bound, _ = _check_entries(fit, 'accelerations', ARCS, True, x, Z, with_basis=False, label='coloured noise')
    white_A, white_l = _host_system('accelerations', tuple(ARCS), True, False)[:2]
    got, expected = float(np.sum(fit.whitened ** 2)), float(ne.residual_square_sum(x[:, None]))
    limit = _square_sum_bounds(white_A, white_l, x, reference, bound)
    print('coloured noise: square sum {0:.2e} of its bound'.format(abs(got - expected) / limit))
    assert abs(got - expected) <= limit
    assert fit.arc_parameters is None and np.array_equal(fit.ranks, np.zeros((3, 3))) and np.array_equal(fit.arcs, ARCS)
    assert np.array_equal(fit.arc_observation_counts, [450, 450, 1200]) and fit.arc_observation_counts.sum() == ne.observation_count
    single = case.post(x, model=ga.lstsq.ColouredNoise(_noise(3)), block_points=256)
    assert np.array_equal(single.arcs, [0]) and single.arc_square_sums.shape == (1,)
    with pytest.raises(ValueError, match='need the Monte-Carlo vectors'):
        single.arc_redundancies()

    xyz = ai.scattered_positions(M, 2943)
    obs = np.random.default_rng(2953).standard_normal((M, 3)) * 1e-3
    device_x = ga.engine.to_device(x)
    plain = ga.lstsq.PostFit.of_accelerations(device_x, ga.engine.to_device(xyz), obs, MIN_DEGREE, N, di.GM, di.R, block_points=256, vectors=Z)
    assert ga.lstsq._is_tensor(plain.whitened) and ga.lstsq._is_tensor(plain.residuals) and bool((plain.whitened == plain.residuals).all())
    assert np.array_equal(plain.arcs, [0]) and plain.arc_parameters is None and np.array_equal(plain.arc_observation_counts, [3 * M])
    At = ga.engine.acceleration_design(N, xyz, di.GM, di.R, MIN_DEGREE)
    A = _host(At).reshape(P, 3 * M).T
    expected = obs.T.ravel() - A @ x
    assert np.all(np.abs(_host(plain.whitened).T.ravel() - expected) <= (P + 3) * U * (np.abs(A) @ np.abs(x) + np.abs(obs.T.ravel())))


# ---- 5: the exact trace ---------------------------------------------------------------------------------------------------------------------
def test_redundancies_with_the_exact_trace():
    """d/o 4 (P = 21): with signs = sqrt(P) I the estimator is the trace itself, and arc_redundancies() is K len_a minus the diagonal
    of the hat matrix of the explicit host system over the arc, within 10 times the disagreement of the host's own two formulations.
    r_a = n_a - trace is rounded once at the size of n_a on either side, which can hide that disagreement altogether: 2 u n_a on top"""
    degree, parameters = 4, 25 - MIN_DEGREE ** 2
    case = _case('accelerations', degree)
    basis, noise = _basis('accelerations', ARCS), _noise(3)
    model = case.model(basis, ARCS, noise)
    ne = case.system(model, block_points=256)
    x, Z, solved = _solve(ne, np.sqrt(parameters) * np.eye(parameters))
    fit = case.post(x, model=model, vectors=Z, block_points=256)
    white_A, white_l, white_B = _transformed(case.At, case.root * case.obs, basis, case.root, noise, ARCS)[:3]
    bounds = arc.bounds_of(ARCS, M)
    units = arc.explicit_columns(white_B, bounds, True)
    expected = pf.hat_redundancies(pf.hat_diagonal(np.hstack([white_A] + units)), bounds, 3, M)
    host = pf.pass_redundancies(white_A, units, pf.projectors(units)[1].reshape(3, 3), bounds, 3, M)
    disagreement = np.abs(host - expected).max()
    got = fit.arc_redundancies()
    print('exact trace: redundancies {0} against the hat matrix {1}: {2:.2e}, host formulations {3:.2e}'.format(got, expected, np.abs(got - expected).max(),
                                                                                                                  disagreement))
    assert np.all(np.abs(got - expected) <= 10 * disagreement + 2 * U * fit.arc_observation_counts)
    assert round(got.sum()) == 3 * M - 36 - parameters                                            # the redundancy of the whole adjustment


# ---- 6: ranks ------------------------------------------------------------------------------------------------------------------------------
def test_ranks_of_short_and_empty_arcs():
    """arcs [0, 1, 4, 300] under four parameters per axis, the second arc with zero weights: ranks 1, 0, 4, 4"""
    xyz = np.vstack((di.positions(), ai.scattered_positions(M - 20, 2941)))
    w = _weights(M, 3, 2942, False)
    w[0], w[1:4] = 1.5, 0.0
    obs = np.random.default_rng(2954).standard_normal((M, 3)) * 1e-3
    model = ga.lstsq.ArcParameters(ga.lstsq.arc_basis(SHORT_ARCS, M, degree=1, periods=(93,)), SHORT_ARCS, _noise(3))
    ne = model.from_accelerations(xyz, obs, MIN_DEGREE, N, di.GM, di.R, weights=w, block_points=256)
    x, Z, solved = _solve(ne, _signs(P, 6))
    fit = ga.lstsq.PostFit.of_accelerations(x, xyz, obs, MIN_DEGREE, N, di.GM, di.R, weights=w, block_points=256, model=model, vectors=Z)
    assert np.array_equal(fit.ranks, np.repeat([[1], [0], [4], [4]], 3, axis=1)) and np.array_equal(fit.ranks, ne.arc_elimination.ranks)
    assert np.array_equal(fit.arc_observation_counts, [0, 9, 3 * 296 - 12, 3 * 400 - 12]) and fit.arc_observation_counts.sum() == ne.observation_count
    assert fit.arc_square_sums[1] == 0.0 and np.all(fit.arc_square_sums >= 0)
    assert np.all(fit.arc_parameters[1] == 0.0) and np.all(np.isfinite(fit.arc_parameters))
    redundancies, factors = fit.arc_redundancies(), fit.arc_variance_factors()
    print('ranks: redundancies {0}, variance factors {1}'.format(redundancies, factors))
    assert redundancies[0] <= 0 and redundancies[1] == 9
    assert np.array_equal(np.isnan(factors), redundancies <= 0) and np.isnan(factors[0]) and factors[1] == 0.0
    assert np.all(np.isfinite(factors[1:]))


# ---- 7: the covariance function, and the loop closed once ----------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['accelerations', 'gradients'])
def test_covariance_function(kind):
    """against the exact estimator on a host copy of `residuals`, within (n + 1) u sum |e_t e_(t+k)| / d_k of n pairs"""
    case = _case(kind)
    model = case.model(_basis(kind, ARCS), ARCS, _noise(case.K))
    x = _solve(case.system(model, block_points=256), _signs(P, 2))[0]
    fit = case.post(x, model=model, block_points=256)
    e = _host(fit.residuals)
    for biased in (True, False):
        c, bound, pooled, pooled_bound = pf.covariance_function(e, ARCS, 5, biased)
        got = fit.covariance_function(5, biased=biased)
        assert len(got) == 6 and all(isinstance(item, np.ndarray) and item.shape == (1, 1) for item in got)
        each = fit.covariance_function(5, per_component=True, biased=biased)
        assert len(each) == case.K and all(len(row) == 6 and all(item.shape == (1, 1) for item in row) for row in each)
        ratio = np.abs(np.array(got).ravel() - pooled) / pooled_bound
        each_ratio = np.abs(np.array(each).reshape(case.K, 6) - c) / bound
        print('{0}, biased {1}: pooled {2:.4f}, per component {3:.4f} of their bounds'.format(kind, biased, ratio.max(), each_ratio.max()))
        assert ratio.max() <= 1 and each_ratio.max() <= 1
    unbiased, biased = np.array(fit.covariance_function(5, biased=False)).ravel(), np.array(fit.covariance_function(5)).ravel()
    assert np.allclose(unbiased * pf.divisors(ARCS, M, 5, False), biased * M, rtol=8 * U, atol=0)
    assert fit.covariance_function(0)[0].shape == (1, 1) and len(fit.covariance_function(128)) == 129
    assert np.array_equal(np.array(fit.covariance_function(128)[:6]).ravel(), biased)            # lag k does not depend on maximum_lag
    with pytest.raises(ValueError, match='maximum_lag'):
        fit.covariance_function(129)


def test_the_loop_closed_once():
    """solve, residuals, arc weights and a covariance function, a new noise model, solve again: no statistical tolerance on the model"""
    case = _case('accelerations')
    model = case.model(_basis('accelerations', ARCS), ARCS, _noise(3))
    ne = case.system(model, block_points=256)
    x, Z, solved = _solve(ne, _signs(P, 6))
    fit = case.post(x, model=model, vectors=Z, block_points=256)
    function = fit.covariance_function(5)
    sequence = ga.lstsq.AutoregressiveModelSequence.from_covariance_function(function)           # positive semi-definite by construction
    assert sequence.maximum_order == 5 and ga.lstsq.whitening_taps(sequence).shape == (1, 6, 6)
    factors = fit.arc_variance_factors()
    assert factors.shape == (3,) and np.all(factors > 0)
    recoloured = case.system(ga.lstsq.ColouredNoise(sequence, ARCS), block_points=256)
    again = _host(recoloured.solve(signs=_signs(P, 2)))
    assert again.shape == (P, 1) and np.all(np.isfinite(again))
    refit = case.post(again, model=ga.lstsq.ColouredNoise(sequence, ARCS), block_points=256)
    variance = float(np.sum(_host(refit.whitened) ** 2)) / (3 * M - P)
    print('the loop closed once: arc variance factors {0}, sigma0^2 under the new model {1:.3f}'.format(factors, variance))
    assert np.isfinite(variance) and variance > 0
