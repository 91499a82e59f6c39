"""
Observation leverages and Huber reweighting on the GPU: the kernel of shg_leverages (engine.leverages) against an np.longdouble oracle
on host copies, bitwise wherever a column lies; PostFit.leverages / redundancies / standardised for the kinds of observation and the
stochastic models against NumPy on host copies of the device's U and A~ and against the hat diagonal of a host QR of the full whitened
model; lstsq.huber_factors, huber_iterate and robust_least_squares against a fixture recorded from the reference and a NumPy IRLS.
"""
import ctypes
import functools

import numpy as np
import pytest

import grates_amd as ga
import leverage_inputs as lev

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = -7.25


def _host(t):
    return ga.engine.to_host(t) if ga.lstsq._is_tensor(t) else np.asarray(t)


# ---- 1: the kernel ----------------------------------------------------------------------------------------------------------------------
def _call(n, cols, Ui_d, ldu, X_d, ldx, out_d, offset=0):
    """shg_leverages on the columns offset .. offset + cols of X_d, straight through the C ABI: the leading dimensions are the caller's"""
    from grates_amd import _lib
    _lib.call('shg_leverages', n, cols, ctypes.c_void_p(Ui_d.data_ptr()), ldu, ctypes.c_void_p(X_d.data_ptr() + 8 * offset), ldx,
              ctypes.c_void_p(out_d.data_ptr()), ga.engine._stream())


@functools.lru_cache(maxsize=None)
def _kernel_case(n):
    """Ui [n, n + 3] upper triangular with NaN below the diagonal and in the padding, X [n, 300 + 5] with NaN padding, the longdouble
    reference [300] and the magnitude sum_p (sum_q |Ui_qp| |X_qj|)^2 of the issue's bound"""
    rng = np.random.default_rng(4240 + n)
    Ui = np.triu(rng.standard_normal((n, n))) / np.sqrt(n)
    X = rng.standard_normal((n, 300))
    reference, magnitude = lev.exact_leverages(Ui, X)
    Ui_pad = np.full((n, n + 3), np.nan)
    Ui_pad[:, :n] = np.where(np.tri(n, k=-1, dtype=bool), np.nan, Ui)
    X_pad = np.full((n, 305), np.nan)
    X_pad[:, :300] = X
    return Ui, X, reference, magnitude, ga.engine.to_device(Ui_pad), ga.engine.to_device(X_pad)


@pytest.mark.parametrize('n', [1, 4, 127, 128, 129, 257])
def test_kernel_against_longdouble(n):
    """entry-wise within (3 n + 4) u sum_p (sum_q |Ui_qp| |X_qj|)^2, the first-order rounding bound of the dot products, the squares and the
    sum, for cols in {1, 63, 64, 65, 128, 129, 300}; ldu > n, ldx > cols, NaN in the padding and below the diagonal; the guard behind
    out stays; two calls give equal bits"""
    import torch
    Ui, X, reference, magnitude, Ui_d, X_d = _kernel_case(n)
    worst = 0.0
    for cols in (1, 63, 64, 65, 128, 129, 300):
        out = torch.full((cols + 7,), GUARD, dtype=torch.float64, device=Ui_d.device)
        _call(n, cols, Ui_d, n + 3, X_d, 305, out)
        got = _host(out)
        assert np.all(got[cols:] == GUARD)
        assert np.all(np.isfinite(got[:cols]))
        bound = (3 * n + 4) * U * magnitude[:cols]
        worst = max(worst, float((np.abs(got[:cols] - reference[:cols]) / bound).max()))
        assert np.all(np.abs(got[:cols] - reference[:cols]) <= bound)
        again = torch.full((cols + 7,), GUARD, dtype=torch.float64, device=Ui_d.device)
        _call(n, cols, Ui_d, n + 3, X_d, 305, again)
        assert bool((again == out).all())
    print('n {0}: {1:.2e} of the bound'.format(n, worst))
    # the wrapper on views: the same bits
    by_wrapper = ga.engine.leverages(Ui_d[:, :n], X_d[:, :300])
    full = torch.empty(300, dtype=torch.float64, device=Ui_d.device)
    _call(n, 300, Ui_d, n + 3, X_d, 305, full)
    assert bool((by_wrapper == full).all())


@pytest.mark.parametrize('n', [1, 4, 127, 128, 129, 257])
def test_identity_gives_the_column_square_sums(n):
    """Ui = I (NaN below the diagonal): out[j] = sum_q X_qj^2 within the same bound, whose magnitude is then the sum itself; the matrix is
    asymmetric, so a transposed operand would show"""
    _, X, _, _, _, X_d = _kernel_case(n)
    identity = np.where(np.tri(n, k=-1, dtype=bool), np.nan, np.eye(n))
    got = _host(ga.engine.leverages(ga.engine.to_device(identity), X_d[:, :300]))
    sums = np.sum(X.astype(np.longdouble) ** 2, axis=0)
    assert np.all(np.abs(got - sums) <= (3 * n + 4) * U * sums.astype(np.float64))


def test_upper_triangle_is_used_not_its_transpose():
    """one entry above the diagonal: z = Ui^T x, so out[j] = x_0^2 + (x_1 + 3 x_0)^2, exactly in small integers"""
    Ui = np.array([[1.0, 3.0], [np.nan, 1.0]])
    X = np.array([[1.0, 2.0, 0.0], [0.0, 1.0, 5.0]])
    got = _host(ga.engine.leverages(ga.engine.to_device(Ui), ga.engine.to_device(X)))
    assert np.array_equal(got, [1.0 + 9.0, 4.0 + 49.0, 25.0])


@pytest.mark.parametrize('n', [4, 129, 257])
def test_a_column_gives_the_same_bits_wherever_it_lies(n):
    """a column alone, and the same column at offsets 0, 1, 63 and 129 inside a batch of 300 (odd offsets: rows that are not 16-byte
    aligned), give equal bits"""
    import torch
    _, X, _, _, Ui_d, X_d = _kernel_case(n)
    whole = torch.empty(300, dtype=torch.float64, device=Ui_d.device)
    _call(n, 300, Ui_d, n + 3, X_d, 305, whole)
    whole = _host(whole)
    for j in (0, 1, 63, 129, 299):
        alone = torch.empty(1, dtype=torch.float64, device=Ui_d.device)
        _call(n, 1, Ui_d, n + 3, X_d, 305, alone, offset=j)
        assert _host(alone)[0] == whole[j]
    column = X[:, 17]
    for offset in (0, 1, 63, 129):
        batch = np.random.default_rng(4250 + offset).standard_normal((n, 200))
        batch[:, offset] = column
        got = _host(ga.engine.leverages(Ui_d[:, :n], ga.engine.to_device(batch)))
        assert got[offset] == whole[17]


def test_empty_sizes():
    import torch
    out = torch.full((5,), GUARD, dtype=torch.float64, device=ga.engine.device())
    empty = torch.empty((0, 5), dtype=torch.float64, device=out.device)
    assert ga.engine.leverages(torch.empty((0, 0), dtype=torch.float64, device=out.device), empty, out=out) is out
    assert bool((out == 0.0).all())                                                               # an empty sum
    assert tuple(ga.engine.leverages(torch.eye(3, dtype=torch.float64, device=out.device), empty.reshape(3, 0)).shape) == (0,)


# ---- 2: leverages through PostFit ----------------------------------------------------------------------------------------------------------
M, MIN_DEGREE, MAX_DEGREE = 300, 2, 8
P = (MAX_DEGREE + 1) ** 2 - MIN_DEGREE ** 2
ARCS = [0, 150]
GOCE = ('xx', 'yy', 'zz', 'xz')
BAND = (MIN_DEGREE, MAX_DEGREE, lev.GM, lev.R)


def _ar2():
    """an AutoregressiveModelSequence of orders 0 .. 2 with seeded coefficients and variances"""
    import whitening_inputs as wi
    return wi.synthetic_sequence(ga.lstsq, 2, 4269)


def _signs(parameters, count=2, seed=4270):
    return np.where(np.random.default_rng(seed).integers(0, 2, (parameters, count)) == 1, 1.0, -1.0)


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(4271)
    xyz = lev.sphere_positions(M, 4272)
    g = rng.standard_normal((M, 3)) * 1e-6
    zeros = rng.uniform(0.25, 4.0, M)
    zeros[[0, 7, 99, 100, 149, 150, 299]] = 0.0
    return xyz, g, zeros


def _models():
    import gradient_design_inputs as gdi
    shared = ga.lstsq.arc_basis(ARCS, M, degree=1)
    return {'white': (None, None), 'zeros': (None, 'zeros'), 'coloured': (ga.lstsq.ColouredNoise(_ar2(), ARCS), None),
            'shared': (ga.lstsq.ArcParameters(shared, ARCS), 'zeros'),
            'general': (ga.lstsq.ArcParameters(ga.lstsq.frame_basis(shared, gdi.frames(M, 4273)), ARCS, _ar2()), None),
            'regularised': (None, None)}


def _host_operands(fit):
    """host copies of what the device holds: the rows A~ [K M, P] of the fit's design blocks (one block of all points), and under
    ArcParameters the units E [K M, u] of B~ with the R of the fit's own reduction"""
    observations, model, _, setup, _ = fit._PostFit__bound
    blocks = [At for _, _, At, _, _, _ in ga.lstsq._design_blocks(observations, model, observations.M)]
    assert len(blocks) == 1
    A = _host(blocks[0]).T.copy()
    if setup is None:
        return A, None, 0
    import arc_inputs as arc
    B = np.ascontiguousarray(_host(setup.Bt).transpose(1, 2, 0))                                     # [K, M, u]
    units = arc.explicit_columns(B, setup.bounds, setup.shared)
    Q = np.hstack([E @ R for E, R in zip(units, setup.R)])                                           # zero columns along dropped directions
    longest = int(np.diff(setup.bounds).max()) * observations.K
    return A, Q, longest


def _check_leverages(fit, normals, label, elimination=None, own=True, extra_rows=None, ranks=0):
    """both oracles, the range, the sum and that the calls leave `whitened` alone; returns h [M, K]"""
    before = _host(fit.whitened).copy()
    h = _host(fit.leverages(normals, elimination))
    r = _host(fit.redundancies(normals, elimination))
    K = h.shape[1]
    assert h.shape == (M, K) and np.array_equal(r, 1.0 - h) and np.array_equal(_host(fit.whitened), before)
    A, Q, longest = _host_operands(fit)
    factor = np.triu(normals.matrix[0, 0])
    first, bound = lev.hat_by_normals(A, factor, Q, longest)
    got = h.T.ravel()
    ratio = np.abs(got - first) / np.where(bound > 0, bound, 1.0)
    full = A if Q is None else np.hstack((A, Q[:, np.any(Q != 0.0, axis=0)]))
    if extra_rows is not None:
        full = np.vstack((full, extra_rows))
    second = lev.hat_by_qr(full)[0][:A.shape[0]]
    disagreement = float(np.abs(first - second).max())
    tolerance = max(10.0 * disagreement, 1e-12)
    print('{0}: {1:.3f} of the dot-product bound; against the QR route {2:.2e}, the host routes differ by {3:.2e}'.format(
        label, ratio.max(), np.abs(got - second).max(), disagreement))
    assert ratio.max() <= 1
    assert np.abs(got - second).max() <= tolerance
    assert got.min() >= 0.0 and got.max() <= 1.0 + tolerance
    if own:
        assert abs(got.sum() - (A.shape[1] + ranks)) <= (A.shape[1] + ranks) * tolerance + bound.sum()
    return h


@pytest.mark.parametrize('block_points', [100, None])
@pytest.mark.parametrize('name', ['white', 'zeros', 'coloured', 'shared', 'general', 'regularised'])
def test_leverages_of_accelerations(name, block_points):
    """300 accelerations, degrees 2 .. 8 (P = 77, 900 rows) on a sphere of 6.8e6 m; blocks of 100 cut the arcs [0, 150], the default
    block holds all points.  Measured (MI355X): the table of DESIGN.md section 4.24."""
    xyz, g, zeros = _inputs()
    model, weights = _models()[name]
    w = zeros if weights == 'zeros' else None
    owner = ga.lstsq.NormalEquations if model is None else model
    ne = owner.from_accelerations(xyz, g, *BAND, weights=w, block_points=block_points)
    elimination, extra, own, ranks = None, None, True, 0
    if name == 'regularised':
        vector = np.full(P, 1e-3 * float(np.trace(ne.matrix[0, 0])) / P)
        ne = ga.lstsq.accumulate_normals([ne, ga.lstsq.TikhonovRegularization(vector, [0, P])], [1.0, 1.0])
        extra, own = np.diag(np.sqrt(vector)), False
    if ne.arc_elimination is not None:
        ranks = ne.arc_elimination.count
    x = ne.solve(signs=_signs(P))
    fit = ga.lstsq.PostFit.of_accelerations(x, xyz, g, *BAND, weights=w, block_points=block_points, model=model)
    label = '{0}, blocks of {1}'.format(name, block_points)
    h = _check_leverages(fit, ne, label, elimination, own, extra, ranks)
    if name == 'zeros':
        assert np.all(h[zeros == 0.0] == 0.0)                                                     # exactly: the rows are zero
    if name == 'shared':                                                                          # a combined system has no elimination of its own
        combined = ga.lstsq.accumulate_normals([owner.from_accelerations(xyz, g, *BAND, weights=w, block_points=block_points)], [1.0])
        combined.solve(signs=_signs(P))
        with pytest.raises(ValueError, match='pass elimination'):
            fit.leverages(combined)
        again = _host(fit.leverages(combined, ne.arc_elimination))
        assert np.allclose(again, h, rtol=0, atol=1e-12)
    # standardised: the definition on the host copies, entry-wise
    t = _host(fit.standardised(ne))
    e = _host(fit.whitened)
    sigma = np.sqrt(np.sum(e * e) / (ne.observation_count - P))
    with np.errstate(invalid='ignore', divide='ignore'):
        expected = np.where(1.0 - h > 0, np.abs(e) / (sigma * np.sqrt(np.where(1.0 - h > 0, 1.0 - h, 1.0))), np.nan)
    assert np.allclose(t, expected, rtol=1e-12, atol=0, equal_nan=True)            # a few roundings per entry and a sum of 900 squares
    halved = _host(fit.standardised(ne, sigma=2.0 * sigma, factors=np.full(M, 0.25)))
    assert np.allclose(halved, expected, rtol=1e-12, atol=0, equal_nan=True)


@pytest.mark.parametrize('kind', ['line_of_sight', 'gradients', 'radial_basis'])
def test_leverages_of_the_other_kinds(kind):
    """K = 1, K = 4 with frames and per-component weights, and the node values of 40 radial basis functions as the parameters"""
    import gradient_design_inputs as gdi
    import los_inputs as li
    import rbf_inputs as ri
    rng = np.random.default_rng(4274)
    xyz, _, zeros = _inputs()
    if kind == 'line_of_sight':
        b = xyz + 2.0e5 * li.unit_vectors(M, 4275)
        obs = rng.standard_normal(M) * 1e-7
        ne = ga.lstsq.NormalEquations.from_line_of_sight(xyz, b, obs, *BAND, weights=zeros)
        x = ne.solve(signs=_signs(P))
        fit = ga.lstsq.PostFit.of_line_of_sight(x, xyz, b, obs, *BAND, weights=zeros)
    elif kind == 'gradients':
        frames, obs, w = gdi.frames(M, 4276), rng.standard_normal((M, 4)) * 1e-9, rng.uniform(0.25, 4.0, (M, 4))
        ne = ga.lstsq.NormalEquations.from_gradients(xyz, obs, *BAND, frames=frames, components=GOCE, weights=w, block_points=128)
        x = ne.solve(signs=_signs(P))
        fit = ga.lstsq.PostFit.of_gradients(x, xyz, obs, *BAND, frames=frames, components=GOCE, weights=w, block_points=128)
    else:
        lon, lat = ri.scattered_nodes(40, 4277)
        k = ri.degree_factors(MIN_DEGREE, MAX_DEGREE)
        basis = ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat, a=ri.A, f=ri.F), ri.shape_factors(k), MIN_DEGREE, MAX_DEGREE, ri.GM, ri.R)
        bound, obs = ga.lstsq.RadialBasisParameters(basis), rng.standard_normal((M, 3)) * 1e-6
        ne = bound.from_accelerations(xyz, obs, weights=zeros, block_points=128)
        x = ne.solve(signs=_signs(40))
        fit = bound.of_accelerations(x, xyz, obs, weights=zeros, block_points=128)
    h = _check_leverages(fit, ne, kind)
    assert h.shape == (M, {'line_of_sight': 1, 'gradients': 4, 'radial_basis': 3}[kind])


def test_leverages_stay_on_the_device_with_the_positions():
    xyz, g, _ = _inputs()
    ne = ga.lstsq.NormalEquations.from_accelerations(xyz, g, *BAND)
    x = ne.solve(signs=_signs(P))
    fit = ga.lstsq.PostFit.of_accelerations(x, ga.engine.to_device(xyz), g, *BAND)
    h, r, t = fit.leverages(ne), fit.redundancies(ne), fit.standardised(ne)
    assert all(ga.lstsq._is_tensor(v) and tuple(v.shape) == (M, 3) for v in (h, r, t))
    assert bool((fit.leverages(ne) == h).all())
    kept = h.clone()
    h.zero_()                                                                                     # what a call returns is the caller's own
    assert bool((fit.redundancies(ne) == r).all()) and bool((fit.leverages(ne) == kept).all())


# ---- 3: Huber, explicit ------------------------------------------------------------------------------------------------------------------
def test_robust_least_squares_against_the_reference(golden):
    """orthonormal columns and max_iter=1: the one setting in which the reference's formulas are the textbook ones.  x_hat and C within
    the rounding of the two routes (the normals of orthonormal columns are well conditioned: 1e-12 relative is ample), flags equal"""
    data = golden('g32_robust')
    l, A, truth, planted = lev.robust_problem(True)
    assert np.array_equal(data['l'], l) and np.array_equal(data['A'], A)
    assert np.array_equal(np.flatnonzero(data['outlier_flag']), planted)
    x_hat, C, flags = ga.lstsq.robust_least_squares(l, A, max_iter=1)
    assert isinstance(x_hat, np.ndarray) and x_hat.shape == (6,) and C.shape == (6, 6) and flags.shape == (200,) and flags.dtype == bool
    print('reference: x_hat {0:.2e}, C {1:.2e}'.format(np.abs(x_hat - data['x_hat']).max() / np.abs(data['x_hat']).max(),
                                                        np.abs(C - data['C']).max() / np.abs(data['C']).max()))
    assert np.abs(x_hat - data['x_hat']).max() <= 1e-12 * np.abs(data['x_hat']).max()
    assert np.abs(C - data['C']).max() <= 1e-12 * np.abs(data['C']).max()
    assert np.array_equal(flags, data['outlier_flag'])


def test_robust_least_squares_against_numpy_irls():
    """a general A, max_iter = 1 .. 10: device flags == oracle flags == planted set at every max_iter, and the solution within 1e-9 of
    the oracle's of the same iteration (both routes are backward stable on a problem of condition ~ 12; the Huber map is smooth away
    from the threshold, which no observation comes nearer to than 0.7 %; from iteration 8 on the device has stopped at
    HUBER_TOLERANCE and the 1e-9 rests on the argument there, not on a derived figure).  robust_least_squares returns no factors:
    they are checked through C = sigma0^2 N^-1 at max_iter=3, which holds the factors of two iterations, and through huber_factors
    on the device applied to the oracle's own t and r of one step.  The robust solution is closer to the truth than the plain one"""
    l, A, truth, planted = lev.robust_problem(False)
    history = lev.irls(l, A)
    assert len(history) == 10 and all(np.array_equal(np.flatnonzero(step['flags']), planted) for step in history)
    for iterations in range(1, 11):
        x_hat, C, flags = ga.lstsq.robust_least_squares(l, A, max_iter=iterations)
        step = history[iterations - 1]
        assert np.array_equal(np.flatnonzero(flags), planted)
        assert np.abs(x_hat - step['x']).max() <= 1e-9 * np.abs(step['x']).max()
    device = ga.lstsq.robust_least_squares(ga.engine.to_device(l), ga.engine.to_device(A))
    assert all(ga.lstsq._is_tensor(v) for v in device) and np.array_equal(_host(device[0]), x_hat)
    plain = np.linalg.lstsq(A, l, rcond=None)[0]
    print('IRLS: |x - truth| {0:.3f} plain, {1:.3f} robust; sigma0 {2:.2f} -> {3:.2f}'.format(
        np.linalg.norm(plain - truth), np.linalg.norm(x_hat - truth), history[0]['sigma0'], history[-1]['sigma0']))
    assert np.linalg.norm(x_hat - truth) < np.linalg.norm(plain - truth)
    C3 = ga.lstsq.robust_least_squares(l, A, max_iter=3)[1]                                        # sigma0^2 N^-1 under the weights of iteration 3
    N = (A * history[1]['factors'][:, None]).T @ A
    assert np.abs(C3 - history[2]['sigma0'] ** 2 * np.linalg.inv(N)).max() <= 1e-10 * np.abs(C3).max()
    # the factors of one step: huber_factors on the oracle's t and r, on the device
    f, o = ga.lstsq.huber_factors(ga.engine.to_device(history[3]['t']), ga.engine.to_device(history[3]['r']), ga.engine.to_device(history[2]['factors']))
    assert np.array_equal(_host(o), history[3]['flags']) and np.allclose(_host(f), history[3]['factors'], rtol=1e-14, atol=0)


# ---- 4: Huber, through the observations ----------------------------------------------------------------------------------------------------
def test_huber_iterate_through_the_observations():
    """the 900-row acceleration case under ArcParameters (bias and drift per axis and arc) with five planted spikes: huber_iterate flags
    exactly the rows the host IRLS of the explicit model [A B] flags, leaves the others at factor 1 and stops before max_iter"""
    import arc_inputs as arc
    xyz, _, _ = _inputs()
    rng = np.random.default_rng(4278)
    noise = lev.clean_noise(rng, (M, 3), cut=1.6) * 1e-6        # (sigma0 of 811 degrees of freedom comes out below 1)
    spikes = [(17, 0), (58, 2), (99, 1), (140, 0), (181, 2)]
    for (i, k), size in zip(spikes, (20.0, -22.5, 25.0, -27.5, 30.0)):
        noise[i, k] += size * 1e-6
    basis = ga.lstsq.arc_basis(ARCS, M, degree=1)
    model = ga.lstsq.ArcParameters(basis, ARCS)
    calls = []

    def system(w):
        calls.append(w)
        return model.from_accelerations(xyz, noise, *BAND, weights=w)

    def post_fit(x, w, ne):
        return ga.lstsq.PostFit.of_accelerations(x, xyz, noise, *BAND, weights=w, model=model)
    x, ne, factors, outliers = ga.lstsq.huber_iterate(system, post_fit, np.ones((M, 3)))
    assert len(calls) < 10 and factors.shape == (M, 3) and outliers.shape == (M, 3) and outliers.dtype == bool
    A = _host(ga.engine.acceleration_design(MAX_DEGREE, xyz, lev.GM, lev.R, MIN_DEGREE)).reshape(P, 3 * M).T
    E = np.hstack(arc.explicit_columns(arc.transformed_basis(basis, None, 3), arc.bounds_of(ARCS, M), True))
    history = lev.irls(noise.T.ravel(), A, extra=E)
    expected = history[-1]['flags'].reshape(3, M).T
    print('huber_iterate: {0} solutions, {1} flagged, oracle {2}'.format(len(calls), int(outliers.sum()), int(expected.sum())))
    assert np.array_equal(outliers, expected)
    assert sorted(zip(*np.nonzero(outliers))) == sorted(spikes)
    assert np.all(factors[~outliers] == 1.0) and np.all(factors[outliers] < 0.01)
    assert np.allclose(factors, history[-1]['factors'].reshape(3, M).T, rtol=1e-5, atol=0)
