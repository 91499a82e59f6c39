"""
CPU checks of the arc-wise parameters: lstsq.arc_basis and lstsq.frame_basis, the Python checks of lstsq.ArcParameters before anything
reaches the device, the argument checks of shg_segment_products before any HIP call, and the host references of
tests/golden/arc_inputs.py against each other (Schur complement, projection, numpy.linalg.lstsq of the explicit system).
"""
import ctypes

import numpy as np
import pytest

import arc_inputs as arc
import design_inputs as di
import grates_amd as ga
import los_inputs as li
import whitening_inputs as wi

U = 2.0 ** -53
ARCS = [0, 1, 4, 300]


# ---- arc_basis, frame_basis ------------------------------------------------------------------------------------------------------------
def test_arc_basis_polynomials():
    basis = ga.lstsq.arc_basis(ARCS, 700, degree=2)
    assert basis.shape == (700, 3) and basis.dtype == np.float64
    assert np.array_equal(basis[:, 0], np.ones(700))                                   # P_0 = 1
    tau = basis[:, 1]                                                                   # P_1 = tau
    for first, last in ((1, 4), (4, 300), (300, 700)):
        assert tau[first] == -1.0 and tau[last - 1] == 1.0 and np.all(np.diff(tau[first:last]) > 0)
        assert np.allclose(tau[first:last], np.linspace(-1.0, 1.0, last - first), rtol=0, atol=4 * U)
    assert tau[0] == 0.0 and np.array_equal(basis[0], [1.0, 0.0, -0.5])                # an arc of one point: tau = 0
    assert np.allclose(basis[:, 2], 1.5 * tau * tau - 0.5, rtol=0, atol=8 * U)
    assert np.array_equal(ga.lstsq.arc_basis(None, 5), ga.lstsq.arc_basis([0], 5, degree=1))
    assert ga.lstsq.arc_basis(None, 5).shape == (5, 2) and ga.lstsq.arc_basis(np.array(ARCS), 700, degree=15).shape == (700, 16)
    assert np.array_equal(ga.lstsq.arc_basis([0, 699], 700, degree=1)[-1], [1.0, 0.0])


def test_arc_basis_periods_and_times():
    basis = ga.lstsq.arc_basis(ARCS, 700, degree=0, periods=(93, 5400.0 / 5.0))
    assert basis.shape == (700, 5)
    t = np.arange(700.0)
    for i, period in enumerate((93.0, 1080.0)):
        assert np.array_equal(basis[:, 1 + 2 * i], np.cos(2 * np.pi * t / period)) and np.array_equal(basis[:, 2 + 2 * i], np.sin(2 * np.pi * t / period))
    only = ga.lstsq.arc_basis(ARCS, 700, degree=None, periods=(93,))
    assert only.shape == (700, 2) and np.array_equal(only, basis[:, 1:3])
    times = 5.0 * t + 17.0
    timed = ga.lstsq.arc_basis(ARCS, 700, degree=1, periods=(465.0,), times=times)
    assert np.allclose(timed[:, :2], ga.lstsq.arc_basis(ARCS, 700, degree=1), rtol=0, atol=4 * U)   # tau does not depend on the unit or the origin
    assert np.array_equal(timed[:, 2], np.cos(2 * np.pi * times / 465.0))
    uneven = np.cumsum(np.random.default_rng(2811).uniform(0.5, 1.5, 700))
    tau = ga.lstsq.arc_basis(ARCS, 700, degree=1, times=uneven)[:, 1]
    assert tau[4] == -1.0 and tau[299] == 1.0 and tau[0] == 0.0
    assert np.allclose(tau[4:300], 2 * (uneven[4:300] - uneven[4]) / (uneven[299] - uneven[4]) - 1, rtol=0, atol=4 * U)


def test_arc_basis_checks():
    basis = ga.lstsq.arc_basis
    for arcs in ([0, 5, 3], [1, 5], [0, 700], [], [0.5, 2.0]):
        with pytest.raises(ValueError, match='arcs must'):
            basis(arcs, 700)
    with pytest.raises(ValueError, match='must not be negative'):
        basis(None, -1)
    for degree in (-1, 1.5):
        with pytest.raises(ValueError, match='degree must be'):
            basis(None, 10, degree=degree)
    for periods in ((0.0,), (-3.0,), (np.inf,), (93.0, np.nan)):
        with pytest.raises(ValueError, match='periods must be finite and positive'):
            basis(None, 10, periods=periods)
    with pytest.raises(ValueError, match='17 columns of the arc basis: expected 1 .. 16'):
        basis(None, 10, degree=16)
    with pytest.raises(ValueError, match='18 columns'):
        basis(None, 10, degree=1, periods=range(1, 9))
    with pytest.raises(ValueError, match='0 columns'):
        basis(None, 10, degree=None)
    for times in (np.arange(9.0), np.arange(20.0).reshape(10, 2), np.full(10, np.nan)):
        with pytest.raises(ValueError, match='times must be 10 finite values'):
            basis(None, 10, times=times)
    assert ga.lstsq.MAX_ARC_PARAMETERS == 16


def test_frame_basis_against_a_loop():
    rng = np.random.default_rng(2812)
    M, u = 40, 5
    basis = rng.standard_normal((M, u))
    frames = np.linalg.qr(rng.standard_normal((M, 3, 3)))[0]
    general = ga.lstsq.frame_basis(basis, frames)
    assert general.shape == (M, 3, 3 * u)
    for t in range(M):
        for k in range(3):
            for i in range(u):
                for a in range(3):
                    assert general[t, k, 3 * i + a] == basis[t, i] * frames[t, a, k]
    # a bias b in the instrument frame is F^T b in Earth-fixed axes
    bias = rng.standard_normal(3)
    seen = np.einsum('tkj,j->tk', ga.lstsq.frame_basis(np.ones((M, 1)), frames), bias)
    assert np.allclose(seen, np.einsum('tak,a->tk', frames, bias), rtol=0, atol=8 * U * np.abs(bias).sum())
    with pytest.raises(ValueError, match='18 columns of the frame basis'):
        ga.lstsq.frame_basis(np.ones((M, 6)), frames)
    with pytest.raises(ValueError, match=r'frames must have shape \(40, 3, 3\)'):
        ga.lstsq.frame_basis(basis, frames[:-1])
    with pytest.raises(ValueError, match=r'basis must have shape \(M, u\)'):
        ga.lstsq.frame_basis(np.ones(M), frames)


# ---- ArcParameters: every check before the device ----------------------------------------------------------------------------------------
def _constructors():
    """components: the from_* call of ArcParameters(basis, ...) on five valid points"""
    xyz = di.positions()[:5]
    a, b = (x[:5] for x in li.pairs())
    bind = ga.lstsq.ArcParameters
    return {3: lambda basis, **kw: bind(basis, **kw).from_accelerations(xyz, np.ones((5, 3)), 0, 4),
            4: lambda basis, **kw: bind(basis, **kw).from_gradients(xyz, np.ones((5, 4)), 0, 4, components=('xx', 'yy', 'zz', 'xz')),
            1: lambda basis, **kw: bind(basis, **kw).from_line_of_sight(a, b, np.ones(5), 0, 4)}


def test_arc_parameters_check_before_the_device(golden):
    """every ValueError below is raised without a GPU: the checks precede require_gpu"""
    two, five = (wi.sequence(golden('g27_whitening'), name, ga.lstsq) for name in ('ar2', 'ar5'))
    bind = ga.lstsq.ArcParameters
    for shape in ((5,), (5, 3, 2, 1), ()):
        with pytest.raises(ValueError, match=r'the arc basis must have shape \(M, u\) or \(M, K, u\)'):
            bind(np.ones(shape))
    for shape in ((5, 17), (5, 3, 17), (5, 0)):
        with pytest.raises(ValueError, match='{0} parameters per arc: expected 1 .. 16'.format(shape[-1])):
            bind(np.ones(shape))
    with pytest.raises(ValueError, match='the arc basis must be finite'):
        bind(np.array([[1.0, np.nan]]))
    with pytest.raises(ValueError, match='noise_model must be'):
        bind(np.ones((5, 2)), noise_model=5)
    with pytest.raises(ValueError, match='differ in their maximum order'):
        bind(np.ones((5, 2)), noise_model=[two, five])
    for components, build in _constructors().items():
        for shape in ((6, 2), (4, 2), (5, components + 1, 2), (6, components, 2)):
            with pytest.raises(ValueError, match=r'the arc basis must have shape \(5, u\) or \(5, {0}, u\), got'.format(components)):
                build(np.ones(shape))
        for arcs in ([0, 5], [1, 2], [0, 3, 3], [0.5]):
            with pytest.raises(ValueError, match='arcs must'):
                build(np.ones((5, 2)), arcs=arcs)
            with pytest.raises(ValueError, match='arcs must'):
                build(np.ones((5, components, 2)), arcs=arcs, noise_model=five)
        with pytest.raises(ValueError, match='{0} noise models for {1} components'.format(components + 1, components)):
            build(np.ones((5, 2)), noise_model=[two] * (components + 1))
    params = bind(np.ones((5, 2)), arcs=[0, 2], noise_model=five, keep=False)
    assert params.basis.shape == (5, 2) and params.arcs == [0, 2] and params.noise_model is five and params.keep is False
    assert bind(np.ones((5, 3, 16))).keep is True


def test_signatures():
    import inspect
    assert list(inspect.signature(ga.lstsq.ArcParameters).parameters) == ['basis', 'arcs', 'noise_model', 'keep']
    assert list(inspect.signature(ga.lstsq.arc_basis).parameters) == ['arcs', 'count', 'degree', 'periods', 'times']
    assert list(inspect.signature(ga.lstsq.frame_basis).parameters) == ['basis', 'frames']
    assert list(inspect.signature(ga.engine.segment_products).parameters) == ['X', 'Bt', 'seg', 'channels', 'out']
    for name in ('from_accelerations', 'from_gradients', 'from_line_of_sight'):             # the arguments of the classmethod of the same name
        bound = [(prm.name, prm.default) for prm in list(inspect.signature(getattr(ga.lstsq.ArcParameters, name)).parameters.values())[1:]]
        plain = [(prm.name, prm.default) for prm in inspect.signature(getattr(ga.lstsq.NormalEquations, name)).parameters.values()]
        assert bound == [item for item in plain if item[0] not in ('noise_model', 'arcs')]
    assert ga.lstsq.NormalEquations.arc_elimination is None


# ---- the C entry point ---------------------------------------------------------------------------------------------------------------
def test_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    call = lib.shg_segment_products
    X, Bt, seg, S = (ctypes.c_void_p(address) for address in (0x10000000, 0x20000000, 0x30000000, 0x40000000))   # never dereferenced

    def error():
        return lib.shg_last_error().decode()
    #    rows channels M X ldx Bt ldb u nseg seg S stream
    for rows, M, ldx, ldb in ((-1, 10, 10, 10), (6, -1, 10, 10), (6, 10, -1, 10), (6, 10, 10, -1)):
        assert call(rows, 3, M, X, ldx, Bt, ldb, 4, 2, seg, S, None) == -1
        assert 'shg_segment_products: negative size' in error()
    for channels in (0, -3):
        assert call(6, channels, 10, X, 10, Bt, 10, 4, 2, seg, S, None) == -1
        assert 'channels {0} below 1'.format(channels) in error()
    assert call(7, 3, 10, X, 10, Bt, 10, 4, 2, seg, S, None) == -1
    assert 'rows 7 are not a multiple of channels 3' in error()
    for u in (0, -1, 17):
        assert call(6, 3, 10, X, 10, Bt, 10, u, 2, seg, S, None) == -1
        assert 'u {0} outside 1 .. 16'.format(u) in error()
    assert call(6, 3, 10, X, 10, Bt, 10, 4, -1, seg, S, None) == -1
    assert 'nseg -1 is negative' in error()
    assert call(6, 3, 10, X, 9, Bt, 10, 4, 2, seg, S, None) == -1
    assert 'ldx 9 below M 10' in error()
    assert call(6, 3, 10, X, 10, Bt, 9, 4, 2, seg, S, None) == -1
    assert 'ldb 9 below M 10' in error()
    for pointers in ((None, Bt, seg, S), (X, None, seg, S), (X, Bt, None, S), (X, Bt, seg, None)):
        assert call(6, 3, 10, pointers[0], 10, pointers[1], 10, 4, 2, pointers[2], pointers[3], None) == -1
        assert 'shg_segment_products: NULL pointer' in error()
    assert call((1 << 20) + 1, 1, 1 << 20, X, 1 << 20, Bt, 1 << 20, 4, 2, seg, S, None) == -1             # 2^40 + 2^20 values of X
    assert 'values of X are too large' in error()
    assert call(1 << 20, 1, 4, X, 4, Bt, 4, 16, (1 << 16) + 1, seg, S, None) == -1                         # ... of S alone
    assert 'values of S are too large' in error()
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(0, 3, 10, None, 10, None, 10, 4, 2, None, None, None) == 0
    assert call(6, 3, 10, None, 10, None, 10, 4, 0, None, None, None) == 0
    with pytest.raises(_lib.ShgError, match='u 17 outside 1 .. 16'):
        _lib.call('shg_segment_products', 6, 3, 10, X, 10, Bt, 10, 17, 2, seg, S, None)


# ---- the host references against each other ------------------------------------------------------------------------------------------------
def test_host_formulations_agree_on_well_conditioned_arcs():
    """arcs [0, 150, 300]: cond(G) is small, so the Schur complement loses nothing against the projection: N, n and lPl agree within the
    bounds 2 L u sqrt(N_ii N_jj) (...) of dot products of length L = K M with the diagonals of the unreduced normals.  The solution
    against lstsq of the explicit system: within arc_inputs.solution_bound."""
    A, l, units, _, _ = arc.host_case([0, 150, 300])
    assert A.shape == (2100, 169) and len(units) == 9 and units[0].shape == (2100, 4)
    cond = arc.conditions(units).max()
    N, n, lPl, count, ranks, parameters = arc.schur(A, l, units)
    Np, np_, lPlp = arc.projection(A, l, units)
    bound_N, bound_n, bound_l = arc.normals_bounds(A, l)
    print('cond(G) {0:.2f}; N {1:.4f}, n {2:.4f}, lPl {3:.4f} of their bounds'.format(cond, (np.abs(N - Np) / bound_N).max(), (np.abs(n - np_) / bound_n).max(),
                                                                                      abs(lPl - lPlp) / bound_l))
    assert cond <= 100
    assert np.all(np.abs(N - Np) <= bound_N) and np.all(np.abs(n - np_) <= bound_n) and abs(lPl - lPlp) <= bound_l
    assert np.array_equal(ranks, np.full(9, 4)) and count == 2100 - 36
    assert np.abs(N - A.T @ A).max() > 1e6 * bound_N.max()                                    # the elimination does change the normals
    x, y = arc.explicit_solution(A, l, units)
    xs = np.linalg.solve(N, n)
    bound = arc.solution_bound(A, N, units)
    print('x against lstsq: {0:.2e} (bound {1:.2e})'.format(np.linalg.norm(xs - x) / np.linalg.norm(x), bound))
    assert np.linalg.norm(xs - x) <= bound * np.linalg.norm(x)
    assert np.linalg.norm(parameters(xs) - y) <= bound * cond * np.linalg.norm(y)
    residual = l - A @ x - np.hstack(units) @ y.ravel()
    assert abs((lPl - n @ xs) - residual @ residual) <= bound * lPl                           # the square sum of the residuals of the joint system


def test_host_formulations_agree_on_short_arcs():
    """arcs [0, 1, 4, 300]: four parameters on one point and on three; the ranks per channel are 1, 3, 4, 4, and the solution still
    agrees with lstsq.  On the three points the period of 93 samples is nearly the constant and the drift, so cond(G) over the kept
    eigenvalues is large and the cancellation in N - D D^T shows: N itself is not compared here, the solution is, within
    arc_inputs.solution_bound."""
    A, l, units, _, _ = arc.host_case(ARCS)
    N, n, lPl, count, ranks, parameters = arc.schur(A, l, units)
    assert np.array_equal(ranks.reshape(4, 3), np.repeat([[1], [3], [4], [4]], 3, axis=1)) and count == 2100 - 36
    x, y = arc.explicit_solution(A, l, units)
    xs = np.linalg.solve(N, n)
    bound = arc.solution_bound(A, N, units)
    print('x against lstsq: {0:.2e} (bound {1:.2e}); cond(G) up to {2:.1e}'.format(np.linalg.norm(xs - x) / np.linalg.norm(x), bound,
                                                                                     arc.conditions(units).max()))
    assert np.linalg.norm(xs - x) <= bound * np.linalg.norm(x)
    ys = parameters(xs)
    assert ys.shape == y.shape == (12, 4)
    for unit in range(6):                                                                     # the dropped directions carry nothing
        G = units[unit].T @ units[unit]
        null = np.linalg.eigh(G)[1][:, :4 - ranks[unit]]
        assert np.abs(null.T @ ys[unit]).max() <= 64 * U * np.abs(ys[unit]).max()
