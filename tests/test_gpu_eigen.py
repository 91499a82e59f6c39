"""
Dense eigen and singular value decompositions on the GPU: shg_jacobi_svd through the C ABI at the seams of the pairing (odd c), of the
wave width and of the LDS limit, with padded leading dimensions, guard bands and the error bounds of DESIGN.md section 4.28 in
numpy.longdouble; engine.syev on the four kinds of matrix; lstsq.teigh on both routes, lstsq.trsvd against the recorded errors of the
reference's own trsvd (tests/golden/g34_trsvd_reference.json) and lstsq.UnscentedTransformSymmetric against the reference's formulas.
Every figure is printed before it is asserted (pytest -s shows them).
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import grates_amd as ga
import eigen_reference as er

pytestmark = pytest.mark.gpu

GUARD = -7.25
TAIL = 64


def _torch():
    return ga.engine._torch()


# ---- 1: the kernel through the C ABI -----------------------------------------------------------------------------------------------------
def _padded(values, rows, cols, ld, stride, batch):
    """host buffer [batch * stride + TAIL]: the matrices at [b * stride + i * ld + j], NaN in every padding, GUARD behind the last"""
    buf = np.full(batch * stride + TAIL, np.nan)
    buf[batch * stride:] = GUARD
    for b in range(batch):
        for i in range(rows):
            buf[b * stride + i * ld:b * stride + i * ld + cols] = values[b, i]
    return buf


def _matrices(buf, rows, cols, ld, stride, batch):
    return np.stack([np.stack([buf[b * stride + i * ld:b * stride + i * ld + cols] for i in range(rows)]) for b in range(batch)])


def _mask(rows, cols, ld, stride, batch):
    """True where the buffer of _padded holds a matrix entry"""
    mask = np.zeros(batch * stride + TAIL, dtype=bool)
    for b in range(batch):
        for i in range(rows):
            mask[b * stride + i * ld:b * stride + i * ld + cols] = True
    return mask


def _run_kernel(G, max_sweeps=30):
    """shg_jacobi_svd on G [batch, r, c] with ldg = c + 3, ldv = c + 2 and gaps between the matrices -> host (G_out, V, sigma, sweeps)
    after the checks of everything the call must not touch"""
    from grates_amd import _lib
    torch = _torch()
    batch, r, c = G.shape
    ldg, ldv = c + 3, c + 2
    sg, sv = r * ldg + 5, c * ldv + 7
    g0 = _padded(G, r, c, ldg, sg, batch)
    v0 = _padded(np.full((batch, c, c), np.nan), c, c, ldv, sv, batch)
    s0 = np.concatenate([np.full(batch * c, np.nan), np.full(TAIL, GUARD)])
    g_d, v_d, s_d = (ga.engine.to_device(x) for x in (g0, v0, s0))
    n_d = torch.full((batch + TAIL,), -77, dtype=torch.int32, device=g_d.device)
    _lib.call('shg_jacobi_svd', ctypes.c_void_p(g_d.data_ptr()), ldg, sg, ctypes.c_void_p(v_d.data_ptr()), ldv, sv, ctypes.c_void_p(s_d.data_ptr()),
              r, c, batch, max_sweeps, ctypes.c_void_p(n_d.data_ptr()), ga.engine._stream())
    g1, v1, s1, n1 = ga.engine.to_host(g_d), ga.engine.to_host(v_d), ga.engine.to_host(s_d), n_d.cpu().numpy()
    for before, after, mask in ((g0, g1, _mask(r, c, ldg, sg, batch)), (v0, v1, _mask(c, c, ldv, sv, batch))):
        assert np.array_equal(before.view(np.int64)[~mask], after.view(np.int64)[~mask]), 'padding or guard band overwritten'
        assert np.isfinite(after[mask]).all()
    assert np.array_equal(s1[batch * c:], np.full(TAIL, GUARD)) and np.isfinite(s1[:batch * c]).all()
    assert (n1[batch:] == -77).all()
    return _matrices(g1, r, c, ldg, sg, batch), _matrices(v1, c, c, ldv, sv, batch), s1[:batch * c].reshape(batch, c), n1[:batch]


KERNEL_CASES = [(n, n, 1) for n in (1, 2, 3, 63, 64, 65, 127, 128)] + [(128, 5, 1), (7, 7, 3)]


@pytest.mark.parametrize('r,c,batch', KERNEL_CASES)
def test_kernel(r, c, batch):
    G = np.stack([er.matrix('general', c, 4100 + 10 * r + c + b, rows=r) for b in range(batch)])
    Go, V, sigma, sweeps = _run_kernel(G)
    again = _run_kernel(G)
    for first, second in zip((Go, V, sigma, sweeps), again):
        assert np.array_equal(first, second), 'two calls differ'
    for b in range(batch):
        assert 1 <= sweeps[b] <= 30
        bound = er.bound(int(sweeps[b]), c)
        figures = er.svd_figures(G[b], Go[b], V[b], sigma[b])
        lapack = er.lapack_svd_figures(G[b])
        print('\njacobi r={0} c={1} b={2}: sweeps {3}, |VtV-I| {4:.2e}, |GV-Gout|/|G| {5:.2e}, dsigma/smax {6:.2e}, bound {7:.2e}, LAPACK {8:.2e} {9:.2e}'
              .format(r, c, b, sweeps[b], *figures, bound, *lapack))
        assert np.abs(sigma[b] - np.sqrt((Go[b] * Go[b]).sum(axis=0))).max() <= 4 * er.U * r * sigma[b].max()        # the column norms of the final G
        assert figures[0] <= bound and figures[1] <= bound and figures[2] <= bound, (figures, bound)


def test_kernel_edges():
    """a zero column stays zero with a unit vector in V; non-finite input ends after one sweep, in bounds (the guard checks of _run_kernel)"""
    G = er.matrix('general', 6, 4300, rows=9)[None]
    G[0, :, 2] = 0.0
    Go, V, sigma, sweeps = _run_kernel(G)
    assert (Go[0, :, 2] == 0.0).all() and sigma[0, 2] == 0.0 and abs(np.linalg.norm(V[0, :, 2]) - 1.0) <= er.bound(int(sweeps[0]), 6)
    from grates_amd import _lib
    torch = _torch()
    bad = ga.engine.to_device(np.where(np.arange(54).reshape(9, 6) == 20, np.nan, er.matrix('general', 6, 4301, rows=9)))
    guard = torch.full((64,), GUARD, dtype=torch.float64, device=bad.device)
    V_d, s_d, n_d = torch.cat([torch.zeros(36, dtype=torch.float64, device=bad.device), guard]), torch.cat([guard[:6] * 0, guard]), torch.zeros(1, dtype=torch.int32, device=bad.device)
    _lib.call('shg_jacobi_svd', ctypes.c_void_p(bad.data_ptr()), 6, 54, ctypes.c_void_p(V_d.data_ptr()), 6, 36, ctypes.c_void_p(s_d.data_ptr()), 9, 6, 1, 30,
              ctypes.c_void_p(n_d.data_ptr()), ga.engine._stream())
    assert int(n_d.item()) == 1 and (V_d[36:] == GUARD).all() and (s_d[6:] == GUARD).all()
    with pytest.raises(ga._lib.ShgError, match='outside 1 .. 128'):
        _lib.call('shg_jacobi_svd', ctypes.c_void_p(bad.data_ptr()), 129, 0, ctypes.c_void_p(V_d.data_ptr()), 129, 0, ctypes.c_void_p(s_d.data_ptr()), 129, 129, 1,
                  30, ctypes.c_void_p(n_d.data_ptr()), ga.engine._stream())


def test_jacobi_svd_wrapper():
    G = np.stack([er.matrix('general', 5, 4400 + b, rows=20) for b in range(3)])
    G[1, :, 3] = 0.0
    U, s, Vt, sweeps = ga.engine.jacobi_svd(ga.engine.to_device(G))
    U, s, Vt = (ga.engine.to_host(x) for x in (U, s, Vt))
    assert U.shape == (3, 20, 5) and s.shape == (3, 5) and Vt.shape == (3, 5, 5) and tuple(sweeps.shape) == (3,)
    for b in range(3):
        ref = np.linalg.svd(G[b], compute_uv=False)
        bound = er.bound(int(sweeps[b]), 5)
        assert (np.diff(s[b]) <= 0).all() and np.abs(s[b] - ref).max() <= bound * ref[0]
        assert er.fro((U[b] * s[b]) @ Vt[b] - G[b]) <= 2 * bound * er.fro(G[b])
    assert s[1, 4] == 0.0 and (U[1, :, 4] == 0.0).all()
    one = ga.engine.jacobi_svd(ga.engine.to_device(G[0]))
    assert isinstance(one[3], int) and np.array_equal(ga.engine.to_host(one[1]), s[0]) and tuple(one[0].shape) == (20, 5)
    with pytest.raises(np.linalg.LinAlgError, match='did not converge'):
        ga.engine.jacobi_svd(ga.engine.to_device(G[0]), max_sweeps=1)
    with pytest.raises(ValueError):
        ga.engine.jacobi_svd(ga.engine.to_device(G[0].T.copy()))


# ---- 2: engine.syev ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 64, 65, 128])
@pytest.mark.parametrize('kind', er.KINDS)
def test_syev(kind, n):
    A = er.matrix(kind, n, 4500 + n)
    S = er.mirror_upper(A)                                   # what syev decomposes: the upper triangle (the general kind is not symmetric)
    shift = er.gershgorin_shift(S)
    w_d, v_d, sweeps = ga.engine.syev(ga.engine.to_device(A))
    w, v = ga.engine.to_host(w_d), ga.engine.to_host(v_d)
    assert 1 <= sweeps <= 30 and (np.diff(w) >= 0).all()
    bound = er.bound(sweeps, n)
    figures = er.eigen_figures(S, w, v, shift)
    print('\nsyev {0} n={1}: sweeps {2}, shift {3:.3g}, dw {4:.2e}, residual {5:.2e}, |VtV-I| {6:.2e}, bound {7:.2e}'.format(kind, n, sweeps, shift, *figures, bound))
    assert figures[0] <= bound and figures[1] <= bound and figures[2] <= bound, (figures, bound)
    dirty = np.where(np.tri(n, k=-1, dtype=bool), np.nan, A)
    w2, v2, sweeps2 = ga.engine.syev(ga.engine.to_device(dirty))
    assert sweeps2 == sweeps and _torch().equal(w2, w_d) and _torch().equal(v2, v_d), 'the strict lower triangle was read'


def test_syev_batch():
    A = np.stack([er.matrix('pairs', 9, 4600 + b) for b in range(4)])
    w, v, sweeps = ga.engine.syev(ga.engine.to_device(A))
    w, v = ga.engine.to_host(w), ga.engine.to_host(v)
    for b in range(4):
        assert max(er.eigen_figures(A[b], w[b], v[b], er.gershgorin_shift(A[b]))) <= er.bound(int(sweeps[b]), 9)


# ---- 3: engine.orthonormalise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,k,cond', [(300, 12, 1e2), (257, 128, 1e6), (1000, 33, 1e12)])
def test_orthonormalise(m, k, cond):
    rng = np.random.default_rng(4700 + k)
    B = (er.orthogonal(m, rng, k) * np.logspace(0, -np.log10(cond), k)) @ er.orthogonal(k, rng)
    Q = ga.engine.to_host(ga.engine.orthonormalise(ga.engine.to_device(B)))
    defect = er.fro(Q.T @ Q - np.eye(k))
    span = er.fro(B - Q @ (Q.T @ B)) / er.fro(B)
    print('\northonormalise {0}x{1} cond {2:g}: |QtQ-I| {3:.2e}, |B - Q Qt B|/|B| {4:.2e}'.format(m, k, cond, defect, span))
    # CholeskyQR3: O(u) orthogonality whatever the condition (Fukaya et al. 2020, Theorem 3.3: 6 (m k + k (k + 1)) u) and a backward stable span
    assert defect <= 6 * (m * k + k * (k + 1)) * er.U and span <= 16 * (m * k + k * (k + 1)) * er.U


def test_orthonormalise_rank_deficient():
    rng = np.random.default_rng(4800)
    B = rng.standard_normal((300, 5)) @ rng.standard_normal((5, 12))
    with pytest.raises(np.linalg.LinAlgError, match='rank deficient'):
        ga.engine.orthonormalise(ga.engine.to_device(B))


# ---- 4: lstsq.teigh -----------------------------------------------------------------------------------------------------------------------
def test_teigh_direct():
    A = er.matrix('symmetric', 128, 4900)
    w, v = ga.lstsq.teigh(A, 5)
    assert isinstance(w, np.ndarray) and w.shape == (5,) and v.shape == (128, 5)
    ref = np.linalg.eigvalsh(A)
    shift = er.gershgorin_shift(A)
    bound = er.bound(30, 128)                                  # teigh does not report the sweeps: the bound of the most it may use
    print('\nteigh direct: dw {0:.2e}, bound {1:.2e}'.format(np.abs(w - ref[::-1][:5]).max() / (np.abs(ref).max() + shift), bound))
    assert np.abs(w - ref[::-1][:5]).max() <= bound * (np.abs(ref).max() + shift)
    assert er.fro(A @ v - v * w) <= bound * (er.fro(A) + shift * np.sqrt(128.0))
    assert er.fro(v.T @ v - np.eye(5)) <= bound


@functools.lru_cache(maxsize=None)
def _decaying(n, decay):
    M = er.symmetric_spectrum_matrix(n, decay, 3500 + n)
    return M, np.linalg.eigvalsh(M)[::-1]


@pytest.mark.parametrize('n,k,decay', [(129, 5, 0.9), (300, 10, 0.9), (257, 40, 0.95)])
def test_teigh_subspace(n, k, decay):
    M, ref = _decaying(n, decay)
    tolerance = 1e-12
    dirty = ga.engine.to_device(np.where(np.tri(n, k=-1, dtype=bool), np.nan, M))
    w_d, v_d = ga.lstsq.teigh(dirty, k, tolerance=tolerance)          # converges within the default max_iter, or raises
    assert _torch().is_tensor(w_d) and tuple(w_d.shape) == (k,) and tuple(v_d.shape) == (n, k)
    w, v = ga.engine.to_host(w_d), ga.engine.to_host(v_d)
    norm = er.fro(M)
    residual = float(np.sqrt(((np.asarray(M, dtype=np.longdouble) @ v - v * w) ** 2).sum(axis=0)).max())
    print('\nteigh n={0} k={1}: dw/u {2:.1f}, residual/|M| {3:.2e}, |vtv-I| {4:.2e}'.format(n, k, np.abs(w - ref[:k]).max() / er.U, residual / norm,
                                                                                         er.fro(v.T @ v - np.eye(k))))
    assert (np.diff(w) <= 0).all()
    assert np.abs(w - ref[:k]).max() <= 2 * tolerance * norm
    assert residual <= tolerance * norm
    assert er.fro(v.T @ v - np.eye(k)) <= 1e-12
    again = ga.lstsq.teigh(dirty, k, tolerance=tolerance)
    assert _torch().equal(again[0], w_d) and _torch().equal(again[1], v_d), 'calls with the default seed differ'


def test_teigh_max_iter():
    M, _ = _decaying(257, 0.95)
    with pytest.raises(np.linalg.LinAlgError, match='after 1 iterations'):
        ga.lstsq.teigh(M, 40, max_iter=1)


# ---- 5: lstsq.trsvd -----------------------------------------------------------------------------------------------------------------------
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g34_trsvd_reference.json')) as _f:
    TRSVD = json.load(_f)


@pytest.mark.parametrize('m,n', [(300, 200), (200, 300)])
def test_trsvd(m, n):
    k = TRSVD['k']
    assert k == 12
    A = er.spectrum_matrix(m, n, TRSVD['decay'], TRSVD['matrix_seed'] + m)
    recorded = TRSVD['cases']['{0}x{1}'.format(m, n)]
    assert len(recorded['values']) == 20 and recorded['worst_values'] == max(recorded['values']) and recorded['worst_residual'] == max(recorded['residual'])
    U, s, Vt = ga.lstsq.trsvd(A, k)
    assert isinstance(U, np.ndarray) and U.shape == (m, k) and s.shape == (k,) and Vt.shape == (k, n)
    sigma = np.linalg.svd(A, compute_uv=False)
    values = np.abs(s - sigma[:k]).max() / sigma[0]
    residual = np.linalg.norm(A - (U * s) @ Vt, 2) / sigma[k]
    print('\ntrsvd {0}x{1}: values {2:.2e} (reference worst {3:.2e}), residual {4:.4f} (reference worst {5:.4f})'.format(
        m, n, values, recorded['worst_values'], residual, recorded['worst_residual']))
    assert (np.diff(s) <= 0).all()
    assert values <= 4 * recorded['worst_values'] and residual <= 4 * recorded['worst_residual']
    assert er.fro(U.T @ U - np.eye(k)) <= 1e-12 and er.fro(Vt @ Vt.T - np.eye(k)) <= 1e-12
    Ut, st, Vtt = ga.lstsq.trsvd(ga.engine.to_device(A), k, generator=7)
    assert _torch().is_tensor(Ut) and _torch().is_tensor(st) and _torch().is_tensor(Vtt)
    assert np.abs(ga.engine.to_host(st) - sigma[:k]).max() / sigma[0] <= 4 * recorded['worst_values']


def test_trsvd_rank_deficient():
    rng = np.random.default_rng(5000)
    A = rng.standard_normal((300, 5)) @ rng.standard_normal((5, 200))
    with pytest.raises(np.linalg.LinAlgError, match='rank deficient'):
        ga.lstsq.trsvd(A, 12)


# ---- 6: lstsq.UnscentedTransformSymmetric -------------------------------------------------------------------------------------------------
def test_unscented_transform():
    rng = np.random.default_rng(5100)
    n, dim, w0 = 40, 7, 0.3
    B = rng.standard_normal((n, n))
    C = B @ B.T + n * np.eye(n)
    x0 = rng.standard_normal(n)
    w, v = ga.lstsq.teigh(C, dim)
    ut = ga.lstsq.UnscentedTransformSymmetric(dim, w0)
    weights = np.full(2 * dim + 1, 0.5 * (1 - w0) / dim)
    weights[0] = w0
    assert np.abs(ut.weights()[0] - weights).max() <= 1e-13 * weights.max() and ut.weights()[1] is ut.weights()[0]
    # the reference's formulas (grates/lstsq.py:1206-1250), with the minus sign of the paper in the second half (see the class docstring)
    scale = np.sqrt(dim / (1 - w0))
    S_ref = np.empty((n, 2 * dim + 1))
    S_ref[:, 0] = x0
    for i in range(dim):
        S_ref[:, i + 1] = x0 + scale * np.sqrt(w[i]) * v[:, i]
        S_ref[:, dim + i + 1] = x0 - scale * np.sqrt(w[i]) * v[:, i]
    S = ut.sigma_points(x0, w, v)
    assert isinstance(S, np.ndarray) and S.shape == (n, 2 * dim + 1)
    assert np.abs(S - S_ref).max() <= 1e-13 * np.abs(S_ref).max()
    mean = ut.average(S)
    assert np.abs(mean - S_ref @ weights).max() <= 1e-13 * np.abs(x0).max()
    assert np.linalg.norm(mean - x0) <= 1e-14 * np.linalg.norm(x0)
    cov = ut.sigma_point_covariance(S)
    cov_ref = (S_ref * weights[np.newaxis, :]) @ S_ref.T
    assert np.abs(cov - cov_ref).max() <= 1e-13 * np.abs(cov_ref).max()
    centred = ut.sigma_point_covariance(S - x0[:, np.newaxis])
    assert np.abs(centred - (v * w) @ v.T).max() <= 1e-12 * np.linalg.norm(C, 2)
    # a tensor in gives a tensor out
    St = ut.sigma_points(ga.engine.to_device(x0), ga.engine.to_device(w), ga.engine.to_device(v))
    assert _torch().is_tensor(St) and np.array_equal(ga.engine.to_host(St), S)
    assert _torch().is_tensor(ut.average(St)) and _torch().is_tensor(ut.sigma_point_covariance(St))
    wt, vt = ga.lstsq.teigh(ga.engine.to_device(C), dim)
    assert _torch().is_tensor(wt) and np.array_equal(ga.engine.to_host(wt), w) and np.array_equal(ga.engine.to_host(vt), v)
