"""
Helpers of tests/test_eigen_cpu.py and tests/test_gpu_eigen.py: a NumPy model of shg_jacobi_svd (csrc/jacobi.hip) and of engine.syev
with the kernel's tournament order, threshold, rotation formula and shift; the test matrices; the error figures in numpy.longdouble.
"""
import numpy as np

U = 2.0 ** -53                                    # unit roundoff of fp64
KINDS = ('symmetric', 'deficient', 'pairs', 'general')


def stage_pairs(c, s):
    """the pairs (p, q), p < q, of stage s (0 .. m - 2) of the round-robin tournament over m = c rounded up to even players; the
    partner of the player that does not exist (odd c) idles"""
    m = (c + 1) & ~1
    out = []
    for k in range(m // 2):
        p, q = (m - 1, s) if k == 0 else ((s + k) % (m - 1), (s - k + m - 1) % (m - 1))
        p, q = min(p, q), max(p, q)
        if q < c:
            out.append((p, q))
    return out


def jacobi_model(G, max_sweeps=30):
    """(G V, V, sigma, sweeps) as shg_jacobi_svd leaves them (sums in NumPy's order, not the kernel's: equal up to rounding)"""
    G = np.array(G, dtype=np.float64)
    r, c = G.shape
    V = np.eye(c)
    tol = np.sqrt(float(r)) * U
    used = 1 if (c < 2 or not np.isfinite(G).all()) else -1
    if used < 0:
        m = (c + 1) & ~1
        for sweep in range(1, max_sweeps + 1):
            rotated = False
            for s in range(m - 1):
                for p, q in stage_pairs(c, s):
                    x, y = G[:, p].copy(), G[:, q].copy()
                    a, b, d = x @ x, y @ y, x @ y
                    if abs(d) > tol * (np.sqrt(a) * np.sqrt(b)):
                        z = (b - a) / (2.0 * d)
                        t = np.copysign(1.0, z) / (abs(z) + np.sqrt(1.0 + z * z))
                        cs = 1.0 / np.sqrt(1.0 + t * t)
                        sn = cs * t
                        G[:, p], G[:, q] = cs * x - sn * y, sn * x + cs * y
                        x, y = V[:, p].copy(), V[:, q].copy()
                        V[:, p], V[:, q] = cs * x - sn * y, sn * x + cs * y
                        rotated = True
            if not rotated:
                used = sweep
                break
    return G, V, np.sqrt((G * G).sum(axis=0)), used


def mirror_upper(A):
    A = np.triu(np.asarray(A, dtype=np.float64))
    return A + np.triu(A, 1).T


def gershgorin_shift(A):
    """max(0, max_i(sum_{j != i} |a_ij| - a_ii)): A + shift I is positive semi-definite"""
    d = np.diag(A)
    return max(0.0, float((np.abs(A).sum(axis=1) - np.abs(d) - d).max()))


def syev_model(A, max_sweeps=30):
    """(w ascending, v, sweeps, shift) as engine.syev computes them: the upper triangle mirrored, the Gershgorin shift, the model
    kernel, the Rayleigh quotients v_i . g_i - shift"""
    A = mirror_upper(A)
    shift = gershgorin_shift(A)
    G, V, _, sweeps = jacobi_model(A + shift * np.eye(A.shape[0]), max_sweeps)
    w = (V * G).sum(axis=0) - shift
    order = np.argsort(w, kind='stable')
    return w[order], V[:, order], sweeps, shift


def orthogonal(n, rng, k=None):
    return np.linalg.qr(rng.standard_normal((n, n if k is None else k)))[0]


def matrix(kind, n, seed, rows=None):
    """the four kinds of test matrix: random symmetric; positive semi-definite of rank n // 2; eigenvalues 1 .. n // 2 and
    -1 .. -(n // 2) (and 0 for odd n) under a random orthogonal basis; random non-symmetric [rows or n, n]"""
    rng = np.random.default_rng(seed)
    if kind == 'symmetric':
        A = rng.standard_normal((n, n))
        return 0.5 * (A + A.T)
    if kind == 'deficient':
        B = rng.standard_normal((n, n // 2))
        return B @ B.T
    if kind == 'pairs':
        h = n // 2
        lam = np.concatenate([np.arange(1.0, h + 1), -np.arange(1.0, h + 1), np.zeros(n - 2 * h)])
        Q = orthogonal(n, rng)
        A = (Q * lam) @ Q.T
        return 0.5 * (A + A.T)
    if kind == 'general':
        return rng.standard_normal((n if rows is None else rows, n))
    raise ValueError(kind)


def spectrum_matrix(m, n, decay, seed):
    """U0 diag(decay^i) V0^T [m, n] with random orthonormal U0, V0 (symmetrised Q diag Q^T for m == n with one basis)"""
    rng = np.random.default_rng(seed)
    k = min(m, n)
    lam = decay ** np.arange(k)
    return (orthogonal(m, rng, k) * lam) @ orthogonal(n, rng, k).T


def symmetric_spectrum_matrix(n, decay, seed):
    Q = orthogonal(n, np.random.default_rng(seed))
    M = (Q * decay ** np.arange(n)) @ Q.T
    return 0.5 * (M + M.T)


def bound(sweeps, c):
    """16 stages sqrt(c) u with stages = sweeps (c - 1): the first-order bound of `stages` sets of disjoint plane rotations (Higham,
    Accuracy and Stability of Numerical Algorithms, Lemma 19.9, with 8 u per rotation, doubled for the Gram product).  c = 1 has
    no stage: one rounding of the norm."""
    return 16.0 * max(sweeps * (c - 1), 1) * np.sqrt(float(c)) * U


def fro(X):
    X = np.asarray(X, dtype=np.longdouble)
    return float(np.sqrt((X * X).sum()))


def svd_figures(G_in, G_out, V, sigma):
    """(|V^T V - I|_F, |G_in V - G_out|_F / |G_in|_F, max |sorted sigma - LAPACK's| / sigma_max) in numpy.longdouble"""
    Gi, Go, Vl = (np.asarray(x, dtype=np.longdouble) for x in (G_in, G_out, V))
    c = Vl.shape[0]
    s = np.linalg.svd(np.asarray(G_in, dtype=np.float64), compute_uv=False)
    mine = np.sort(np.asarray(sigma, dtype=np.float64))[::-1][:len(s)]
    scale = fro(Gi) or 1.0
    return fro(Vl.T @ Vl - np.eye(c)), fro(Gi @ Vl - Go) / scale, float(np.abs(mine - s).max() / (s[0] or 1.0))


def lapack_svd_figures(G_in):
    """the same figures of numpy.linalg.svd on the same matrix (the third against itself is zero and left out)"""
    G = np.asarray(G_in, dtype=np.float64)
    Us, s, Vt = np.linalg.svd(G, full_matrices=False)
    Vl = np.asarray(Vt.T, dtype=np.longdouble)
    return fro(Vl.T @ Vl - np.eye(Vl.shape[1])), fro(np.asarray(G, dtype=np.longdouble) @ Vl - np.asarray(Us * s, dtype=np.longdouble)) / (fro(G) or 1.0)


def eigen_figures(A, w, v, shift):
    """(max |w - LAPACK's| / (|A|_2 + shift), |A v - v diag(w)|_F / (|A|_F + shift sqrt(n)), |v^T v - I|_F) for the symmetric A"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    ref = np.linalg.eigvalsh(A)
    Al, vl, wl = (np.asarray(x, dtype=np.longdouble) for x in (A, v, w))
    return (float(np.abs(np.asarray(w) - ref).max() / ((np.abs(ref).max() + shift) or 1.0)),
            fro(Al @ vl - vl * wl) / ((fro(Al) + shift * np.sqrt(float(n))) or 1.0),
            fro(vl.T @ vl - np.eye(vl.shape[1])))
