"""
Plain references, error figures and seeded inputs for the dense Cholesky factorisation, the triangular inverse and the solve behind
BlockMatrix.cholesky() / solve_triangular() / sparse_inverse() (tests/test_gpu_factorisation_seams.py,
tests/test_factorisation_reference_cpu.py).  NumPy only, written from the definitions in np.longdouble; nothing of the library is used.

Conventions: A = U^T U with U upper triangular, X = U^-1, Z = A^-1 = X X^T; only the upper triangle of A is ever read.

Figures (all evaluated in long double; u = 2^-53):
  scaled_residual   max_{i <= j} |U^T U - A|_ij / sqrt(a_ii a_jj).  Cholesky is backward stable row- and column-scaled: |U^T U - A|_ij <=
                    gamma(n + 1) sqrt(a_ii a_jj) / (1 - gamma(n + 1)) whatever the condition number (Higham, Accuracy and Stability of
                    Numerical Algorithms, Theorem 10.5 and (10.7)), and the figure does not change under A -> D A D.
  inverse_error     max_{i <= j} |X - X_ref|_ij / (|X_ref| |U_ref| |X_ref|)_ij, where U_ref is the triangular matrix that was inverted (the
                    factor as the routine under test computed it) and X_ref its inverse in long double: the componentwise forward bound
                    c_n u |X| |U| |X| holds for every stable triangular inversion, block methods included (Higham, chapter 14), whatever
                    the condition number, and is invariant under U -> U D as well.  (Against the inverse of the EXACT factor the figure
                    would be the forward error of the factor, kappa u, with the inversion's own error buried under it.)
  forward_error     max |x - x_ref| / max |x_ref|.
"""

import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# ---- the cases shared by the CPU and the GPU tests ------------------------------------------------------------------------------
# every leaf size next to a border of the leaf's 32-row groups and of its padding to 128, and the multi-panel sizes whose last panel
# is one row, one group, ... wide (513: recursion 256 | 128 | 128 | 1, five look-ahead panels)
SIZES = (1, 2, 3, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257, 300, 384, 385, 513)
PIVOT_N = 300
PIVOTS = (1, 2, 3, 32, 33, 64, 65, 127, 128, 129, 130, 256, 257, 258, 300)
RANK1_N = 40
NAN_SITES = ((0, 0), (5, 5), (3, 140), (130, 131), (200, 299))              # (i, j), i <= j, of an otherwise good 300 x 300 matrix
WALKER_N, WALKER_CUT = 430, (0, 300, 430)
WALKER_PIVOTS = (17, 300, 301, 430)
WALKER_SCHUR_PIVOTS = (1, 2, 64, 129, 130)                                  # local index within the 130 rows of the second block row
# (n, kappa, seed, block bounds)
CONDITIONING = tuple((n, kappa, 7 * n + k, (0, n)) for n in (96, 300) for k, kappa in enumerate((1e4, 1e8, 1e11))) + ((430, 1e8, 430, WALKER_CUT),)
GRADED_N = (96, 300)


def as_ld(a):
    return np.asarray(a, dtype=LD)


# ---- the operations ---------------------------------------------------------------------------------------------------------------
def cholesky_upper(A):
    """Right-looking Cholesky factorisation A = U^T U of the upper triangle of A in long double.  Returns (U, p): p = 0, or the
    1-based index of the first pivot that is not > 0 (a NaN pivot included); the rows from p on are then left as they were at that step."""
    W = np.triu(as_ld(A))                                                   # a copy; the strictly lower triangle is never looked at
    n = W.shape[0]
    for k in range(n):
        d = W[k, k]
        if not d > 0:
            return W, k + 1
        s = np.sqrt(d)
        W[k, k] = s
        W[k, k + 1:] /= s
        r = W[k, k + 1:]
        W[k + 1:, k + 1:] -= np.triu(r[:, None] * r[None, :])
    return W, 0


def triangular_inverse(Uf):
    """X = U^-1 of an upper triangular U by back substitution, row by row from the last one: X[i, :] = (e_i - U[i, i+1:] X[i+1:, :]) / u_ii"""
    Uf = as_ld(Uf)
    n = Uf.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n - 1, -1, -1):
        row = -(Uf[i, i + 1:] @ X[i + 1:, i:]) if i + 1 < n else np.zeros(n - i, dtype=LD)
        row[0] += 1
        X[i, i:] = row / Uf[i, i]
    return X


def solve(Uf, b):
    """x of U^T U x = b: forward substitution with U^T, backward substitution with U; b [n] or [n, k]"""
    Uf = as_ld(Uf)
    y = np.array(as_ld(b), copy=True)
    n = Uf.shape[0]
    for i in range(n):
        y[i] = (y[i] - Uf[:i, i] @ y[:i]) / Uf[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - Uf[i, i + 1:] @ y[i + 1:]) / Uf[i, i]
    return y


def inverse_from_factor(Uf):
    """(U^T U)^-1 = X X^T"""
    X = triangular_inverse(Uf)
    return X @ X.T


# ---- the figures -----------------------------------------------------------------------------------------------------------------
def scaled_residual(Uf, A):
    Uf, A = np.triu(as_ld(Uf)), as_ld(A)
    d = np.sqrt(np.diag(A))
    R = np.abs(Uf.T @ Uf - A) / (d[:, None] * d[None, :])
    return float(np.max(np.triu(R)))


def inverse_error(X, U_ref, X_ref):
    X, U_ref, X_ref = np.triu(as_ld(X)), np.triu(as_ld(U_ref)), np.triu(as_ld(X_ref))
    bound = np.abs(X_ref) @ np.abs(U_ref) @ np.abs(X_ref)
    iu = np.triu_indices(X.shape[0])
    return float(np.max(np.abs(X - X_ref)[iu] / bound[iu]))


def forward_error(x, x_ref):
    x, x_ref = as_ld(x), as_ld(x_ref)
    return float(np.max(np.abs(x - x_ref)) / np.max(np.abs(x_ref)))


def max_norm_error(Z, Z_ref):
    """max |Z - Z_ref| / max |Z_ref| over the upper triangle (the inverse of section 'conditioning')"""
    Z, Z_ref = np.triu(as_ld(Z)), np.triu(as_ld(Z_ref))
    return float(np.max(np.abs(Z - Z_ref)) / np.max(np.abs(Z_ref)))


# ---- the inputs (float64, seeded) ---------------------------------------------------------------------------------------------------
def spd_spectrum(n, kappa, seed):
    """Q diag(lambda) Q^T with lambda = logspace(0, -log10 kappa) and a random orthogonal Q, symmetrised: condition number kappa"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, -np.log10(kappa), n)
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


def graded(A, seed, emax=40):
    """(D A D, e) with D = diag(2^e_i), integer e_i in [-emax, emax]: every entry is scaled by a power of two, exactly"""
    rng = np.random.default_rng(seed)
    e = rng.integers(-emax, emax + 1, size=A.shape[0])
    return np.ldexp(A, e[:, None] + e[None, :]), e


def first_bad_minor(n, p, seed):
    """A = U0^T D U0 with U0 = 2 I + (strictly upper random part) / n and D = I except D_pp = -1 (p counts from 1; p = 0: D = I, positive
    definite).  In exact arithmetic the pivots are +4 and -4: the leading minor of order p is the first that fails, far from any
    rounding decision, and whatever an elimination does after the failure cannot move the index."""
    rng = np.random.default_rng(seed)
    U0 = 2.0 * np.eye(n) + np.triu(rng.standard_normal((n, n)), 1) / n
    D = np.ones(n)
    if p:
        D[p - 1] = -1.0
    A = U0.T @ (D[:, None] * U0)
    return 0.5 * (A + A.T)


def semidefinite_rank1(n):
    """v v^T with v = 1, 2, 3, 4, 1, 2, ...: the second pivot a_22 - a_12^2 / a_11 = 4 - 2 * 2 is exactly zero.  v_1 = 1 makes the first
    elimination step exact whether it divides by the pivot or multiplies with its reciprocal, so the zero is no rounding decision either."""
    v = 1.0 + (np.arange(n) % 4)
    return np.outer(v, v)


def with_nan(A, i, j):
    """A with one NaN at (i, j) of the upper triangle (and, symmetric, at (j, i))"""
    B = A.copy()
    B[i, j] = B[j, i] = np.nan
    return B


@functools.lru_cache(maxsize=None)
def reference(n, kappa, seed):
    """(A, U_ref, X_ref) of spd_spectrum(n, kappa, seed): computed once, shared by the tests, never written to"""
    A = spd_spectrum(n, kappa, seed)
    Uf, p = cholesky_upper(A)
    assert p == 0
    X = triangular_inverse(Uf)
    for a in (A, Uf, X):
        a.setflags(write=False)
    return A, Uf, X
