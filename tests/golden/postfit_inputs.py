"""Host references of the tests of the post-fit pass (lstsq.PostFit, shg_segment_lag_products): lagged products in exact integer
arithmetic, the divisors of the covariance function, the pass itself on explicit matrices, and the redundancy of an arc from the hat
matrix of the explicit system.  Rows are component-major, k M + t, as the columns of the transposed design matrices.  Needs NumPy
only."""

from fractions import Fraction

import numpy as np

from arc_inputs import DROP, bounds_of, reduction

U = 2.0 ** -53


def _integers(x):
    """the doubles x as exact integers: x[i] = integers[i] / 2^shift"""
    fractions = [Fraction(float(v)) for v in x]
    shift = max([f.denominator.bit_length() - 1 for f in fractions] + [0])
    return [f.numerator * ((1 << shift) // f.denominator) for f in fractions], shift


def exact_lag_products(X, seg, lags):
    """S [rows, nseg, lags + 1] of shg_segment_lag_products in exact arithmetic, rounded once, with the magnitudes sum |x_t x_(t+k)| and
    the numbers of pairs [nseg, lags + 1]; seg as given (0 <= seg[s] <= seg[s+1] <= M, or empty segments)"""
    rows, nseg = X.shape[0], len(seg) - 1
    S, magnitude, pairs = np.zeros((rows, nseg, lags + 1)), np.zeros((rows, nseg, lags + 1)), np.zeros((nseg, lags + 1), dtype=np.int64)
    for s in range(nseg):
        first, last = int(seg[s]), max(int(seg[s + 1]), int(seg[s]))
        pairs[s] = np.maximum(last - first - np.arange(lags + 1), 0)
        for r in range(rows):
            x, shift = _integers(X[r, first:last])
            scale = 1 << (2 * shift)
            for k in range(min(lags + 1, last - first)):
                terms = [a * b for a, b in zip(x, x[k:])]
                S[r, s, k], magnitude[r, s, k] = float(Fraction(sum(terms), scale)), float(Fraction(sum(abs(term) for term in terms), scale))
    return S, magnitude, pairs


def plain_lag_products(X, seg, lags):
    """the same sums by a plain double loop in fractions.Fraction (for small cases: the check of exact_lag_products)"""
    rows, nseg = X.shape[0], len(seg) - 1
    S = np.zeros((rows, nseg, lags + 1))
    for r in range(rows):
        for s in range(nseg):
            for k in range(lags + 1):
                total = Fraction(0)
                for t in range(int(seg[s]), int(seg[s + 1]) - k):
                    total += Fraction(float(X[r, t])) * Fraction(float(X[r, t + k]))
                S[r, s, k] = float(total)
    return S


def divisors(arcs, count, maximum_lag, biased):
    """d_k of PostFit.covariance_function for k = 0 .. maximum_lag: sum_a max(len_a - k, 0), or d_0 for all k (biased)"""
    lengths = np.diff(bounds_of(arcs, count))
    d = np.array([np.maximum(lengths - k, 0).sum() for k in range(maximum_lag + 1)], dtype=np.int64)
    return np.full(maximum_lag + 1, d[0]) if biased else d


def covariance_function(residuals, arcs, maximum_lag, biased):
    """(c [K, q + 1], bound [K, q + 1], pooled c [q + 1], pooled bound [q + 1]) of the estimator on residuals [M, K]: exact sums,
    rounded once, and the bounds (n + 1) u sum |e_t e_(t+k)| / d_k of sums of n pairs formed in floating point"""
    M, K = residuals.shape
    bounds = bounds_of(arcs, M)
    S, magnitude, pairs = exact_lag_products(np.ascontiguousarray(residuals.T), bounds, maximum_lag)
    d = divisors(arcs, M, maximum_lag, biased).astype(np.float64)
    n = pairs.sum(axis=0)
    c, bound = S.sum(axis=1) / d, (n + 1) * U * magnitude.sum(axis=1) / d
    return c, bound, S.sum(axis=(0, 1)) / (K * d), (K * n + 1) * U * magnitude.sum(axis=(0, 1)) / (K * d)


def arc_rows(bounds, K, M):
    """the rows k M + t of every arc in the component-major order, a list of index arrays"""
    return [np.concatenate([k * M + np.arange(first, last) for k in range(K)]) for first, last in zip(bounds[:-1], bounds[1:])]


def projectors(units):
    """(rows, Q) of every unit of arc_inputs.explicit_columns: the rows it touches and an orthonormal basis of its range (SVD; squared
    singular values at or below DROP times the largest are dropped, the rank rule of the elimination); also the ranks"""
    out, ranks = [], []
    for E in units:
        rows = np.flatnonzero(np.any(E != 0.0, axis=1))
        if rows.size == 0:
            out.append((rows, np.zeros((0, 0))))
            ranks.append(0)
            continue
        Q, s, _ = np.linalg.svd(E[rows], full_matrices=False)
        Q = Q[:, s * s > DROP * s[0] * s[0]]
        out.append((rows, Q))
        ranks.append(Q.shape[1])
    return out, np.array(ranks)


def project(values, units):
    """(I - Q Q^T) values for the units (they do not overlap); values [K M] or [K M, n]"""
    values = values.copy()
    for rows, Q in projectors(units)[0]:
        if rows.size:
            values[rows] -= Q @ (Q.T @ values[rows])
    return values


def parameters(values, units):
    """y [units, u] = R R^T E^T values of every unit, with R of arc_inputs.reduction: zero along the dropped directions"""
    out = []
    for E in units:
        R = reduction(E.T @ E)[0]
        out.append(R @ (R.T @ (E.T @ values)))
    return np.array(out)


def hat_diagonal(F):
    """diagonal of the hat matrix F F^+ of the explicit system F, from the SVD (relative rank tolerance 1e-10)"""
    Q, s, _ = np.linalg.svd(F, full_matrices=False)
    Q = Q[:, s > 1e-10 * s[0]]
    return np.einsum('ij,ij->i', Q, Q)


def hat_diagonal_lstsq(F):
    """the same from numpy.linalg.lstsq: H = F X with X the minimum-norm solution of F X = I"""
    return np.einsum('ij,ji->i', F, np.linalg.lstsq(F, np.eye(F.shape[0]), rcond=1e-10)[0])


def hat_redundancies(diagonal, bounds, K, M):
    """r_a = K len_a - sum over the rows i of arc a of H_ii"""
    return np.array([rows.size - diagonal[rows].sum() for rows in arc_rows(bounds, K, M)])


def pass_redundancies(A, units, unit_ranks, bounds, K, M):
    """r_a the way the pass forms it with the exact trace: n_a - trace((I - Q_a Q_a^T) A_a N^-1 A_a^T (I - Q_a Q_a^T)), N the normals of
    the projected design matrix, n_a = K len_a - the ranks of the units of the arc (unit_ranks [arcs, units per arc])"""
    Ap = project(A, units)
    Ninv = np.linalg.inv(Ap.T @ Ap)
    return np.array([rows.size - ranks.sum() - np.einsum('ij,jk,ik->', Ap[rows], Ninv, Ap[rows])
                     for rows, ranks in zip(arc_rows(bounds, K, M), unit_ranks)])
