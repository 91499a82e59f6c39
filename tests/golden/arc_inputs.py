"""Inputs and host references of the tests of arc-wise parameters (lstsq.ArcParameters, shg_segment_products): the explicit columns of
the parameters of every arc, and three NumPy formulations of their elimination from a least-squares problem that the tests hold against
each other and against the device: the Schur complement of the normals, the projection of the design matrix, and numpy.linalg.lstsq of
the system with the explicit columns.  Rows are component-major, k M + t, as the columns of the transposed design matrices.  Needs
NumPy only."""

from fractions import Fraction

import numpy as np

U = 2.0 ** -53
DROP = 1e-12                                          # eigenvalues of G at or below DROP times the largest are dropped


def bounds_of(arcs, count):
    return np.append(np.asarray(arcs, dtype=np.int64), count)


def transformed_basis(basis, root, K, filters=None):
    """B [K, M, u] the way of the design matrix: basis [M, u'] (shared) or [M, K, u] (general), times root [M, K] (sqrt of the weights,
    None: 1), then the dense W [M, M] of every channel (filters, a list of K matrices, None: white noise)"""
    basis = np.asarray(basis, dtype=np.float64)
    B = np.repeat(basis[None], K, axis=0) if basis.ndim == 2 else np.ascontiguousarray(basis.transpose(1, 0, 2))
    if root is not None:
        B = B * np.broadcast_to(root, (B.shape[1], K)).T[:, :, None]
    if filters is not None:
        B = np.stack([filters[k] @ B[k] for k in range(K)])
    return B


def explicit_columns(B, bounds, shared):
    """the columns of the parameters as a list of units [K M, u], zero outside the unit: (arc, channel) pairs, arc-major, for a
    shared basis; arcs for the general form"""
    K, M, u = B.shape
    units = []
    for first, last in zip(bounds[:-1], bounds[1:]):
        if shared:
            for k in range(K):
                E = np.zeros((K, M, u))
                E[k, first:last] = B[k, first:last]
                units.append(E.reshape(K * M, u))
        else:
            E = np.zeros((K, M, u))
            E[:, first:last] = B[:, first:last]
            units.append(E.reshape(K * M, u))
    return units


def reduction(G, b=None):
    """R = V_keep Lambda_keep^-1/2 of one G (rank 0 when the largest eigenvalue is not positive) and its rank"""
    values, vectors = np.linalg.eigh(G)
    if not values[-1] > 0.0:
        return np.zeros((G.shape[0], 0)), 0
    kept = values > DROP * values[-1]
    return vectors[:, kept] / np.sqrt(values[kept]), int(np.count_nonzero(kept))


def schur(A, l, units):
    """(N, n, lPl, observation count, ranks, parameters(x)) of the Schur formulation: A [L, P], l [L]"""
    N, n, lPl = A.T @ A, A.T @ l, float(l @ l)
    ranks, kept = [], []
    for E in units:
        R, rank = reduction(E.T @ E)
        D, g = (A.T @ E) @ R, R.T @ (E.T @ l)
        N, n, lPl = N - D @ D.T, n - D @ g, lPl - float(g @ g)
        ranks.append(rank)
        kept.append((R, D, g))
    return N, n, lPl, A.shape[0] - sum(ranks), np.array(ranks), lambda x: np.array([R @ (g - D.T @ x) for R, D, g in kept])


def projection(A, l, units):
    """(N, n, lPl) of (I - Q Q^T) A and (I - Q Q^T) l, Q an orthonormal basis of the range of every unit (the units do not overlap);
    the same rank rule on the squared singular values"""
    A, l = A.copy(), l.copy()
    for E in units:
        rows = np.flatnonzero(np.any(E != 0.0, axis=1))
        if rows.size == 0:
            continue
        Q, s, _ = np.linalg.svd(E[rows], full_matrices=False)
        Q = Q[:, s * s > DROP * s[0] * s[0]]
        A[rows] -= Q @ (Q.T @ A[rows])
        l[rows] -= Q @ (Q.T @ l[rows])
    return A.T @ A, A.T @ l, float(l @ l)


def explicit_solution(A, l, units):
    """(x [P], y [units, u]) of numpy.linalg.lstsq of [A | E]: the minimum-norm solution, zero along the dropped directions (y is a
    list where the units differ in their number of parameters)"""
    solution = np.linalg.lstsq(np.hstack([A] + units), l, rcond=None)[0]
    P, widths = A.shape[1], [E.shape[1] for E in units]
    parts = np.split(solution[P:], np.cumsum(widths)[:-1])
    return solution[:P], np.array(parts) if len(set(widths)) == 1 else parts


def normals_bounds(A, l, factor=1.0):
    """entry-wise bounds factor * 2 L u sqrt(N_ii N_jj), ... sqrt(N_ii l^T l), ... l^T l of dot products of length L = rows of A, with
    the diagonals of the unreduced A^T A"""
    L = A.shape[0]
    d, lPl = np.sqrt(np.einsum('ij,ij->j', A, A)), float(l @ l)
    return factor * 2 * L * U * np.outer(d, d), factor * 2 * L * U * d * np.sqrt(lPl), factor * 2 * L * U * lPl


def conditions(units):
    """cond(G) of the units over the eigenvalues that are kept (1 for a unit of rank 0)"""
    out = []
    for E in units:
        values = np.linalg.eigvalsh(E.T @ E)
        kept = values[values > DROP * values[-1]] if values[-1] > 0.0 else np.ones(1)
        out.append(kept[-1] / kept[0])
    return np.array(out)


def solution_bound(A, N, units):
    """Relative bound of the deviation of the solution of the reduced normals N from that of the explicit system.  The normals carry
    a relative perturbation of 2 L u from their dot products of length L, and the subtracted C G^+ C^T, which is at most the arc's own
    share of A^T A, one of u' u cond(G) from the eigenpairs of G (an eigenvalue is known to u lambda_max, so its reciprocal to
    u cond(G), for each of the u' directions); the solve amplifies both by cond(N) at most."""
    return (2 * A.shape[0] + units[0].shape[1] * conditions(units).max()) * U * np.linalg.cond(N)


def host_case(arcs, seed=2801):
    """the seeded host case of the three formulations: M = 700, K = 3, P = 169, a random design matrix, weights with zeros and the
    shared basis of Legendre degrees 0 and 1 plus one period of 93 samples (u' = 4): (A [K M, P], l [K M], units, root [M, K], basis)"""
    from grates_amd import lstsq
    M, K, P = 700, 3, 169
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 4.0, (M, K))
    w[4 + rng.choice(M - 4, 30, replace=False), rng.integers(0, K, 30)] = 0.0           # not in the two short arcs of [0, 1, 4, 300]: their ranks stay 1 and 3
    root = np.sqrt(w)
    A = rng.standard_normal((K, M, P)) * root.T[:, :, None]
    l = rng.standard_normal((K, M)) * root.T
    basis = lstsq.arc_basis(arcs, M, degree=1, periods=(93,))
    units = explicit_columns(transformed_basis(basis, root, K), bounds_of(arcs, M), True)
    return A.reshape(K * M, P), l.reshape(K * M), units, root, basis


def exact_segment_products(X, Bt, seg, channels):
    """S [rows, nseg, u] of shg_segment_products in exact rational arithmetic, rounded once, with the magnitudes sum |x_t b_t| and the
    lengths of the segments; seg as given (0 <= seg[s] <= seg[s+1] <= M, or empty segments)"""
    rows, u, nseg = X.shape[0], Bt.shape[0], len(seg) - 1
    S, magnitude = np.zeros((rows, nseg, u)), np.zeros((rows, nseg, u))
    for r in range(rows):
        for s in range(nseg):
            columns = range(int(seg[s]), max(int(seg[s + 1]), int(seg[s])))
            x = [Fraction(float(X[r, t])) for t in columns]
            for j in range(u):
                terms = [xt * Fraction(float(Bt[j, r % channels, t])) for xt, t in zip(x, columns)]
                S[r, s, j], magnitude[r, s, j] = float(sum(terms, Fraction(0))), float(sum((abs(term) for term in terms), Fraction(0)))
    lengths = np.maximum(np.diff(np.asarray(seg, dtype=np.int64)), 0)
    return S, magnitude, lengths


def clamped(seg, M):
    """the table shg_segment_products uses in place of seg: clamped to 0 .. M, then the running maximum"""
    return np.maximum.accumulate(np.clip(np.asarray(seg, dtype=np.int64), 0, M))
