"""
Plain references and derived error bounds for the kernels of csrc/filters.hip (tests/test_gpu_filter_seams.py,
tests/test_filters_reference_cpu.py).  NumPy only; np.longdouble where it says so; nothing of the library is used.

Order-wise filter.  Every output coefficient is one dot product of n = N + 1 - m terms, y = sum_k W[r][k] x[k].  Whatever the order of
summation, an fp64 evaluation with n - 1 additions (fused or not) satisfies |fl(y) - y| <= gamma(n) sum_k |W[r][k]| |x[k]| with
gamma(k) = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  The kernels form two partial
sums (the even and the odd columns of a step of eight) and add them at the end, and they add terms that are exactly zero (the padding
of the K loop), which costs no rounding: gamma(n + 2) covers both with room.  E = gamma(n + 2) (|W| |x|) is therefore a bound that a correct
kernel cannot exceed -- derived, not measured -- and it is far below the size of any single misplaced term.

Cholesky solve.  The computed solution of A x = b satisfies (A + dA) x = b with |dA| <= gamma(3 d + 1) |R^T| |R| (Higham, Theorem 10.4),
and || |R^T| |R| ||_2 <= d ||A||_2, so that ||A X - B||_F / (||A||_F ||X||_F) <= d gamma(3 d + 1) column by column and for any set of columns.
"""

import functools

import numpy as np

import inputs

LD = np.longdouble
U = 2.0 ** -53
POISON = 1e30


def gamma(k):
    """k u / (1 - k u) in long double"""
    return LD(k) * LD(U) / (LD(1) - LD(k) * LD(U))


def slot_order(s):
    """order m of slot s (0: order 0 cosine, 2m - 1: order m cosine, 2m: order m sine -- the order of the DDK block list)"""
    return (s + 1) >> 1


def slot_index(N, s):
    """(rows, columns) of the coefficients of slot s, degrees m .. N, in a reference array [N+1][N+1]: C_nm at [n][m], S_nm at [m-1][n]"""
    m = slot_order(s)
    n = np.arange(m, N + 1)
    if s == 0 or s & 1:
        return n, np.full(n.size, m)
    return np.full(n.size, m - 1), n


def orderwise_reference(blocks, batch):
    """OrderWiseFilter.filter of every epoch of batch [B][N+1][N+1] at once in long double: one W[:n, :n] @ X per slot, degrees 0 and 1
    restored.  Returns (ref, E), both long double and laid out like the output: E = gamma(n + 2) (|W[:n, :n]| @ |X|), zero at degrees 0
    and 1.  (E is evaluated in float64, whose sum of n non-negative terms is low by a factor of 1 - gamma(n) at the most: divided out.)"""
    batch = np.asarray(batch, dtype=np.float64)
    B, N = batch.shape[0], batch.shape[-1] - 1
    assert batch.shape == (B, N + 1, N + 1) and len(blocks) >= 2 * N + 1 and blocks[0].shape[0] >= N + 1
    ref = batch.astype(LD)
    E = np.zeros(batch.shape, dtype=LD)
    for s in range(2 * N + 1):
        n = N + 1 - slot_order(s)
        r, c = slot_index(N, s)
        W = np.ascontiguousarray(blocks[s][:n, :n], dtype=np.float64)
        X = batch[:, r, c].T                                                    # [n][B]
        ref[:, r, c] = (W.astype(LD) @ X.astype(LD)).T
        E[:, r, c] = (gamma(n + 2) / (LD(1) - gamma(n + 2)) * (np.abs(W) @ np.abs(X)).astype(LD)).T
    ref[:, 0:2, 0:2] = batch[:, 0:2, 0:2]
    E[:, 0:2, 0:2] = 0
    return ref, E


def worst_ratio(got, ref, E):
    """max |got - ref| / E over the entries with E > 0; where E == 0 (degrees 0 and 1, or an all-zero product) the values must be equal:
    inf if they are not"""
    diff = np.abs(np.asarray(got).astype(LD) - ref)
    if np.any(diff[E == 0] != 0):
        return float('inf')
    pos = E > 0
    return float(np.max(diff[pos] / E[pos])) if np.any(pos) else 0.0


def order_major_rows(N):
    """int64 [N+1][N+1]: the row of an order-major series of degree N that holds entry [r][c] of a reference array.  From the layout's
    definition (csrc/filters.hip, header of the order-major section): the slots s = 0 .. 2N follow each other, slot s holds the degrees
    m .. N of its order in consecutive rows."""
    rows = np.full((N + 1, N + 1), -1, dtype=np.int64)
    first = 0
    for s in range(2 * N + 1):
        r, c = slot_index(N, s)
        rows[r, c] = first + np.arange(r.size)
        first += r.size
    assert first == (N + 1) ** 2
    return rows


@functools.lru_cache(maxsize=3)
def _random_blocks(seed, Nb):
    return inputs.orderwise_random_blocks(seed, Nb)


def random_blocks(seed, Nb):
    """inputs.orderwise_random_blocks(seed, Nb); the last three sets are kept (d/o 300: 145 MB).  Callers do not write into them."""
    return _random_blocks(int(seed), int(Nb))


def poisoned_blocks(seed, Nb, N):
    """inputs.orderwise_random_blocks(seed, Nb) with every entry outside the leading (N + 1 - m)^2 corner of each block set to 1e30: what a
    filter of degree N < Nb must never let through.  Finite on purpose: the kernels multiply these entries by staged zeros, and 0 * NaN
    would fail a correct kernel."""
    out = []
    for s, blk in enumerate(random_blocks(seed, Nb)):
        n = max(N + 1 - slot_order(s), 0)
        bad = np.full(blk.shape, POISON)
        bad[:n, :n] = blk[:n, :n]
        out.append(bad)
    return out


def coefficient_batch(seed, N, B):
    """[B][N+1][N+1] of N(0, 1) * 1e-10, epoch e = inputs.coefficients(seed + e, N)"""
    return np.stack([inputs.coefficients(seed + e, N) for e in range(B)])


# ---- solvers ---------------------------------------------------------------------------------------------------------------------

def solve_bound(d):
    """d gamma(3 d + 1): the cap of solve_residual for a Cholesky solve of dimension d in fp64"""
    return float(LD(d) * gamma(3 * d + 1))


def solve_residual(A, X, B):
    """||A X - B||_F / (||A||_F ||X||_F) in long double"""
    A, X, B = (np.asarray(v, dtype=np.float64).astype(LD) for v in (A, X, B))
    if X.ndim == 1:
        X, B = X[:, np.newaxis], B[:, np.newaxis]
    den = np.sqrt(np.sum(A * A)) * np.sqrt(np.sum(X * X))
    num = np.sqrt(np.sum((A @ X - B) ** 2))
    return float(num / den) if den > 0 else float(num)


def solve_residual_columns(A, X, B):
    """the same measure column by column, ||A x - b||_2 / (||A||_F ||x||_2): [k]; the bound holds for every column on its own"""
    A, X, B = (np.asarray(v, dtype=np.float64).astype(LD) for v in (A, X, B))
    den = np.sqrt(np.sum(A * A)) * np.sqrt(np.sum(X * X, axis=0))
    num = np.sqrt(np.sum((A @ X - B) ** 2, axis=0))
    return np.where(den > 0, num / np.where(den > 0, den, 1), num).astype(np.float64)


SPD_CASES = [(1, 1), (5, 3), (40, 256), (40, 257), (33, 600), (165, 165)]      # (n, k): one column tile, its end, a second, a third ragged one


def spd_case(n, k):
    """A = inputs.spd_covariance(seed, n, scale=1.0) + I, B ~ N(0, 1) [n][k]"""
    A = inputs.spd_covariance(1000 + n, n, scale=1.0) + np.eye(n)
    return A, np.random.default_rng(2000 + 7 * n + k).standard_normal((n, k))


DDK_DEGREES = [0, 1, 2, 5, 40, 120]
DDK5_SCALE = 1e11


def ddk_case(Nb):
    """(normal blocks, weights) of a DDK5-type construction at degree Nb: inputs.orderwise_normal_blocks and w_0 = 1, w_n = 1e11 n^4"""
    w = DDK5_SCALE * np.arange(Nb + 1, dtype=float) ** 4
    w[0] = 1
    return inputs.orderwise_normal_blocks(3000 + Nb, Nb), w
