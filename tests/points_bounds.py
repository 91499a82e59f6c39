"""
Bounds of the point-list tests, shared by tests/test_points_reference_cpu.py (which measures the float64 oracle against the
long-double reference of tests/points_reference.py and asserts the figures below) and tests/test_gpu_points.py (which holds the
device to the bounds derived from them).  No GPU import.

The rule, the convention of tests/test_gpu_design.py: a per-row bound is 1e-12 where the oracle's own per-row error is below a
quarter of it, and four times that error otherwise.  The two tables hold the oracle's error as measured on
base_points(POINT_SEED, 131) with degree_factors(KN_SEED, N, 131), rounded up to two digits.  The CPU test asserts that a new
measurement stays within CEILING of them: the figures hang on the last bit of cos(colat) at one point, which another libm may
round the other way, while a defect moves them by orders of magnitude.
"""

import numpy as np

import points_reference as pr

LD = pr.LD
U = 2.0 ** -53          # unit roundoff of float64
CEILING = 1.25          # a new measurement of a table entry may exceed it by this factor

# Harmonic matrix (spherical_harmonics + scale_packed_by_degree against harmonic_rows), worst row max|row diff| / max|row ref|.
# It is always the point 1e-3 rad from the south pole: half an ulp of t = cos(colat) there moves P_n0 by n (n + 1) / 2 * 2^-54 / |t|,
# 2e-12 of the value at d/o 256, of which the degree factors q^(n+1) of that row leave a tenth.  The scattered rows stay below 1e-13.
ORACLE_ROW_ERROR = {45: 2.1e-14, 180: 6.0e-14, 256: 2.0e-13, 300: 3.1e-13}
# Blocks of one order (synthesis_matrix_per_order_tables against order_block), worst row over orders 0 | 1 | N/2 | N and first
# degrees 0 | 2 | 2N/3, after the share of s = sqrt(1 - t^2) (order_block_bound) is taken off.  The worst is order 0 at the same
# point: the per-order recursion has its own coefficient form for m = 0, three times less accurate there than the column
# recursion.  Every order above 0 stays below 1e-13.
ORACLE_BLOCK_ERROR = {45: 2.4e-14, 180: 2.3e-13, 256: 5.8e-13, 300: 7.0e-13}


def _rule(table, max_degree):
    cap = min(n for n in table if n >= max_degree)                       # the first measured degree that covers max_degree
    worst = max(v for n, v in table.items() if n <= cap)
    return 1e-12 if worst < 0.25e-12 else 4.0 * worst


def matrix_row_bound(max_degree):
    """Per-row bound of the harmonic matrix on the device up to max_degree: 1e-12 up to d/o 256, 1.24e-12 at d/o 300."""
    return _rule(ORACLE_ROW_ERROR, max_degree)


def block_row_bound(max_degree):
    """Per-row bound of an order block up to max_degree, before the share of the sine: 1e-12 up to d/o 180, 2.32e-12 at d/o 256,
    2.8e-12 at d/o 300."""
    return _rule(ORACLE_BLOCK_ERROR, max_degree)


def sine_loss(colat):
    """Relative error bound of s = sqrt(1 - t^2), t = fl(cos(colat)), the sine of the per-order recursion (shg_legendre_order and
    the reference it restates), against sin(colat): t carries half an ulp (2^-54 below 1), t t and 1 - t t one rounding each, so
    |d(s^2)| <= 2 t 2^-54 + 2^-54 + 2^-53 s^2 < 2^-52 and |ds| / s < 2^-53 / s^2 (+ half an ulp of the root).  At 1e-3 rad from
    a pole that is 1.1e-10, at 1e-9 rad (t rounds to 1, s to 0) and at the poles themselves the sine has no digit left: 1."""
    s = np.abs(np.sin(np.asarray(colat, dtype=np.float64)))
    with np.errstate(divide='ignore'):
        return np.minimum(1.0, U / (s * s) + U)


def _seed(m, th):
    return np.abs(pr._sectorials(m, np.sin(th.astype(LD)))[m])


def lost_rows(m, colat):
    """Points whose order-m block (m >= 1) has no digit in float64 with s = sqrt(1 - t^2): the sine itself has none (the poles and
    1e-9 rad from one), or the seed P_mm lies below 2^-1022 / 2^-53 = 2e-292, so that the float64 chain of m products ends among
    the subnormals or at 0 while the long-double one carries on (m = 180 at 1e-3 rad from a pole: 1e-540)."""
    th = np.atleast_1d(np.asarray(colat, dtype=np.float64))
    if m == 0:
        return np.zeros(th.size, dtype=bool)
    return (sine_loss(th) >= 1.0) | (_seed(m, th) < LD(2.0 ** -1022) / LD(U))


def zero_rows(m, colat):
    """Points whose order-m block (m >= 1) is exactly 0 in float64: fl(1 - t t) = 0 with t = fl(cos(colat)) (t = +-1: the poles,
    and 1e-9 rad from one, where 1 - cos = 5e-19 is a 200th of the spacing of the doubles below 1), or a seed below 2^-1080, a
    64th of the smallest subnormal, which the chain of m products cannot reach: from there on every entry of the row is an exact
    0 times a finite number.  In the cases of both test modules these are all of lost_rows."""
    th = np.atleast_1d(np.asarray(colat, dtype=np.float64))
    if m == 0:
        return np.zeros(th.size, dtype=bool)
    t = np.cos(th)
    return (1.0 - t * t == 0.0) | (_seed(m, th) < LD(2.0) ** -1080)


def order_block_bound(base, m, colat):
    """Bound per point of the row error of an order-m block from the per-order recursion: the block is proportional to s^m (the
    sectorial seed; t enters the recursion as in every other path), so its rows inherit (1 + sine_loss)^m - 1 on top of `base`.
    The rows of lost_rows get 1 + base, the error of an exact 0 against the reference; the tests ask for that exact 0 too (zero_rows)."""
    th = np.atleast_1d(np.asarray(colat, dtype=np.float64))
    if m == 0:
        return np.full(th.size, float(base))
    e = sine_loss(th)
    return base + np.where(lost_rows(m, th), 1.0, np.expm1(m * np.log1p(np.minimum(e, 0.5))))


def block_row_errors(got_cos, got_sin, ref_cos, ref_sin):
    """Row errors of the cosine and the sine block of one order, both against max(|cosine row ref|, |sine row ref|) of the point:
    cos(m lon) and sin(m lon) carry the absolute error m |lon| 2^-53 of the rounded argument, which is relative to 1, not to a
    cosine that happens to vanish at the point's longitude; the pair's scale is at least 0.7 max|kn P_nm|."""
    if ref_sin is None:
        return pr.row_errors(got_cos, ref_cos), None
    scale = np.maximum(np.max(np.abs(ref_cos), axis=1), np.max(np.abs(ref_sin), axis=1))
    return pr.row_errors(got_cos, ref_cos, scale), pr.row_errors(got_sin, ref_sin, scale)
