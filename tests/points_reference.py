"""
Long-double reference of the point-list family (shg_synthesis_points, shg_covprop_points, shg_synthesis_matrix and the pointwise
branch of shg_synthesis_matrix_order), shared by tests/test_points_reference_cpu.py (the reference against the float64 oracle, no
GPU) and tests/test_gpu_points.py (the kernels against the reference).  No GPU import.

It works from the tables the C ABI takes -- colat [npts], lon [npts], kn [npts][N+1], all float64 and taken as exact -- and does
everything else in np.longdouble: cos / sin of the long-double angles, recursion factors as sqrt of long-double rationals, the
standard fully normalised column recursion
    P_00 = 1,  P_11 = sqrt(3) s,  P_mm = sqrt((2m+1) / (2m)) s P_m-1,m-1,
    P_nm = a_nm t P_n-1,m - b_nm P_n-2,m,   a_nm = sqrt((2n-1)(2n+1) / ((n-m)(n+m))),
                                            b_nm = sqrt((2n+1)(n-m-1)(n+m-1) / ((2n-3)(n-m)(n+m)))
with t = cos(colat), s = sin(colat) (never sqrt(1 - t^2): 1e-9 from a pole that has no correct digit even in long double).
Columns are in the degree-wise order of shg_ravel: C_n0, C_n1, S_n1, C_n2, S_n2, ... for n = nmin .. N.
"""

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, \
    'tests/points_reference.py needs an extended-precision np.longdouble (eps < 1e-18, x87 80-bit or wider); this platform has eps = {0}'.format(np.finfo(LD).eps)

POINT_SEED, KN_SEED = 7, 11             # base_points / degree_factors of both test modules
TOL_VALUES = 1e-12                      # synthesis values, max-norm per epoch: the TOL of tests/test_gpu_synthesis.py
TOL_SIGMA = 1e-11                       # the TOL_SIGMA of tests/test_gpu_covariance.py

# The special entries at the head of base_points: both poles, the equator, 1e-9 rad from the pole (t rounds to 1 in float64 and
# the sectorials underflow from m = 35 on), 1e-3 rad from either pole; longitudes on the antimeridian with both signs, 0 and 3.0.
SPECIAL_COLAT = np.array([0.0, np.pi, 0.5 * np.pi, 1e-9, 1e-3, np.pi - 1e-3])
SPECIAL_LON = np.array([np.pi, -np.pi, 0.0, 3.0, -np.pi, np.pi])


def base_points(seed, count):
    """(colat, lon) float64 [count]: the special entries first, the rest scattered (colatitude = acos of a uniform draw).  A shorter
    list of the same seed is the head of a longer one."""
    draw = np.random.default_rng(seed).uniform(-1.0, 1.0, (count, 2))
    colat, lon = np.arccos(draw[:, 0]), np.pi * draw[:, 1]
    k = min(count, SPECIAL_COLAT.size)
    colat[:k] = SPECIAL_COLAT[:k]
    lon[:k] = SPECIAL_LON[:k]
    return colat, lon


def degree_factors(seed, N, count):
    """kn [count][N+1] float64, kn[p][n] = q_p^(n+1) with q_p in [0.97, 1.0]: every row differs (a transposed or shifted knT shows), the
    rows of one seed start alike for every N."""
    q = np.random.default_rng(seed).uniform(0.97, 1.0, count)
    return np.power(q[:, None], np.arange(1, N + 2, dtype=float)[None, :])


def general_covariance(S):
    """S plus an antisymmetric part: a^T (S + K) a = a^T S a stays positive, but a product that reads one triangle only (the
    symmetric shortcut of the regular-grid kernel) sees S + 0.6 triu(S, 1) - ... and gives another number."""
    K = 0.3 * np.triu(S, 1)
    return S + K - K.T


def _angles(colat, lon):
    th, lam = np.atleast_1d(np.asarray(colat, dtype=np.float64)).astype(LD), np.atleast_1d(np.asarray(lon, dtype=np.float64)).astype(LD)
    return np.cos(th), np.sin(th), lam


def _sectorials(N, s):
    """P_mm [N+1][npts]"""
    out = np.empty((N + 1, s.size), dtype=LD)
    out[0] = LD(1)
    for m in range(1, N + 1):
        out[m] = np.sqrt(LD(3)) * s if m == 1 else np.sqrt(LD(2 * m + 1) / LD(2 * m)) * s * out[m - 1]
    return out


def _column(N, m, t, pmm, kn):
    """kn[p][n] P_nm(p) for n = m .. N: [npts][N + 1 - m]"""
    out = np.empty((t.size, N + 1 - m), dtype=LD)
    p1, p2 = pmm, np.zeros_like(pmm)
    out[:, 0] = p1
    for n in range(m + 1, N + 1):
        a = np.sqrt(LD((2 * n - 1) * (2 * n + 1)) / LD((n - m) * (n + m)))
        b = np.sqrt(LD((2 * n + 1) * (n - m - 1) * (n + m - 1)) / LD((2 * n - 3) * (n - m) * (n + m))) if n > m + 1 else LD(0)
        p1, p2 = a * t * p1 - b * p2, p1
        out[:, n - m] = p1
    return out * kn[:, m:]


def _orders(N, colat, lon, kn):
    """yields (m, PK [npts][N+1-m], cos(m lon) [npts], sin(m lon) [npts])"""
    t, s, lam = _angles(colat, lon)
    k = np.asarray(kn, dtype=np.float64).astype(LD)
    assert k.shape == (t.size, N + 1) and lam.size == t.size
    pmm = _sectorials(N, s)
    for m in range(N + 1):
        yield m, _column(N, m, t, pmm[m], k), np.cos(LD(m) * lam), np.sin(LD(m) * lam)


def harmonic_rows(N, nmin, colat, lon, kn):
    """A [npts][(N+1)^2 - nmin^2] (long double): A[p][n^2 - nmin^2 + r] = kn[p][n] P_nm(colat_p) cos|sin(m lon_p), r = 0 for m = 0,
    2m - 1 for the cosine and 2m for the sine of order m."""
    npts = np.atleast_1d(colat).size
    A = np.zeros((npts, (N + 1) ** 2 - nmin ** 2), dtype=LD)
    for m, pk, c, s in _orders(N, colat, lon, kn):
        n0 = max(m, nmin)
        if n0 > N:
            continue
        n = np.arange(n0, N + 1)
        base = n * n - nmin * nmin
        if m == 0:
            A[:, base] = pk[:, n0 - m:]
        else:
            A[:, base + 2 * m - 1] = pk[:, n0 - m:] * c[:, None]
            A[:, base + 2 * m] = pk[:, n0 - m:] * s[:, None]
    return A


def synthesis(anm, colat, lon, kn):
    """values [npts] (long double) of one epoch anm [N+1][N+1] (C_nm at [n][m], S_nm at [m-1][n])."""
    x = np.asarray(anm, dtype=np.float64).astype(LD)
    N = x.shape[0] - 1
    values = np.zeros(np.atleast_1d(colat).size, dtype=LD)
    for m, pk, c, s in _orders(N, colat, lon, kn):
        values += c * (pk @ x[m:, m])
        if m > 0:
            values += s * (pk @ x[m - 1, m:])
    return values


def sigma(cov, nmin, N, colat, lon, kn):
    """sqrt(a_p^T cov a_p) [npts] (long double) with the full matrix cov [(N+1)^2 - nmin^2]^2, symmetric or not."""
    A = harmonic_rows(N, nmin, colat, lon, kn)
    if A.shape[1] == 0:
        return np.zeros(A.shape[0], dtype=LD)
    S = np.asarray(cov, dtype=np.float64).astype(LD)
    return np.sqrt(np.einsum('ij,ij->i', A @ S, A))


def order_block(N, m, nmin, colat, lon, kn):
    """(cosine block, sine block) [npts][N + 1 - max(m, nmin)] of order m; the sine block of m = 0 is None."""
    t, s, lam = _angles(colat, lon)
    k = np.asarray(kn, dtype=np.float64).astype(LD)
    pk = _column(N, m, t, _sectorials(m, s)[m], k)[:, max(nmin - m, 0):]
    if m == 0:
        return pk, None
    return pk * np.cos(LD(m) * lam)[:, None], pk * np.sin(LD(m) * lam)[:, None]


def order_columns(N, m, nmin):
    """columns of harmonic_rows(N, nmin, ...) that hold the cosine and the sine block of order m"""
    n = np.arange(max(m, nmin), N + 1)
    base = n * n - nmin * nmin
    return (base, None) if m == 0 else (base + 2 * m - 1, base + 2 * m)


def max_error(got, ref):
    """max|got - ref| / max|ref| (the relerr of tests/conftest.py) with the difference taken in long double"""
    ref = np.asarray(ref, dtype=LD)
    scale = np.max(np.abs(ref)) if ref.size else LD(0)
    diff = np.max(np.abs(np.asarray(got).astype(LD) - ref)) if ref.size else LD(0)
    return float(diff if scale == 0 else diff / scale)


def row_errors(got, ref, scale=None):
    """per point: max|row diff| / max|row ref| (the plain max|row diff| for a row of zeros); scale [npts] replaces max|row ref|"""
    ref = np.asarray(ref, dtype=LD)
    diff = np.max(np.abs(np.asarray(got).astype(LD) - ref), axis=1)
    scale = np.max(np.abs(ref), axis=1) if scale is None else np.asarray(scale, dtype=LD)
    return np.where(scale == 0, diff, diff / np.where(scale == 0, LD(1), scale)).astype(np.float64)
