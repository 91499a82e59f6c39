"""
Long-double reference of covariance propagation on regular grids (shg_covprop_diag, shg_covprop_diag_symmetric,
shg_covprop_diag_separable, shg_covprop_diag_separable_symmetric), the case lists of tests/test_gpu_covariance_routes.py and the
route table of the direct kernels written out in Python.  Shared by tests/test_covariance_reference_cpu.py (no GPU) and the GPU
module.  No GPU import.

A grid is the point list (colat_i, lon_j, kn_i) of tests/points_reference.py: sigma(i, j) = sqrt(a_ij^T Sigma a_ij) with the row
a_ij of the synthesis matrix in np.longdouble, for any matrix, symmetric or not.
"""

import functools

import numpy as np

import points_reference as pr

LD = pr.LD
GRID_SEED = 23
SPECIAL_COLAT = np.array([0.0, np.pi, 0.5 * np.pi, 1e-3])
ODD_MERIDIAN = 0.7390851332151607            # the fixed point of cos: no multiple of pi / k for any small k


def grid_tables(seed, N, nlat, nlon):
    """colat [nlat], kn [nlat][N+1], meridians [nlon] (float64).  Colatitudes: both poles, the equator and 1e-3 rad first (as far
    as nlat allows), the rest scattered, all distinct and in no order; the tables of a smaller nlat are the head of those of a larger
    one.  kn: pr.degree_factors, every parallel differs.  Meridians: irregular and sorted, with -pi and ODD_MERIDIAN among them, so
    that neither a longitude symmetry of the plan nor a swap of two columns cancels."""
    colat = np.random.default_rng([seed, 1]).uniform(0.05, np.pi - 0.05, nlat)
    k = min(nlat, SPECIAL_COLAT.size)
    colat[:k] = SPECIAL_COLAT[:k]
    assert np.unique(colat).size == nlat
    kn = pr.degree_factors(seed, N, nlat)
    lon = np.random.default_rng([seed, 2, nlon]).uniform(-np.pi, np.pi, nlon)
    lon[0] = -np.pi
    if nlon > 1:
        lon[1] = ODD_MERIDIAN
    lon = np.sort(lon)
    assert np.unique(lon).size == nlon
    return colat, kn, lon


def general_matrix(seed, P, eps=0.05):
    """diag(d) + eps E [P][P]: d uniform in [0.5, 1.5] with distinct entries, E standard normal and not symmetric: a wrong diagonal
    entry, a swapped pair and a transposed tile all change a^T Sigma a, which stays near |a|^2."""
    rng = np.random.default_rng([seed, P])
    d = rng.uniform(0.5, 1.5, P)
    assert np.unique(d).size == P
    S = rng.standard_normal((P, P))
    S *= eps
    S[np.diag_indices(P)] += d
    return S


def symmetric_matrix(seed, P, eps=0.05):
    """the same with (E + E^T) / 2: exactly symmetric"""
    S = general_matrix(seed, P, eps)
    d = np.diag(S).copy()
    S = 0.5 * (S + S.T)
    S[np.diag_indices(P)] = d
    assert np.array_equal(S, S.T)
    return S


def grid_points(colat, kn, meridians, rows=None):
    """(colat, lon, kn) of the flat grid rows r = i * nlon + j (all of them for rows=None)"""
    nlon = meridians.size
    rows = np.arange(colat.size * nlon) if rows is None else np.asarray(rows, dtype=np.int64)
    i, j = rows // nlon, rows % nlon
    return colat[i], meridians[j], kn[i]


def sigma_grid(cov, nmin, N, colat, kn, meridians, rows=None, chunk=512, with_norm=False):
    """sqrt(a^T cov a) (long double) for all grid rows (row-major, [nlat * nlon]) or for the listed flat rows.  Accumulates over row
    chunks of cov: no long-double copy of a whole large matrix is made.  with_norm: also |a|^2."""
    th, lam, k = grid_points(np.asarray(colat), np.asarray(kn), np.asarray(meridians), rows)
    A = pr.harmonic_rows(N, nmin, th, lam, k)
    P = A.shape[1]
    q = np.zeros(A.shape[0], dtype=LD)
    cov = np.asarray(cov)
    assert cov.shape == (P, P)
    for c0 in range(0, P, chunk):
        q += np.einsum('ij,ij->i', A[:, c0:c0 + chunk] @ cov[c0:c0 + chunk].astype(LD), A)
    out = np.sqrt(q)
    return (out, np.einsum('ij,ij->i', A, A)) if with_norm else out


# ---- the route of the direct kernels (csrc/gemm.hip: covprop_route), written out
ROUTES = ('NONE', 'ROWS', 'DIRECT', 'REGISTER', 'PADDED', 'SYMMETRIC')


def route(nlon, P, aligned, M, symmetric):
    """nlon meridians, P x P matrix at a base that is (aligned) or is not a multiple of 16 bytes, M grid rows in the band"""
    if P == 0 or M == 0:
        return 'NONE'
    if symmetric:
        return 'SYMMETRIC'
    padding = -nlon % 128
    if 25 * padding <= nlon:                        # nlon 124 .. 128, 247 .. 256, 370 .. 384, ...
        return 'ROWS'
    if P % 2 == 0 and aligned:
        return 'DIRECT'
    return 'PADDED' if float(M) * P * P > 1e12 else 'REGISTER'


def padded_row_length(P):
    """leading dimension of the padded copy: even, and no multiple of 512 doubles"""
    ld = P + (P & 1)
    return ld + 2 if ld % 512 == 0 else ld


# ---- case lists of the GPU module
DEGREE_PAIRS = ((0, 0), (2, 0), (3, 0), (4, 2), (11, 4), (22, 20), (15, 0), (16, 0), (17, 0))          # (N, nmin)
PAIR_SIZES = (1, 9, 16, 21, 128, 129, 256, 289, 324)
ROWS_NLON, ROWS_NLAT, ROWS_BANDS = (124, 127, 128, 247, 256), 3, ((0, 3), (1, 3), (1, 2))
GENERAL_SHAPES = ((1, 130), (3, 43), (123, 2), (129, 1), (129, 2), (130, 3))                           # (nlon, nlat)
SYMMETRIC_PAIRS = ((0, 0), (4, 2), (11, 4), (22, 20), (16, 0), (17, 0))                               # P = 1, 21, 128, 129, 289, 324
PADDED_PAIRS, PADDED_GRID = ((62, 0), (63, 1)), (360, 180)                                           # P = 3969, 4095; (nlon, nlat)
SEPARABLE_DEGREES, SEPARABLE_NLAT, SEPARABLE_NLON, SEPARABLE_NB, SEPARABLE_LAT0 = (0, 2, 15, 16, 31, 32), 35, 5, (1, 31, 33), 2
PERMUTE_CASE = (90, 0, 2, 3)                                                                          # N, nmin, nlat, nlon: P = 8281


def size(N, nmin):
    return (N + 1) ** 2 - nmin ** 2


def general_bands(nlat):
    """the full grid, a band that ends at the last parallel and one that does not (both with lat0 > 0 where nlat allows)"""
    if nlat == 1:
        return ((0, 1),)
    return ((0, nlat), (nlat // 2, nlat), (nlat // 3, nlat - 1))


def separable_pairs():
    """(N, nmin) with nmin in {0, 3, N}, as far as nmin <= N + 1"""
    out = []
    for N in SEPARABLE_DEGREES:
        for nmin in (0, 3, N):
            if nmin <= N + 1 and (N, nmin) not in out:
                out.append((N, nmin))
    return out


def padded_rows():
    """16 flat rows of the PADDED_GRID: its first and last row, both sides of a 128-row block seam and of a parallel seam, and others"""
    nlon, nlat = PADDED_GRID
    last = nlon * nlat - 1
    rows = [0, last, 127, 128, nlon - 1, nlon, 64 * 128 - 1, 64 * 128, 90 * nlon - 1, 90 * nlon, last - nlon, last - nlon + 1, 1, 129, 33333, 47111]
    assert len(set(rows)) == 16 and max(rows) == last
    return np.array(rows)


def slots(N, nmin):
    """slot (rank inside its degree) of every degree-wise index of an (N, nmin) matrix"""
    return np.concatenate([np.arange(2 * n + 1) for n in range(nmin, N + 1)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def small_matrix(kind, P):
    """the matrix of a case (P <= 1100), shared and never modified"""
    assert P <= 1100
    S = {'general': general_matrix, 'symmetric': symmetric_matrix}[kind](1000 + P, P)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def grid_reference(kind, N, nmin, nlat, nlon):
    """(sigma, |a|^2) in long double on the whole grid_tables(GRID_SEED, N, nlat, nlon) grid with small_matrix(kind, P); computed
    once per session and never modified"""
    colat, kn, lon = grid_tables(GRID_SEED, N, nlat, nlon)
    ref, norm = sigma_grid(small_matrix(kind, size(N, nmin)), nmin, N, colat, kn, lon, with_norm=True)
    ref.setflags(write=False)
    norm.setflags(write=False)
    return ref, norm


def small_references():
    """every (kind, N, nmin, nlat, nlon) the GPU module takes from grid_reference"""
    out = []
    for N, nmin in DEGREE_PAIRS:
        out += [('general', N, nmin, ROWS_NLAT, nlon) for nlon in ROWS_NLON]
        out += [('general', N, nmin, nlat, nlon) for nlon, nlat in GENERAL_SHAPES]
    for N, nmin in SYMMETRIC_PAIRS:
        out += [('symmetric', N, nmin, nlat, nlon) for nlon, nlat in GENERAL_SHAPES]
    for N, nmin in separable_pairs():
        if size(N, nmin) > 0:
            out += [(kind, N, nmin, SEPARABLE_NLAT, SEPARABLE_NLON) for kind in ('general', 'symmetric')]
    return out


def assert_positive(ref, norm, what):
    """the condition every case checks on the reference before it looks at the GPU: a^T Sigma a > |a|^2 / 2"""
    assert np.all(ref ** 2 > 0.5 * norm), '{0}: a^T Sigma a / |a|^2 falls to {1:.3f}'.format(what, float(np.min(ref ** 2 / norm)))
