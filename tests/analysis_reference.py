"""
A plain high-precision reference of the regular-grid analysis for ALL orders, and the grids of the analysis branch tests
(tests/test_gpu_analysis_branches.py, tests/test_analysis_reference_cpu.py).

The oracle (orc.analysis_regular) forms the [nlat * nlon, d] design matrix of every order, which is why the tests at d/o 127 compare a
sample of the orders only.  The least-squares problem of a slot s = (m, cos | sin) is separable (header of csrc/analysis.hip):
    g[b][i] = sum_j area[i][j] v[b][i][j] T(m lon_j)        w2[i] = sum_j area[i][j] T(m lon_j)^2
    N_s = PK^T diag(w2) PK,   rhs = PK^T g,                 PK[i][n] = kn[i][n] P_nm(theta_i),  n = max(m, nmin) .. N
Here the sums over the meridians and the right-hand sides are formed in np.longdouble, the normal matrix is solved in float64 and
the solution is refined once with a residual PK^T (g - w2 (PK x)) formed in long double -- nothing of the library is used, PK comes
from the oracle's tables (orc.kn_table, orc.legendre_functions).  All orders of d/o 126 on a 128 x 256 grid take the CPU about a second.

Agreement with orc.analysis_regular on the orders [0, 1, 2, 3, N/2, N-1, N] (max |difference| / max |reference|) is measured and
asserted by tests/test_analysis_reference_cpu.py; the figures are in its docstring.
"""

import numpy as np

from oracle import shg_oracle as orc

LD = np.longdouble
GM, R = orc.GM_DEFAULT, orc.R_DEFAULT


# ---- grids ---------------------------------------------------------------------------------------------------------------------

def parallels(nlat):
    """cell-centred, equi-angular, north -> south"""
    return 0.5 * np.pi - (np.arange(nlat) + 0.5) * np.pi / nlat


def mirrored_meridians(nlon):
    """Cell-centred equi-angular meridians built from the quarter domain by mirroring, so that the three identities of the plan's
    four-fold symmetry test hold with difference exactly 0 (nlon a multiple of 4)."""
    assert nlon % 4 == 0
    q = (np.arange(nlon // 4) + 0.5) * 2.0 * np.pi / nlon
    return np.concatenate((q - np.pi, -q[::-1], q, (np.pi - q)[::-1]))


def plain_meridians(nlon):
    """cell-centred equi-angular meridians for any count (no symmetry is constructed)"""
    return (np.arange(nlon) + 0.5) * 2.0 * np.pi / nlon - np.pi


def weights(kind, nlat, nlon, seed):
    """'const': cos(lat), constant along every parallel; 'varying': cos(lat) * uniform(0.5, 1.5) per cell, which also breaks the
    north-south mirror symmetry"""
    w = np.tile(np.cos(parallels(nlat))[:, np.newaxis], (1, nlon))
    if kind == 'varying':
        w = w * np.random.default_rng(seed).uniform(0.5, 1.5, (nlat, nlon))
    else:
        assert kind == 'const'
    return w


class Case:
    """One grid of the branch tests.  transform: 'fused2' | 'fused3' | 'fused4' (analysis_transform_kernel<MT, .>), 'fold' (fold kernel +
    GEMMs) or 'plain' (weight transpose + GEMM); product: 'parity' | 'operator' | 'gemm' (gemm + scatter)."""

    def __init__(self, N, nmin, nlat, nlon, kind, transform, product, shift=0.0):
        self.N, self.nmin, self.nlat, self.nlon, self.kind = N, nmin, nlat, nlon, kind
        self.transform, self.product, self.shift = transform, product, shift
        self.id = 'N{0}-from{1}-{2}x{3}{4}-{5}-{6}-{7}'.format(N, nmin, nlat, nlon, '-shifted' if shift else '', kind, transform, product)

    @property
    def fourfold(self):
        return self.transform != 'plain'

    def meridians(self):
        return (mirrored_meridians(self.nlon) if self.nlon % 4 == 0 else plain_meridians(self.nlon)) + self.shift

    def parallels(self):
        return parallels(self.nlat)

    def seed(self):
        return 1000 * self.N + 10 * self.nlat + self.nmin + (5 if self.kind == 'varying' else 0)

    def area(self):
        return weights(self.kind, self.nlat, self.nlon, self.seed())

    def values(self, B):
        return np.random.default_rng(self.seed() + 1).standard_normal((B, self.nlat, self.nlon))


def both(N, nmin, nlat, nlon, transform, product_const, product_varying):
    return [Case(N, nmin, nlat, nlon, 'const', transform, product_const), Case(N, nmin, nlat, nlon, 'varying', transform, product_varying)]


# degree and shape seams: mt = N <= 64 ? 2 : (N <= 96 ? 3 : 4), the fused kernel up to N = 126, the batched factorisation up to
# R = N + 1 = 128, the operator kernels for R <= 128 and even nlat, the parity split for nlat % 4 == 0 and mirror-symmetric weights
SEAM_CASES = (
    both(64, 0, 66, 132, 'fused2', 'operator', 'operator')              # nq = 33: the last aligned column pair is half outside
    + both(65, 0, 67, 132, 'fused3', 'gemm', 'gemm')                      # lower edge of MT = 3, odd nlat
    + both(96, 3, 98, 196, 'fused3', 'operator', 'operator')            # upper edge, nq = 49
    + both(97, 2, 100, 196, 'fused4', 'parity', 'operator')             # lower edge of MT = 4
    + both(126, 0, 128, 256, 'fused4', 'parity', 'operator')            # upper edge: 63 orders per group, partial 4th tile; nq = 64
    + [Case(127, 4, 130, 256, 'varying', 'fold', 'operator')]           # R = 128: the largest batched factorisation
    + both(128, 0, 130, 260, 'fold', 'gemm', 'gemm')                      # R = 129: potrf / trtri loop, gemm + scatter
    + [Case(128, 2, 130, 259, 'varying', 'plain', 'gemm'),
       Case(65, 0, 67, 132, 'varying', 'plain', 'gemm', shift=0.05),
       Case(20, 20, 24, 44, 'const', 'fused2', 'parity')])              # every slot has one row

# batch seams (kAnaEpochChunk = 256 epochs per pass, 64 epochs per workgroup of the operator kernels)
BATCH_CASES = [Case(12, 1, 16, 28, 'const', 'fused2', 'parity'),
               Case(12, 1, 18, 28, 'varying', 'fused2', 'operator'),
               Case(12, 1, 17, 28, 'varying', 'fused2', 'gemm'),
               Case(12, 1, 18, 28, 'varying', 'plain', 'operator', shift=0.05)]

# dense operator: the same grid with both kinds of weights
DENSE_CASES = both(33, 2, 36, 68, 'fused2', 'parity', 'operator')

TRANSFORM_DEGREES = {'fused2': (0, 64), 'fused3': (65, 96), 'fused4': (97, 126), 'fold': (127, 1 << 30), 'plain': (0, 1 << 30)}


# ---- reference -----------------------------------------------------------------------------------------------------------------

def analysis(values, area, nmin, N, meridians, parallels, kernel='potential'):
    """values [B, nlat, nlon] (or [nlat, nlon]), area [nlat, nlon] -> anm [B, N+1, N+1] (float64); degrees below nmin stay zero."""
    v = np.asarray(values, dtype=float)
    if v.ndim == 2:
        v = v[np.newaxis]
    B, nlat, nlon = v.shape
    a = np.asarray(area, dtype=float).reshape(nlat, nlon).astype(LD)
    colat, _, kn = orc.kn_table(orc.KernelTable(kernel), N, np.asarray(parallels, dtype=float), GM, R)
    PK = orc.scale_packed_by_degree(orc.legendre_functions(N, colat), kn)              # kn P_nm at [i, n, m]
    lon = np.asarray(meridians, dtype=float).astype(LD)
    # trig table of all slots: 0 = order 0, 2m - 1 = cos m, 2m = sin m
    T = np.ones((nlon, 2 * N + 1), dtype=LD)
    for m in range(1, N + 1):
        T[:, 2 * m - 1] = np.cos(LD(m) * lon)
        T[:, 2 * m] = np.sin(LD(m) * lon)
    G = ((a[np.newaxis] * v.astype(LD)).reshape(B * nlat, nlon) @ T).reshape(B, nlat, 2 * N + 1)
    W2 = a @ (T * T)                                                                   # [nlat, S]
    out = np.zeros((B, N + 1, N + 1))
    for s in range(2 * N + 1):
        m = (s + 1) // 2
        n0 = max(m, nmin)
        pk = PK[:, n0:, m]                                                             # [nlat, d]
        pkl = pk.astype(LD)
        g, w2 = G[:, :, s].T, W2[:, s]                                                 # [nlat, B], [nlat]
        normal = (pk * w2.astype(float)[:, np.newaxis]).T @ pk
        x = np.linalg.solve(normal, (pkl.T @ g).astype(float)).astype(LD)
        residual = pkl.T @ (g - w2[:, np.newaxis] * (pkl @ x))
        x = (x + np.linalg.solve(normal, residual.astype(float)).astype(LD)).astype(float)
        if s > 0 and s % 2 == 0:
            out[:, m - 1, n0:] = x.T
        else:
            out[:, n0:, m] = x.T
    return out


def order_mask(N, nmin, orders):
    """the entries of anm that the slots of `orders` fill"""
    mask = np.zeros((N + 1, N + 1), dtype=bool)
    for m in orders:
        mask[max(m, nmin):, m] = True
        if m:
            mask[m - 1, max(m, nmin):] = True
    return mask


def sample_orders(N):
    return sorted(set([0, 1, 2, 3, N // 2, N - 1, N]) & set(range(N + 1)))
