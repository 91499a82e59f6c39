"""
The long-double reference of the point-list family (tests/points_reference.py) against the float64 oracle, without a GPU: the two
are independent restatements (long double / float64, sin / the oracle's own expressions, one recursion loop / the packed tables of
the reference), so their agreement pins the reference, and their difference is the error of a correct float64 evaluation -- the
figure the bounds of tests/test_gpu_points.py are set against.  Every figure is printed before it is asserted (pytest -s).

On base_points(7, 131) (both poles, the equator, 1e-9 and 1e-3 rad from a pole, 125 scattered points), kn = degree_factors(11):
    d/o   synthesis, max-norm per epoch   harmonic matrix, worst row (max|row diff| / max|row ref|)
     45            6.1e-15                         2.1e-14
    180            2.3e-14                         6.0e-14
    256            6.1e-14                         2.0e-13
    300            6.1e-14                         3.1e-13
The synthesis figures are below a quarter of the 1e-12 the device values are held to; the rows up to d/o 256 are below a quarter
of 1e-12 as well (points_bounds.matrix_row_bound), at d/o 300 the rule gives 1.24e-12.

The blocks of one order from the oracle's per-order recursion, beyond the share of its s = sqrt(1 - t^2) (points_bounds):
    d/o   order 0 (the worst row)   orders 1 | N/2 | N      points_bounds.block_row_bound
     45          2.4e-14                 7.3e-15                  1e-12
    180          2.3e-13                 4.4e-14                  1e-12
    256          5.8e-13                 5.4e-14                  2.32e-12
    300          7.0e-13                 9.3e-14                  2.8e-12
sigma: 3.3e-15 at d/o 20, 5.9e-15 at d/o 33, 1.4e-14 at d/o 45 from degree 30 (bound 1e-11).
The tables of points_bounds hold these figures; a new measurement may exceed them by a quarter (another libm's last bit of
cos(colat) at the worst point), not more.
"""

import numpy as np
import pytest

import inputs
import points_bounds as pb
import points_reference as pr
from oracle import shg_oracle as orc

NPTS = 131


def tables(N, npts=NPTS):
    colat, lon = pr.base_points(pr.POINT_SEED, npts)
    return colat, lon, pr.degree_factors(pr.KN_SEED, N, npts)


def test_lds_seams_of_the_recursion_kernel():
    """synthesis_points_kernel stages (N + 1) x 2 x 16 doubles = 256 (N + 1) bytes of coefficients per order: why the GPU cases
    run d/o 255 | 256 (the last request within 64 KB, the first that needs the opt-in) and d/o 640 (the first beyond the 160 KB
    of a CDNA4 compute unit)."""
    slab = lambda N: (N + 1) * 2 * 16 * 8
    assert slab(255) == 256 * (255 + 1) == 65536
    assert slab(256) == 65792 > 64 * 1024
    assert slab(639) == 160 * 1024 and 256 * (640 + 1) > 160 * 1024


def test_shared_inputs():
    colat, lon = pr.base_points(pr.POINT_SEED, NPTS)
    assert np.array_equal(colat[:6], [0.0, np.pi, 0.5 * np.pi, 1e-9, 1e-3, np.pi - 1e-3])
    assert {np.pi, -np.pi, 0.0, 3.0} <= set(lon[:6])
    assert np.all((colat >= 0) & (colat <= np.pi)) and np.all(np.abs(lon) <= np.pi) and np.unique(colat).size == NPTS
    short = pr.base_points(pr.POINT_SEED, 70)
    assert np.array_equal(short[0], colat[:70]) and np.array_equal(short[1], lon[:70])
    kn = pr.degree_factors(pr.KN_SEED, 45, NPTS)
    q = kn[:, 0]
    assert kn.shape == (NPTS, 46) and np.all((q >= 0.97) & (q <= 1.0)) and np.unique(q).size == NPTS
    np.testing.assert_allclose(kn[:, 45], q ** 46, rtol=1e-14)
    assert np.array_equal(pr.degree_factors(pr.KN_SEED, 20, 70), kn[:70, :21])


def test_reference_closed_forms():
    """Values that need no recursion: P_n0(1) = sqrt(2n + 1) at the pole, (-1)^n of it at the other, the sectorial
    P_nn = sqrt((2n + 1)!! / (2n)!!) sin^n and the addition theorem sum_m P_nm^2 = 2n + 1 at every point."""
    N = 60
    colat, lon = pr.base_points(pr.POINT_SEED, 40)
    ones = np.ones((40, N + 1))
    A = pr.harmonic_rows(N, 0, colat, lon, ones)
    n = np.arange(N + 1)
    assert pr.max_error(A[0, n * n], np.sqrt((2 * n + 1).astype(pr.LD))) < 1e-18
    assert pr.max_error(A[1, n * n], (-1.0) ** n * np.sqrt((2 * n + 1).astype(pr.LD))) < 1e-17
    for k in n:
        total = np.sum(A[:, k * k:(k + 1) * (k + 1)] ** 2, axis=1)
        assert float(np.max(np.abs(total / (2 * k + 1) - 1))) < 1e-16, k
    sect = np.sqrt(np.cumprod(np.concatenate(([pr.LD(1), pr.LD(3)], (2 * n[2:] + 1).astype(pr.LD) / (2 * n[2:]).astype(pr.LD)))))
    rc, rs = pr.order_block(N, N, 0, colat, lon, ones)
    expect = sect[N] * np.sin(colat.astype(pr.LD)) ** N
    assert pr.max_error(np.hypot(rc[:, 0], rs[:, 0]), expect) < 1e-17
    # the blocks of an order are columns of the matrix
    for m, nmin in ((0, 0), (1, 3), (7, 3), (60, 0)):
        rc, rs = pr.order_block(N, m, nmin, colat, lon, ones)
        cc, cs = pr.order_columns(N, m, nmin)
        An = pr.harmonic_rows(N, nmin, colat, lon, ones)
        assert np.array_equal(An[:, cc], rc) and (rs is None or np.array_equal(An[:, cs], rs))
    assert np.array_equal(pr.harmonic_rows(N, 7, colat, lon, ones), A[:, 49:])


@pytest.mark.parametrize('N', [45, 180, 256, 300])
def test_oracle_against_reference(N):
    colat, lon, kn = tables(N)
    A = pr.harmonic_rows(N, 0, colat, lon, kn)
    packed = orc.scale_packed_by_degree(orc.spherical_harmonics(N, colat, lon), kn)
    # synthesis: the oracle's sum (gravityfield.py:370-388) against the reference, two epochs; the reference's own two routes agree
    for e in (0, 1):
        anm = inputs.coefficients(300 + N + e, N)
        ref = pr.synthesis(anm, colat, lon, kn)
        assert pr.max_error(A @ orc.ravel_coefficients(anm, 0, N).astype(pr.LD), ref) < 1e-16
        values = np.zeros(NPTS)
        for k in range(N + 1):
            values += packed[:, k, :] @ anm[k, :]
        err = pr.max_error(values, ref)
        print('d/o {0} epoch {1}: synthesis of the oracle against the reference {2:.2e}'.format(N, e, err))
        assert err < 0.25 * pr.TOL_VALUES
    # harmonic matrix, per row
    rows = pr.row_errors(orc.ravel_coefficients(packed, 0, N), A)
    print('d/o {0}: worst row of the oracle {1:.2e} (point {2}), special points {3}, scattered {4:.2e}'.format(
        N, rows.max(), rows.argmax(), ' '.join('{0:.1e}'.format(v) for v in rows[:6]), rows[6:].max()))
    assert rows.max() <= pb.CEILING * pb.ORACLE_ROW_ERROR[N]             # the table the device bound is derived from still holds
    assert rows[6:].max() < 1e-13
    if N <= 256:
        assert pb.matrix_row_bound(N) == 1e-12 and rows.max() < 0.25e-12
    else:
        assert pb.matrix_row_bound(N) == 4.0 * pb.ORACLE_ROW_ERROR[N]


@pytest.mark.parametrize('N', [45, 180, 256, 300])
def test_oracle_order_blocks_against_reference(N):
    """The blocks of one order from the oracle's per-order recursion (synthesis_matrix_per_order_tables: s = sqrt(1 - t^2), order 0
    in its own coefficient form) against order_block, per row.  What a row is off beyond the share of the sine
    (points_bounds.order_block_bound) is the oracle's block error: at most ORACLE_BLOCK_ERROR[N], from which block_row_bound(N)
    follows -- 1e-12 up to d/o 180, where every row is also within a quarter of its bound, 2.32e-12 at d/o 256 and 2.8e-12 at d/o
    300, where order 0 at 1e-3 rad from the south pole is 5.8e-13 and 7.0e-13 off.  Rows that float64 cannot hold are exactly 0."""
    colat, lon, kn = tables(N)
    base = pb.block_row_bound(N)
    assert base == (1e-12 if N <= 180 else 4.0 * pb.ORACLE_BLOCK_ERROR[N])
    worst = 0.0
    for m in (0, 1, N // 2, N):
        sine = pb.order_block_bound(0.0, m, colat)                          # the share of the sine alone
        bound = base + sine
        lost, zero = pb.lost_rows(m, colat), pb.zero_rows(m, colat)
        assert np.array_equal(lost, zero), m
        for nmin in (0, 2, 2 * N // 3):
            ref_c, ref_s = pr.order_block(N, m, nmin, colat, lon, kn)
            out = orc.synthesis_matrix_per_order_tables(m, nmin, N, colat, kn, np.zeros(1))
            pm = out if m == 0 else out[0]                              # lon = 0: cos = 1, the block without its longitude factor
            blocks = [(pm, ref_c)] if m == 0 else [(pm * np.cos(m * lon)[:, None], ref_c), (pm * np.sin(m * lon)[:, None], ref_s)]
            errors = pb.block_row_errors(blocks[0][0], blocks[-1][0] if m else None, ref_c, ref_s)
            for (got, _), e in zip(blocks, errors):
                assert got.shape == ref_c.shape and not got[zero].any(), (m, nmin)
                own = float(np.max((e - sine)[~lost]))
                print('d/o {0} order {1} from degree {2}: block rows of the oracle {3:.2e} beyond the sine (point {4}), {5:.3f} of the bound; '
                      '{6} rows exactly 0'.format(N, m, nmin, own, int(np.argmax(np.where(lost, -1.0, e - sine))), float(np.max((e / bound)[~lost])),
                                                  int(zero.sum())))
                assert np.all(e[lost] <= bound[lost]), (m, nmin)
                assert own <= pb.CEILING * pb.ORACLE_BLOCK_ERROR[N], (m, nmin, own)
                if m:
                    assert own < 1e-13, (m, nmin, own)
                if N <= 180:
                    assert np.all(e[~lost] < 0.25 * bound[~lost]), (m, nmin)
                worst = max(worst, own)
    print('d/o {0}: block error of the oracle {1:.2e}, bound of the device {2:.2e} + sine'.format(N, worst, base))


@pytest.mark.parametrize('N,nmins', [(20, (0, 2)), (33, (0, 2)), (45, (30,))])
def test_oracle_sigma_against_reference(N, nmins):
    """sqrt(a^T Sigma a) as covariance_propagation_points forms it (grid.py:1096-1120) from the same tables, symmetric and general
    Sigma, at the degrees of the device cases and at d/o 45 from degree 30 (1216 parameters).  Not at d/o 180, 256 and 300: the
    long-double product is 2 npts P^2 operations without a BLAS, and from d/o 180 on the matrix alone is 8.6 GB; the harmonic rows
    that enter the product are compared at those degrees by test_oracle_against_reference."""
    colat, lon, kn = tables(N)
    for nmin in nmins:
        P = (N + 1) ** 2 - nmin ** 2
        S = inputs.spd_covariance(40 + N, P)
        # both kinds at d/o 20; one each at d/o 33 and the general one at d/o 45, where a product takes seconds
        kinds = (S, pr.general_covariance(S)) if N == 20 else (S,) if (N, nmin) == (33, 2) else (pr.general_covariance(S),)
        for cov in kinds:
            F = orc.ravel_coefficients(orc.scale_packed_by_degree(orc.spherical_harmonics(N, colat, lon), kn), nmin, N)
            got = np.sqrt(np.einsum('ij,ij->i', F @ cov, F))
            err = pr.max_error(got, pr.sigma(cov, nmin, N, colat, lon, kn))
            print('d/o {0} from degree {1}: sigma of the oracle against the reference {2:.2e}'.format(N, nmin, err))
            assert err < 0.25 * pr.TOL_SIGMA
    assert not pr.sigma(np.zeros((0, 0)), N + 1, N, colat, lon, kn).any()
