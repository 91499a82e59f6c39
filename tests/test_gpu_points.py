"""
The point-list family on the device -- shg_synthesis_points, shg_covprop_points, shg_synthesis_matrix and the pointwise branch of
shg_synthesis_matrix_order, straight through the C ABI -- against the long-double reference of tests/points_reference.py: high
degrees, the poles, the launch seams of the recursion kernel, the dispatch seam at 48 epochs and the second and third trip of the
chunk loops.  Every output buffer is filled with NaN before the call, so an entry the library leaves unwritten fails its check.

Bounds (tests/test_points_reference_cpu.py measures the float64 oracle against the same reference and asserts these figures):
  * synthesis values: max-norm per epoch < 1e-12, the TOL of test_gpu_synthesis.py; the oracle itself is within 6.1e-14 up to d/o 300;
  * sigma < 1e-11, the TOL_SIGMA of test_gpu_covariance.py (oracle: 5.9e-15);
  * matrix rows, per point, max|row diff| / max|row ref|: the oracle's worst row is 2.1e-14 at d/o 45, 6.0e-14 at d/o 180 and
    2.0e-13 at d/o 256 (always the point 1e-3 rad from the south pole, where half an ulp of cos(colat) is worth that much), below
    a quarter of 1e-12, so the bound is 1e-12 (points_bounds.matrix_row_bound; it would be 1.24e-12 at d/o 300, which no
    matrix case here reaches);
  * blocks of shg_synthesis_matrix_order at d/o 180: the oracle's own blocks are 2.3e-13 off (order 0, the same point), below a
    quarter of 1e-12, so 1e-12 again (points_bounds.block_row_bound; 2.32e-12 at d/o 256, 2.8e-12 at d/o 300), plus what
    s = sqrt(1 - t^2) loses against sin(colat) near a pole, (1 + 2^-53 / sin^2)^m - 1 (points_bounds.order_block_bound: 1.1e-10 m
    at 1e-3 rad); the cosine and the sine block of a point share max(|cos row|, |sin row|) as scale.  Where float64 cannot hold
    the block -- s = 0 at the poles and 1e-9 rad from one, P_180,180 = 1e-540 at 1e-3 rad -- it has to be exactly 0
    (points_bounds.zero_rows).
Measured on an MI355X: see DESIGN.md 4.5, "point lists: limits".
"""

import functools

import numpy as np
import pytest

import inputs
import points_bounds as pb
import points_reference as pr
from grates_amd import _lib, engine
from oracle import shg_oracle as orc

pytestmark = pytest.mark.gpu
TOL = pr.TOL_VALUES
ROW_TOL = pb.matrix_row_bound(256)
BLOCK_TOL = pb.block_row_bound(180)
assert ROW_TOL == 1e-12 and BLOCK_TOL == 1e-12
NEPOCHS = 49


def tables(N, npts):
    colat, lon = pr.base_points(pr.POINT_SEED, npts)
    return colat, lon, pr.degree_factors(pr.KN_SEED, N, npts)


@functools.lru_cache(maxsize=None)
def epochs(N, count=NEPOCHS):
    return np.stack([inputs.coefficients(500 + e, N) for e in range(count)])


@functools.lru_cache(maxsize=None)
def reference_values(N, npts, which):
    """long-double values [len(which)][npts] of the epochs `which` of epochs(N) on the first npts base points: one pass over the
    harmonic rows, shared by every case of that degree"""
    colat, lon, kn = tables(N, npts)
    x = orc.ravel_coefficients(epochs(N)[list(which)], 0, N).astype(pr.LD)
    return (pr.harmonic_rows(N, 0, colat, lon, kn) @ x.T).T


def nan_filled(shape):
    torch = engine.require_gpu()
    return torch.full(shape, float('nan'), dtype=torch.float64, device=engine.device())


def synthesis_points(N, colat, lon, kn, anm):
    th, lam, k, x = engine.to_device(colat), engine.to_device(lon), engine.to_device(kn), engine.to_device(anm)
    out = nan_filled((x.shape[0], th.numel()))
    _lib.call('shg_synthesis_points', N, engine._ptr(th), engine._ptr(lam), engine._ptr(k), th.numel(), engine._ptr(x), x.shape[0], engine._ptr(out),
              engine._stream())
    return engine.to_host(out)


def synthesis_matrix(N, nmin, colat, lon, kn):
    th, lam, k = engine.to_device(colat), engine.to_device(lon), engine.to_device(kn)
    out = nan_filled((th.numel(), (N + 1) ** 2 - nmin ** 2))
    _lib.call('shg_synthesis_matrix', N, nmin, engine._ptr(th), engine._ptr(lam), engine._ptr(k), th.numel(), engine._ptr(out), engine._stream())
    return engine.to_host(out)


def matrix_order(N, m, nmin, colat, lon, kn):
    th, lam, k = engine.to_device(colat), engine.to_device(lon), engine.to_device(kn)
    cnt = N + 1 - max(m, nmin)
    out_c = nan_filled((th.numel(), cnt))
    out_s = nan_filled((th.numel(), cnt)) if m > 0 else None
    _lib.call('shg_synthesis_matrix_order', N, m, nmin, engine._ptr(th), th.numel(), engine._ptr(lam), th.numel(), engine._ptr(k), 1, engine._ptr(out_c),
              engine._ptr(out_s) if m > 0 else None, engine._stream())
    return engine.to_host(out_c), (engine.to_host(out_s) if m > 0 else None)


def covprop_points(N, nmin, colat, lon, kn, cov):
    th, lam, k = engine.to_device(colat), engine.to_device(lon), engine.to_device(kn)
    c = engine.to_device(cov) if cov.size else None
    out = nan_filled((th.numel(),))
    _lib.call('shg_covprop_points', N, engine._ptr(th), engine._ptr(lam), engine._ptr(k), th.numel(), engine._ptr(c) if c is not None else None, nmin,
              engine._ptr(out), engine._stream())
    return engine.to_host(out)


def check_values(got, ref, what):
    """every epoch of got against ref; returns the worst error"""
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    worst = 0.0
    for e in range(ref.shape[0]):
        err = pr.max_error(got[e], ref[e])
        assert err < TOL, (what, e, err)
        worst = max(worst, err)
    return worst


SEAM_POINTS = (1, 63, 64, 65, 130)


@pytest.mark.parametrize('N', [0, 1, 45])
def test_launch_seams_of_the_recursion_kernel(N):
    """One wave is 64 points and a pass 16 epochs: 1 | 63 | 64 | 65 | 130 points x 1 | 15 | 16 | 17 | 47 epochs, every epoch
    against the reference (the first points are the poles, the equator and the near-polar ones)."""
    ref = reference_values(N, 130, tuple(range(NEPOCHS)))
    colat, lon, kn = tables(N, 130)
    worst = 0.0
    for npts in SEAM_POINTS:
        for B in (1, 15, 16, 17, 47):
            got = synthesis_points(N, colat[:npts], lon[:npts], kn[:npts], epochs(N)[:B])
            worst = max(worst, check_values(got, ref[:B, :npts], (N, npts, B)))
    print('d/o {0}: recursion kernel, worst epoch {1:.2e}'.format(N, worst))


@pytest.mark.parametrize('N', [0, 1, 45])
def test_dispatch_seam_at_48_epochs(N):
    """48 and 49 epochs take the GEMM path (harmonic rows generated inside the MFMA kernel): against the reference, and epochs
    0 .. 46 against the recursion kernel's result for 47 epochs to 1e-13, the bound test_point_list_many_epochs holds the two paths to."""
    ref = reference_values(N, 130, tuple(range(NEPOCHS)))
    colat, lon, kn = tables(N, 130)
    worst, apart = 0.0, 0.0
    for npts in SEAM_POINTS:
        short = synthesis_points(N, colat[:npts], lon[:npts], kn[:npts], epochs(N)[:47])
        check_values(short, ref[:47, :npts], (N, npts, 47))
        for B in (48, 49):
            got = synthesis_points(N, colat[:npts], lon[:npts], kn[:npts], epochs(N)[:B])
            worst = max(worst, check_values(got, ref[:B, :npts], (N, npts, B)))
            for e in range(47):
                err = pr.max_error(got[e], short[e].astype(pr.LD))
                assert err < 1e-13, (N, npts, B, e, err)
                apart = max(apart, err)
    print('d/o {0}: GEMM path, worst epoch {1:.2e}; the two paths differ by at most {2:.2e}'.format(N, worst, apart))


@pytest.mark.parametrize('N', [180, 255, 256, 300])
@pytest.mark.parametrize('B', [3, 48])
def test_high_degree_and_poles(N, B):
    """d/o 180 .. 300 on 64 + 6 points, with the recursion kernel (3 epochs) and the GEMM path (48).  The recursion kernel stages
    256 (N + 1) bytes of coefficients in LDS: d/o 255 asks for exactly 64 KB, d/o 256 is the first request beyond it.  Every
    output is finite -- 1e-9 rad from the pole the sectorials underflow from order 35 on -- and epochs 0 and B - 1 match."""
    colat, lon, kn = tables(N, 70)
    ref = reference_values(N, 70, (0, 2, 47))
    got = synthesis_points(N, colat, lon, kn, epochs(N)[:B])
    assert got.shape == (B, 70) and np.all(np.isfinite(got))
    print('d/o {0}, {1} epochs: worst epoch {2:.2e}'.format(N, B, check_values(got[[0, B - 1]], ref[[0, 1 if B == 3 else 2]], (N, B))))


def test_degree_beyond_the_lds_of_a_compute_unit():
    """d/o 640 would need 164096 bytes of LDS for the recursion kernel, more than the 160 KB of a CDNA4 compute unit: the call
    has to take the GEMM path for its 2 epochs and return values, not a launch error.  One epoch is checked (the long-double
    pass at this degree takes seconds)."""
    N = 640
    colat, lon, kn = tables(N, 24)
    anm = epochs(N, 2)
    got = synthesis_points(N, colat, lon, kn, anm)
    assert got.shape == (2, 24) and np.all(np.isfinite(got))
    err = pr.max_error(got[1], pr.synthesis(anm[1], colat, lon, kn))
    print('d/o 640: {0:.2e}'.format(err))
    assert err < TOL, err


# Chunk seams.  A pass of shg_synthesis_matrix and of the GEMM path of shg_synthesis_points holds point_chunk() points: 2 GB of
# Legendre table, 2^31 / 8 = 2^28 doubles, over Pfull = (N + 1)^2 table rows per point.  At d/o 255, Pfull = 65536 = 2^16 and a
# chunk is 2^28 / 2^16 = 4096 points.  2 * 4096 + 70 points are three chunks, the last one ragged against tiles of 32, 64 and 128.
# The list repeats 131 base points (prime: the period lines up with no tile), so every output has a long-double reference.
CHUNK_N, CHUNK_BASE, CHUNK_NPTS = 255, 131, 2 * 4096 + 70


def chunk_tables():
    colat, lon, kn = tables(CHUNK_N, CHUNK_BASE)
    idx = np.arange(CHUNK_NPTS) % CHUNK_BASE
    return idx, colat[idx], lon[idx], kn[idx]


@functools.lru_cache(maxsize=None)
def chunk_rows():
    """harmonic rows of the 131 base points from degree 0, shared by the two chunk cases (read only)"""
    return pr.harmonic_rows(CHUNK_N, 0, *tables(CHUNK_N, CHUNK_BASE))


def test_chunk_seams_of_the_synthesis_matrix():
    assert (CHUNK_N + 1) ** 2 == 65536 and 2 ** 28 // 65536 == 4096 and CHUNK_NPTS == 8262
    idx, colat, lon, kn = chunk_tables()
    nmin = 255
    A = synthesis_matrix(CHUNK_N, nmin, colat, lon, kn)                         # 8262 x 511
    assert A.shape == (CHUNK_NPTS, 511) and np.all(np.isfinite(A))
    ref = chunk_rows()[:, nmin * nmin:]
    rows = pr.row_errors(A, ref[idx])
    print('d/o 255, degree 255 of 8262 points: worst row {0:.2e} (base point {1})'.format(rows.max(), int(idx[rows.argmax()])))
    assert rows.max() < ROW_TOL, (rows.max(), int(rows.argmax()), int(idx[rows.argmax()]))
    # the three chunks generate the same rows for the same point
    for p in range(CHUNK_BASE):
        same = A[p::CHUNK_BASE]
        assert np.array_equal(same, np.broadcast_to(same[0], same.shape)), p


def test_chunk_seams_of_the_gemm_path():
    idx, colat, lon, kn = chunk_tables()
    B = 48
    anm = epochs(CHUNK_N)[:B]
    got = synthesis_points(CHUNK_N, colat, lon, kn, anm)                        # X is 25 MB, the product 26 GFLOP
    assert got.shape == (B, CHUNK_NPTS) and np.all(np.isfinite(got))
    ref = (chunk_rows() @ orc.ravel_coefficients(anm, 0, CHUNK_N).astype(pr.LD).T).T
    print('d/o 255, 48 epochs on 8262 points: worst epoch {0:.2e}'.format(check_values(got, ref[:, idx], 'chunks')))


def test_synthesis_matrix_from_degree_zero_and_column_offset():
    """nmin = 0 at d/o 45 on 130 points against the reference, every row; the columns from nmin^2 on equal the nmin = 7 matrix
    bit for bit (p0 = nmin^2 is a plain offset into the generated table)."""
    N = 45
    colat, lon, kn = tables(N, 130)
    A = synthesis_matrix(N, 0, colat, lon, kn)
    assert A.shape == (130, 46 * 46) and np.all(np.isfinite(A))
    rows = pr.row_errors(A, pr.harmonic_rows(N, 0, colat, lon, kn))
    print('d/o 45 matrix: worst row {0:.2e} (point {1})'.format(rows.max(), int(rows.argmax())))
    assert rows.max() < ROW_TOL, (rows.max(), int(rows.argmax()))
    A7 = synthesis_matrix(N, 7, colat, lon, kn)
    assert A7.shape == (130, 46 * 46 - 49) and np.array_equal(A7, A[:, 49:])
    for npts in (1, 63, 65):                                                    # ragged tiles of 32
        assert np.array_equal(synthesis_matrix(N, 7, colat[:npts], lon[:npts], kn[:npts]), A7[:npts])


@functools.lru_cache(maxsize=None)
def covariance_case(N, nmin, general):
    P = (N + 1) ** 2 - nmin ** 2
    S = inputs.spd_covariance(40 + N, P) if P else np.zeros((0, 0))
    cov = pr.general_covariance(S) if general else S
    colat, lon, kn = tables(N, 130)
    return cov, pr.sigma(cov, nmin, N, colat, lon, kn)


@pytest.mark.parametrize('N', [20, 33])
@pytest.mark.parametrize('nmin', [0, 2, 'N+1'])
def test_covariance_propagation_at_points(N, nmin):
    """sqrt(a^T Sigma a) on 1 | 65 | 130 points (poles and near-polar points first), for a symmetric positive definite Sigma and
    for a general one -- the ABI promises a^T Sigma a for any matrix, the reference multiplies with the full matrix -- and
    nmin = N + 1, an empty band: zeros."""
    nmin = N + 1 if nmin == 'N+1' else nmin
    colat, lon, kn = tables(N, 130)
    for general in (False, True):
        cov, ref = covariance_case(N, nmin, general)
        if general and cov.size:
            assert not np.array_equal(cov, cov.T)
        for npts in (1, 65, 130):
            got = covprop_points(N, nmin, colat[:npts], lon[:npts], kn[:npts], cov)
            assert got.shape == (npts,) and np.all(np.isfinite(got))
            if cov.size == 0:
                assert not got.any()
            else:
                err = pr.max_error(got, ref[:npts])
                print('d/o {0} from degree {1}, {2} points, general {3}: sigma {4:.2e}'.format(N, nmin, npts, general, err))
                assert err < pr.TOL_SIGMA, (N, nmin, general, npts, err)


@pytest.mark.parametrize('nmin', [0, 2, 120])
def test_order_blocks_of_a_point_list(nmin):
    """shg_synthesis_matrix_order, pointwise, d/o 180, orders 0 | 1 | 90 | 180 on the 70 points: per row against the reference's
    block and against the matching columns of shg_synthesis_matrix, both to the bound of the header (this recursion takes
    s = sqrt(1 - t^2), not sin: another rounding near the poles, which order_block_bound carries; where that leaves no digit the
    block is exactly 0).  Order 0 passes out_sin = NULL."""
    N = 180
    colat, lon, kn = tables(N, 70)
    A = synthesis_matrix(N, nmin, colat, lon, kn)
    rows = pr.row_errors(A, pr.harmonic_rows(N, nmin, colat, lon, kn))
    print('d/o 180 matrix from degree {0}: worst row {1:.2e} (point {2})'.format(nmin, rows.max(), int(rows.argmax())))
    assert np.all(np.isfinite(A)) and rows.max() < ROW_TOL, (rows.max(), int(rows.argmax()))
    for m in (0, 1, 90, 180):
        got_c, got_s = matrix_order(N, m, nmin, colat, lon, kn)
        ref_c, ref_s = pr.order_block(N, m, nmin, colat, lon, kn)
        assert got_c.shape == ref_c.shape and np.all(np.isfinite(got_c)) and (m == 0 or np.all(np.isfinite(got_s)))
        bound = pb.order_block_bound(BLOCK_TOL, m, colat)
        zero = pb.zero_rows(m, colat)
        assert np.array_equal(zero, pb.lost_rows(m, colat)) and zero.sum() == (0, 3, 3, 5)[(0, 1, 90, 180).index(m)]
        assert not got_c[zero].any() and (m == 0 or not got_s[zero].any()), m
        ec, es = pb.block_row_errors(got_c, got_s, ref_c, ref_s)
        print('   order {0}: block rows at most {1:.3f} of their bound; special points {2}'.format(
            m, max(float(np.max(e / bound)) for e in (ec, es) if e is not None), ' '.join('{0:.1e}'.format(v) for v in ec[:6])))
        assert np.all(ec < bound), (m, int(np.argmax(ec / bound)), float(np.max(ec / bound)))
        assert m == 0 or np.all(es < bound), (m, int(np.argmax(es / bound)), float(np.max(es / bound)))
        # the same entries as columns of the dense operator (the column recursion with sin): same scale, same bound
        cc, cs = pr.order_columns(N, m, nmin)
        scale = np.max(np.abs(ref_c), axis=1) if m == 0 else np.maximum(np.max(np.abs(ref_c), axis=1), np.max(np.abs(ref_s), axis=1))
        dc = pr.row_errors(got_c, A[:, cc].astype(pr.LD), scale)
        assert np.all(dc < bound), (m, int(np.argmax(dc / bound)), float(np.max(dc / bound)))
        if m:
            ds = pr.row_errors(got_s, A[:, cs].astype(pr.LD), scale)
            assert np.all(ds < bound), (m, int(np.argmax(ds / bound)), float(np.max(ds / bound)))
