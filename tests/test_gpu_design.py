"""
The design matrix of the gravitational acceleration on the GPU (gravityfield.acceleration_design_matrix, engine.acceleration_design)
and the normal equations built from it (lstsq.NormalEquations.from_accelerations): against the reference's unit-field accelerations
(tests/golden/g24_acceleration_design.npz), against the host and GPU acceleration, for the kernels' contract (entries independent
of the batch, reproducible, min_degree a column slice, weights a row scaling) and through solve / posterior_sigma /
compute_covariance / accumulate_normals, closed loop included.
"""
import functools

import numpy as np
import pytest

import acceleration_inputs as ai
import design_inputs as di
import grates_amd as ga

pytestmark = pytest.mark.gpu

TOL = 5e-14          # of max|A| per case: the acceleration suite's bound (the fixture's restatement_err, 1.6e-15, is below a quarter of it)
TOL_AX = 1e-13       # of max|g|: design matrix times coefficients against the GPU acceleration (ax_err, 6.8e-16, is below a quarter)
U = 2.0 ** -53


def _host(t):
    return ga.engine.to_host(t)


def _design(xyz, min_degree, max_degree, **kwargs):
    return ga.gravityfield.acceleration_design_matrix(xyz, min_degree, max_degree, di.GM, di.R, **kwargs)


def _host_acceleration(xyz):
    def acceleration(anm):
        gf = ga.gravityfield.PotentialCoefficients(di.GM, di.R)
        gf.anm = anm
        return gf.gravitational_acceleration(xyz)
    return acceleration


def _check_tolerances(data):
    assert float(data['restatement_err']) <= TOL / 4 and float(data['ax_err']) <= TOL_AX / 4


# ---- 1: fixture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,min_degree', [(8, 0), (8, 2), (2, 0), (2, 2)])
def test_matches_reference(golden, N, min_degree):
    import torch
    data = golden('g24_acceleration_design')
    _check_tolerances(data)
    xyz = data['xyz']
    ref = data['A{0}'.format(N) + ('_min2' if min_degree else '')]
    A = _design(xyz, min_degree, N, as_tensor=True)
    assert isinstance(A, torch.Tensor) and A.is_cuda and A.dtype == torch.float64 and tuple(A.shape) == ref.shape
    At = ga.engine.acceleration_design(N, xyz, di.GM, di.R, min_degree)
    assert At.is_cuda and At.is_contiguous() and tuple(At.shape) == (ref.shape[1], 3, xyz.shape[0])
    assert bool((At.permute(2, 1, 0).reshape(A.shape) == A).all())
    host = _design(xyz, min_degree, N)
    assert isinstance(host, np.ndarray) and host.dtype == np.float64 and np.array_equal(host, _host(A))
    assert np.all(np.isfinite(host))
    err = np.abs(host - ref).max(axis=1).reshape(-1, 3).max(axis=1) / np.abs(ref).max()        # per point (poles: 0 .. 3, 1 mm: 12)
    print('d/o {0} from {1}: {2:.2e} of max|A| (worst point {3})'.format(N, min_degree, err.max(), err.argmax()))
    assert err.max() <= TOL, err


# ---- 2: degree edges ---------------------------------------------------------------------------------------------------------------
EDGE_POINTS = [0, 5, 12, 15]          # pole, equator, 1 mm off the pole, scattered


@pytest.mark.parametrize('N', [0, 1, 2])
@pytest.mark.parametrize('lowest', ['0', 'N'])
def test_degree_edges_against_unit_fields(N, lowest):
    min_degree = 0 if lowest == '0' else N
    xyz = di.positions()[EDGE_POINTS]
    ref = di.unit_field_matrix(_host_acceleration(xyz), xyz, min_degree, N)
    A = _design(xyz, min_degree, N)
    assert A.shape == ref.shape and np.all(np.isfinite(A))
    err = np.abs(A - ref).max() / np.abs(ref).max()
    print('d/o {0} from {1}: {2:.2e} of max|A|'.format(N, min_degree, err))
    assert err <= TOL


def test_degree_65_against_unit_fields():
    """d/o 65: every column of degree 65 (min_degree = N) against the host acceleration of its unit field.  From min_degree 0 the
    matrix has 4356 columns and a host call takes 20 ms, so there: the columns of degrees 0 .. 2, those of (64, 63), (64, 64) and a
    seeded sample of 40 more against their unit fields, the columns of degree 65 bitwise equal to the min_degree = N matrix, and all
    columns at once through A @ x against the host acceleration of a full field (an entry is within TOL max|A|, so the product is
    within TOL max|A| sum|x|)."""
    N = 65
    xyz = di.positions()[EDGE_POINTS]
    acceleration = _host_acceleration(xyz)
    top = _design(xyz, N, N)
    ref = di.unit_field_matrix(acceleration, xyz, N, N)
    scale = np.abs(ref).max()
    err = np.abs(top - ref).max() / scale
    print('d/o 65 from 65: {0:.2e} of max|A|'.format(err))
    assert top.shape == (12, 2 * N + 1) and err <= TOL
    A = _design(xyz, 0, N)
    assert A.shape == (12, (N + 1) ** 2) and np.all(np.isfinite(A))
    assert np.array_equal(A[:, N * N:], top)
    columns = di.degreewise(0, N)
    rng = np.random.default_rng(2451)
    sample = sorted(set(range(9)) | {64 * 64 + 125, 64 * 64 + 126, 64 * 64 + 127, 64 * 64 + 128} | set(rng.choice(N * N, 40, replace=False).tolist()))
    scale = max(scale, np.abs(A).max())
    for col in sample:
        n, m, sine = columns[col]
        err = np.abs(A[:, col] - acceleration(di.unit_field(n, m, sine, N)).ravel()).max() / scale
        assert err <= TOL, (n, m, sine, err)
    anm = rng.standard_normal((N + 1, N + 1))
    x = di.ravel(anm, 0, N)
    g = acceleration(anm).ravel()
    assert np.abs(A @ x - g).max() <= TOL * np.abs(A).max() * np.abs(x).sum()


# ---- 3: linearity at size ----------------------------------------------------------------------------------------------------------
def test_times_coefficients_is_the_gpu_acceleration_at_degree_96(golden):
    _check_tolerances(golden('g24_acceleration_design'))
    N, kind, seed, _ = ai.CASES['anomaly96']
    xyz = golden('g22_acceleration')['xyz_anomaly96']
    gf = ga.gravityfield.PotentialCoefficients(ai.GM, ai.R)
    gf.anm = ai.coefficients(N, kind, seed)
    g = _host(gf.gravitational_acceleration(xyz, as_tensor=True))
    A = _design(xyz, 0, N)
    assert A.shape == (3 * xyz.shape[0], 9409)
    err = np.abs(A @ ga.utilities.ravel_coefficients(gf.anm, 0, N) - g.ravel()).max() / np.abs(g).max()
    print('A @ x against the GPU acceleration, d/o 96: {0:.2e} of max|g|'.format(err))
    assert err <= TOL_AX
    A2 = _design(xyz, 2, N)                                                    # the field has nothing below degree 2
    err = np.abs(A2 @ ga.utilities.ravel_coefficients(gf.anm, 2, N) - g.ravel()).max() / np.abs(g).max()
    assert err <= TOL_AX


# ---- 4 .. 6: the kernels' contract ---------------------------------------------------------------------------------------------------
NC, MC = 12, 700


@functools.lru_cache(maxsize=None)
def _contract():
    """700 positions (the special ones first), their d/o-12 design matrix rows [M, 3, P] on the host, weights and accelerations"""
    xyz = np.vstack((ai.special_positions(), ai.scattered_positions(MC - 13, 2461)))
    rows = _design(xyz, 0, NC).reshape(MC, 3, -1)
    rng = np.random.default_rng(2462)
    w = rng.uniform(0.25, 4.0, (MC, 3))
    w[rng.choice(MC, 20, replace=False), rng.integers(0, 3, 20)] = 0.0
    w[5] = 0.0
    obs = rng.standard_normal((MC, 3)) * 1e-3
    return xyz, rows, w, obs


@pytest.mark.parametrize('M', [1, 255, 256, 257, 700])
def test_rows_do_not_depend_on_the_batch(M):
    xyz, rows, _, _ = _contract()
    assert np.array_equal(_design(xyz[:M], 0, NC).reshape(M, 3, -1), rows[:M])
    assert np.array_equal(_design(xyz[MC - M:], 0, NC).reshape(M, 3, -1), rows[MC - M:])           # other lanes, other workgroups
    assert np.array_equal(_design(xyz[:M][::-1].copy(), 0, NC).reshape(M, 3, -1), rows[:M][::-1])
    assert np.array_equal(_design(xyz[:M], 0, NC).reshape(M, 3, -1), rows[:M])                    # repeated call


def test_rows_do_not_depend_on_the_pass():
    """d/o 96 keeps the solid harmonics of 3328 points within the 256 MB of a pass: 3400 points take two passes (min_degree 96 keeps
    the matrix at 193 columns)"""
    N, M = 96, 3400
    assert (256 << 20) // 8 // (2 * (N + 2) * (N + 3) // 2) // 256 * 256 == 3328
    xyz = ai.scattered_positions(M, 2471)
    rows = _design(xyz, N, N).reshape(M, 3, -1)
    assert rows.shape == (M, 3, 2 * N + 1) and np.all(np.isfinite(rows))
    for first, last in ((0, 300), (3200, 3400), (3328, 3400), (3327, 3329)):
        assert np.array_equal(_design(xyz[first:last], N, N).reshape(last - first, 3, -1), rows[first:last]), (first, last)
    w = np.random.default_rng(2472).uniform(0.0, 2.0, (M, 3))
    assert np.array_equal(_design(xyz, N, N, weights=w).reshape(M, 3, -1), rows * np.sqrt(w)[:, :, np.newaxis])
    assert np.array_equal(_design(xyz, N, N, weights=w[:, 1].copy()).reshape(M, 3, -1), rows * np.sqrt(w[:, 1])[:, np.newaxis, np.newaxis])


def test_min_degree_is_a_column_slice():
    xyz, rows, _, _ = _contract()
    for min_degree in (2, 5, NC):
        A = _design(xyz, min_degree, NC)
        assert np.array_equal(A, rows.reshape(3 * MC, -1)[:, min_degree ** 2:]), min_degree


def test_weights_scale_the_rows():
    xyz, rows, w, _ = _contract()
    per_component = _design(xyz, 0, NC, weights=w).reshape(MC, 3, -1)
    assert np.array_equal(per_component, rows * np.sqrt(w)[:, :, np.newaxis])
    assert np.all(per_component[w == 0.0] == 0.0) and np.count_nonzero(w == 0.0) >= 20
    per_point = _design(xyz, 0, NC, weights=w[:, 0].copy()).reshape(MC, 3, -1)
    assert np.array_equal(per_point, rows * np.sqrt(w[:, 0])[:, np.newaxis, np.newaxis])
    on_device = _design(ga.engine.to_device(xyz), 0, NC, weights=ga.engine.to_device(w)).reshape(MC, 3, -1)
    assert np.array_equal(on_device, per_component)
    assert np.array_equal(_design(xyz, 0, NC, weights=np.ones(MC)).reshape(MC, 3, -1), rows)


# ---- 7 .. 10: normal equations -------------------------------------------------------------------------------------------------------
K = 3 * MC           # 2100 terms per dot product


@functools.lru_cache(maxsize=None)
def _normals_reference():
    """float64 NumPy normals from the host copy of the weighted d/o-12 design matrix, with the entry-wise bounds
    2 K 2^-53 sqrt(N_ii N_jj) (N), 2 K 2^-53 sqrt(N_ii l^T P l) (n) and 2 K 2^-53 l^T P l: the standard bound K u |a| |b| on a dot
    product of length K, once for each side of the comparison"""
    xyz, rows, w, obs = _contract()
    A = (rows * np.sqrt(w)[:, :, np.newaxis]).reshape(K, -1)
    l = (obs * np.sqrt(w)).reshape(K)
    N, n, lPl = A.T @ A, A.T @ l, float(l @ l)
    d = np.sqrt(np.diag(N))
    return N, n, lPl, 2 * K * U * np.outer(d, d), 2 * K * U * d * np.sqrt(lPl), 2 * K * U * lPl


def _build(block_points, first=0, last=MC):
    xyz, _, w, obs = _contract()
    return ga.lstsq.NormalEquations.from_accelerations(xyz[first:last], obs[first:last], 0, NC, di.GM, di.R, weights=w[first:last],
                                                       block_points=block_points)


def _check_against_reference(ne, label):
    N, n, lPl, bound_N, bound_n, bound_l = _normals_reference()
    got_N, got_n, got_l, count = ne.to_array()
    assert got_N.shape == N.shape and got_n.shape == (N.shape[0], 1)
    print('{0}: N {1:.2f}, n {2:.2f}, lPl {3:.2f} of their bounds'.format(label, (np.abs(got_N - N) / bound_N).max(),
                                                                          (np.abs(got_n[:, 0] - n) / bound_n).max(), abs(got_l - lPl) / bound_l))
    assert np.all(np.abs(got_N - N) <= bound_N)
    assert np.all(np.abs(got_n[:, 0] - n) <= bound_n)
    assert abs(got_l - lPl) <= bound_l
    return got_N, got_n, got_l, count


def test_normals_against_numpy():
    import torch
    ne = _build(256)                                                            # three blocks, the last of 188 points
    assert isinstance(ne, ga.lstsq.NormalEquations) and ne.status == 'normal_matrix'
    P = (NC + 1) ** 2
    assert ne.matrix.shape == (1, 1) and tuple(ne.matrix.device_block(0, 0).shape) == (P, P)
    assert isinstance(ne.right_hand_side, torch.Tensor) and ne.right_hand_side.is_cuda and tuple(ne.right_hand_side.shape) == (P, 1)
    assert isinstance(ne.observation_square_sum, float)
    assert ne.observation_count == 3 * MC                                       # zero weights still count
    _check_against_reference(ne, 'blocks of 256')


def test_normals_are_symmetric_and_reproducible():
    first, second = _build(256), _build(256)
    N = first.matrix.device_block(0, 0)
    assert bool((N == N.t()).all())
    assert bool((second.matrix.device_block(0, 0) == N).all())
    assert bool((second.right_hand_side == first.right_hand_side).all())
    assert second.observation_square_sum == first.observation_square_sum


def test_block_sizes_agree():
    _, _, _, bound_N, bound_n, bound_l = _normals_reference()
    base = _check_against_reference(_build(256), 'blocks of 256')
    for block_points in (512, None, 100):
        other = _check_against_reference(_build(block_points), 'blocks of {0}'.format(block_points))
        assert np.all(np.abs(other[0] - base[0]) <= bound_N)
        assert np.all(np.abs(other[1] - base[1])[:, 0] <= bound_n)
        assert abs(other[2] - base[2]) <= bound_l and other[3] == base[3]


def test_arcs_add_up():
    parts = [_build(256, 0, 350), _build(256, 350, MC)]
    combined = ga.lstsq.accumulate_normals(parts, [1.0, 1.0])
    assert combined.observation_count == 3 * MC
    _check_against_reference(combined, 'two arcs')
    single = _build(256).to_array()
    _, _, _, bound_N, bound_n, bound_l = _normals_reference()
    got = combined.to_array()
    upper = np.triu(np.ones_like(bound_N, dtype=bool))
    assert np.all(np.abs(got[0] - single[0])[upper] <= bound_N[upper])
    assert np.all(np.abs(got[1] - single[1])[:, 0] <= bound_n) and abs(got[2] - single[2]) <= bound_l


# ---- 11, 12: closed loop -------------------------------------------------------------------------------------------------------------
def test_closed_loop_recovers_the_field(golden):
    """field -> GPU accelerations at 600 points -> normals -> solve -> field.  The host solves the same loop through its normals to
    host_rel_err = 8.7e-16 (cond(A) = 3.2, recorded in the fixture); the GPU loop must stay within 10 times that."""
    data = golden('g24_acceleration_design')
    host_rel_err = float(data['host_rel_err'])
    assert float(data['loop_cond']) <= 1e4 and host_rel_err <= 1e-8
    N, min_degree = di.LOOP['N'], di.LOOP['min_degree']
    xyz = ga.engine.to_device(di.loop_positions())
    gf = ga.gravityfield.PotentialCoefficients(di.GM, di.R)
    gf.anm = di.loop_field()
    g = gf.gravitational_acceleration(xyz, as_tensor=True)
    ne = ga.lstsq.NormalEquations.from_accelerations(xyz, g, min_degree, N, di.GM, di.R)
    assert ne.observation_count == 1800
    x = ne.solve()
    truth = ga.utilities.ravel_coefficients(gf.anm, min_degree, N)
    solution = _host(x)[:, 0]
    rel = np.linalg.norm(solution - truth) / np.linalg.norm(truth)
    rms = float(np.sqrt(np.mean(_host(g) ** 2)))
    sigma = float(ne.posterior_sigma(x))
    print('closed loop: relative error {0:.2e} (host {1:.2e}), posterior sigma {2:.2e} of rms|g|'.format(rel, host_rel_err, sigma / rms))
    assert rel <= 10 * host_rel_err
    anm = ga.utilities.unravel_coefficients(solution, min_degree, N)
    assert anm.shape == gf.anm.shape and np.abs(anm - gf.anm).max() <= 10 * host_rel_err * np.linalg.norm(truth)
    assert sigma < 1e-10 * rms
    ne.compute_covariance(sparse=False)
    assert ne.status == 'covariance_matrix'
    diagonal = ne.matrix.diag()
    assert diagonal.shape == (77,) and np.all(diagonal > 0)
