"""
Arc-wise parameters on the GPU: the kernel of shg_segment_products (engine.segment_products) against exact sums, bitwise wherever a
segment lies, and the reduced normal equations of lstsq.ArcParameters for the three kinds of observation against NumPy formulations of
the elimination (tests/golden/arc_inputs.py) on host copies of the device's design matrices, ranks, closed loop and combination
included.
"""
import functools

import numpy as np
import pytest

import acceleration_inputs as ai
import arc_inputs as arc
import design_inputs as di
import gradient_design_inputs as gdi
import grates_amd as ga
import los_inputs as li
import whitening_inputs as wi

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHORT_ARCS = [0, 1, 4, 300]
ARCS = [0, 150, 300]
TWO_ARCS = [0, 140]


def _host(t):
    return ga.engine.to_host(t)


def _int32(values):
    import torch
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=ga.engine.device())


def _padded(values, pad, fill):
    """device tensor with `pad` more columns than `values` [..., M], filled with `fill`; returns it and the view of the values"""
    import torch
    full = torch.full(values.shape[:-1] + (values.shape[-1] + pad,), fill, dtype=torch.float64, device=ga.engine.device())
    full[..., :values.shape[-1]] = ga.engine.to_device(values)
    return full, full[..., :values.shape[-1]]


# ---- 1: the kernel against exact sums ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seg', [[0, 1, 4, 300, 700], [3, 3, 70, 650]])
@pytest.mark.parametrize('u', [1, 4, 16])
def test_kernel_against_exact_sums(u, seg):
    """entry-wise within (len + 1) u sum |x_t b_t|: a chain and the tree round at most len times between them, and the exact
    reference once.  The padding of the rows and every column outside the segments is NaN: a read of it would poison a sum."""
    rows, channels, M = 6, 3, 700
    rng = np.random.default_rng(2820 + u)
    X, Bt = rng.standard_normal((rows, M)), rng.standard_normal((u, channels, M))
    reference, magnitude, lengths = arc.exact_segment_products(X, Bt, seg, channels)
    covered = np.zeros(M, dtype=bool)
    for first, last in zip(seg[:-1], seg[1:]):
        covered[first:last] = True
    X_nan, Bt_nan = np.where(covered, X, np.nan), np.where(covered, Bt, np.nan)
    Xv, Btv = _padded(X_nan, 4, float('nan'))[1], _padded(Bt_nan, 4, float('nan'))[1]
    S = ga.engine.segment_products(Xv, Btv, _int32(seg), channels=channels)
    assert tuple(S.shape) == (rows, len(seg) - 1, u) and S.is_contiguous()
    got = _host(S)
    assert np.all(np.isfinite(got))
    bound = (lengths[None, :, None] + 1) * U * magnitude
    ratio = np.abs(got - reference) / np.where(bound > 0, bound, 1.0)
    print('u {0}, seg {1}: {2:.3f} of the bound'.format(u, seg, ratio.max()))
    assert np.all(np.abs(got - reference) <= bound)
    assert np.all(got[:, lengths == 0] == 0.0)                                                     # an empty segment gives 0
    import torch
    out = torch.full((rows, len(seg) - 1, u), -7.25, dtype=torch.float64, device=S.device)
    assert ga.engine.segment_products(ga.engine.to_device(X_nan), ga.engine.to_device(Bt_nan), _int32(seg), channels=channels, out=out) is out
    assert np.array_equal(_host(out), got)                                                         # dense operands, a given output: bitwise
    if u == 1 and channels == 3:
        single = ga.engine.segment_products(ga.engine.to_device(X_nan[:1]), ga.engine.to_device(Bt_nan[:, 0]), _int32(seg))
        assert np.array_equal(_host(single), got[:1])                                              # Bt [u, M], channels = 1


# ---- 2: locality, bitwise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('length', [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_a_segment_gives_the_same_bits_wherever_it_lies(length):
    """the kernel's chains have stride 64 (its only chunk size: 63, 64, 65 and their multiples are the seams).  The data of one segment
    at offsets 0, 1, 63 and 517 of a longer row, alone and between other segments, in a matrix of 1 and of 7 rows (a full group of four
    rows and a short one), for u = 4 (four rows per wave) and u = 9 (two)"""
    rng = np.random.default_rng(2840 + length)
    for u in (4, 9):
        x, b = rng.standard_normal(length), rng.standard_normal((u, length))
        reference = _host(ga.engine.segment_products(ga.engine.to_device(x[None]), ga.engine.to_device(b), _int32([0, length])))
        assert reference.shape == (1, 1, u)
        for offset in (0, 1, 63, 517):
            M = offset + length + 130
            row, basis = rng.standard_normal(M), rng.standard_normal((u, M))
            row[offset:offset + length], basis[:, offset:offset + length] = x, b
            X7 = rng.standard_normal((7, M))
            X7[3], X7[6] = row, row
            one, seven, Bd = ga.engine.to_device(row[None]), ga.engine.to_device(X7), ga.engine.to_device(basis)
            alone, between = _int32([offset, offset + length]), _int32([0, offset, offset + length, M - 7, M])
            assert np.array_equal(_host(ga.engine.segment_products(one, Bd, alone)), reference)
            assert np.array_equal(_host(ga.engine.segment_products(one, Bd, between))[:, 1:2], reference)
            many = _host(ga.engine.segment_products(seven, Bd, between))
            assert np.array_equal(many[3:4, 1:2], reference) and np.array_equal(many[6:7, 1:2], reference)
            assert np.array_equal(_host(ga.engine.segment_products(seven, Bd, alone))[[3, 6]], np.concatenate((reference, reference)))


# ---- 3: clamping -----------------------------------------------------------------------------------------------------------------------
def test_segment_table_is_clamped():
    """a wrong table gives wrong numbers, not a fault: entries are clamped to 0 .. M and made non-decreasing.  With four columns of
    padding even an unclamped read would stay inside the allocation, and at 1e300 it would show"""
    rows, channels, M, u = 6, 3, 700, 4
    rng = np.random.default_rng(2860)
    X, Bt = rng.standard_normal((rows, M)), rng.standard_normal((u, channels, M))
    Xv, Btv = _padded(X, 4, 1e300)[1], _padded(Bt, 4, 1e300)[1]
    wrong = [-2, 5, 3, M + 3]
    assert arc.clamped(wrong, M).tolist() == [0, 5, 5, M]
    got = ga.engine.segment_products(Xv, Btv, _int32(wrong), channels=channels)
    expected = ga.engine.segment_products(Xv, Btv, _int32(arc.clamped(wrong, M)), channels=channels)
    assert bool((got == expected).all()) and bool(got.isfinite().all()) and bool((got[:, 1] == 0).all())
    reference, magnitude, lengths = arc.exact_segment_products(X, Bt, arc.clamped(wrong, M), channels)
    assert np.all(np.abs(_host(got) - reference) <= (lengths[None, :, None] + 1) * U * magnitude)
    extreme = ga.engine.segment_products(Xv, Btv, _int32([2 ** 31 - 1, -2 ** 31, 5, 2]), channels=channels)
    assert bool((extreme == 0).all())                                                              # everything lies behind the first entry


# ---- the reference of a reduced system -------------------------------------------------------------------------------------------------
def _device_tables(model, arcs, M):
    import torch
    taps = ga.lstsq.whitening_taps(model)
    return ga.engine.to_device(taps), torch.from_numpy(ga.lstsq.arc_stages(arcs, M, taps.shape[1] - 1)).to(ga.engine.device()), taps.shape[0]


def _transformed(At, l, basis, root, model, arcs):
    """host copies of what the device holds: the whitened At^T [K M, P], observations [K M] and basis [K, M, u].  At [P, K, M] is the
    device's design matrix times sqrt(w), l [M, K] the observations times sqrt(w), basis [M, u'] or [M, K, u], root [M, K] or None"""
    P, K, M = (int(size) for size in At.shape)
    Bt = arc.transformed_basis(basis, root, K).transpose(2, 0, 1)                                  # [u, K, M]
    lt = np.ascontiguousarray(l.T)
    if model is not None:
        taps, stage, channels = _device_tables(model, arcs, M)
        At = ga.engine.whiten_rows(At, taps, stage, channels=channels)
        Bt = _host(ga.engine.whiten_rows(ga.engine.to_device(Bt), taps, stage, channels=channels))
        lt = _host(ga.engine.whiten_rows(ga.engine.to_device(lt), taps, stage, channels=channels))
    return _host(At).reshape(P, K * M).T.copy(), lt.ravel(), np.ascontiguousarray(Bt.transpose(1, 2, 0))


def _reference(At, l, basis, root, model, arcs):
    """(A, l, units, normals of the projection, their bounds) of a reduced system"""
    A, lbar, B = _transformed(At, l, basis, root, model, arcs)
    units = arc.explicit_columns(B, arc.bounds_of(arcs, B.shape[1]), np.ndim(basis) == 2)
    return A, lbar, units, arc.projection(A, lbar, units), arc.normals_bounds(A, lbar)


def _check(ne, reference, label, count):
    """the device's reduced normals against the projection, entry-wise within 2 L u sqrt(N_ii N_jj), 2 L u sqrt(N_ii l^T l) and
    2 L u l^T l of dot products of length L = K M with the diagonals of the unreduced normals"""
    A, lbar, units, (N, n, lPl), (bound_N, bound_n, bound_l) = reference
    cond = arc.conditions(units).max()
    got_N, got_n, got_l, got_count = ne.to_array()
    assert got_N.shape == N.shape and got_n.shape == (N.shape[0], 1) and got_count == count
    print('{0}: cond(G) {1:.1f}; N {2:.4f}, n {3:.4f}, lPl {4:.4f} of their bounds'.format(
        label, cond, (np.abs(got_N - N) / bound_N).max(), (np.abs(got_n[:, 0] - n) / bound_n).max(), abs(got_l - lPl) / bound_l))
    assert cond <= 100
    assert np.all(np.abs(got_N - N) <= bound_N)
    assert np.all(np.abs(got_n[:, 0] - n) <= bound_n)
    assert abs(got_l - lPl) <= bound_l
    matrix = ne.matrix.device_block(0, 0)
    assert bool((matrix == matrix.t()).all())
    assert np.abs(A.T @ A - N).max() > 1e3 * bound_N.max()                                         # and the elimination does change the normals
    return ne


def _same(first, second):
    return (bool((first.matrix.device_block(0, 0) == second.matrix.device_block(0, 0)).all()) and bool((first.right_hand_side == second.right_hand_side).all())
            and first.observation_square_sum == second.observation_square_sum and first.observation_count == second.observation_count
            and np.array_equal(first.arc_elimination.ranks, second.arc_elimination.ranks))


# ---- 4: reduced normals of accelerations ---------------------------------------------------------------------------------------------------
NA, MA = 12, 700


@functools.lru_cache(maxsize=None)
def _acceleration_inputs():
    """the 700-point d/o-12 case of tests/test_gpu_whitening.py: positions, point weights with zeros, observations, the AR(5) model,
    the basis of a bias, a drift and one period of 93 samples per axis (u' = 4) on the arcs [0, 150, 300], and the device's design matrix"""
    model = wi.sequence(wi.fixture(), 'ar5', ga.lstsq)
    xyz = np.vstack((di.positions(), ai.scattered_positions(MA - 20, 2721)))
    rng = np.random.default_rng(2722)
    w = rng.uniform(0.25, 4.0, MA)
    w[rng.choice(MA, 20, replace=False)] = 0.0
    w[[0, 3, 4, 299, 300]] = 0.0
    obs = rng.standard_normal((MA, 3)) * 1e-3
    basis = ga.lstsq.arc_basis(ARCS, MA, degree=1, periods=(93,))
    At = ga.engine.acceleration_design(NA, xyz, di.GM, di.R, 0, weights=w)                          # [P, 3, M], times sqrt(w)
    return xyz, w, obs, model, basis, At


@functools.lru_cache(maxsize=None)
def _acceleration_reference(noise):
    xyz, w, obs, model, basis, At = _acceleration_inputs()
    root = np.sqrt(w)[:, None]
    return _reference(At, root * obs, basis, root, model if noise else None, ARCS)


def _build_accelerations(block_points, noise, **kwargs):
    xyz, w, obs, model, basis, _ = _acceleration_inputs()
    params = ga.lstsq.ArcParameters(basis, ARCS, model if noise else None, **kwargs)
    return params.from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w, block_points=block_points)


@pytest.mark.parametrize('noise', [True, False])
@pytest.mark.parametrize('block_points', [256, 100, None])
def test_reduced_normals_of_accelerations(block_points, noise):
    """blocks of 256 and of 100 cut the arcs [0, 150, 300] of 700 points, the default block holds them all"""
    xyz, w, obs, model, basis, _ = _acceleration_inputs()
    count = 3 * MA - 36
    ne = _check(_build_accelerations(block_points, noise), _acceleration_reference(noise), 'blocks of {0}, noise {1}'.format(block_points, noise), count)
    assert ne.status == 'normal_matrix' and ne.right_hand_side.is_cuda
    elimination = ne.arc_elimination
    assert isinstance(elimination, ga.lstsq.ArcElimination) and elimination.count == 36 and ne.observation_count == 3 * MA - elimination.count
    assert elimination.ranks.shape == (3, 3) and np.array_equal(elimination.ranks, np.full((3, 3), 4))
    assert _same(_build_accelerations(block_points, noise), ne)                                    # two runs are bitwise equal
    assert _same(_build_accelerations(block_points, noise, keep=False), ne)
    internal = ga.lstsq.NormalEquations._normals(
        ga.lstsq._observations('accelerations', dict(xyz=xyz, g=obs, weights=w), ga.engine.Band(0, NA, di.GM, di.R)),
        ga.lstsq._StochasticModel(model if noise else None, ARCS, ga.lstsq.ArcParameters(basis)), block_points)
    assert _same(internal, ne)                                                                     # the bound form is the internal path
    plain = ga.lstsq.NormalEquations.from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w, block_points=block_points,
                                                        noise_model=model if noise else None, arcs=ARCS if noise else None)
    assert plain.arc_elimination is None and plain.observation_count == 3 * MA
    difference = _host(plain.matrix.device_block(0, 0)) - _host(ne.matrix.device_block(0, 0))
    assert np.abs(difference).max() > 1e3 * _acceleration_reference(noise)[4][0].max()             # far more than the bound
    assert plain.observation_square_sum > ne.observation_square_sum


# ---- 5: gradients, line of sight, the general form -----------------------------------------------------------------------------------------
NG, MG = 8, 300
GOCE = ('xx', 'yy', 'zz', 'xz')


def test_reduced_normals_of_gradients(golden):
    """K = 4 components with a model each, a bias and a drift per component (the shared form, u' = 2); blocks of 128 cut both arcs"""
    models = [wi.sequence(golden('g27_whitening'), 'ar5', ga.lstsq), wi.synthetic_sequence(ga.lstsq, 5, 2731), wi.synthetic_sequence(ga.lstsq, 5, 2732),
              wi.synthetic_sequence(ga.lstsq, 5, 2733)]
    xyz, frames = ai.scattered_positions(MG, 2734), gdi.frames(MG, 2735)
    rng = np.random.default_rng(2736)
    w = rng.uniform(0.25, 4.0, (MG, 4))
    w[rng.choice(MG, 10, replace=False), rng.integers(0, 4, 10)] = 0.0
    obs = rng.standard_normal((MG, 4)) * 1e-9
    basis = ga.lstsq.arc_basis(TWO_ARCS, MG, degree=1)
    At = ga.engine.gradient_design(NG, xyz, gdi.GM, gdi.R, 0, frames=frames, components=GOCE, weights=w)            # [P, 4, M]
    reference = _reference(At, np.sqrt(w) * obs, basis, np.sqrt(w), models, TWO_ARCS)

    def build():
        return ga.lstsq.ArcParameters(basis, TWO_ARCS, models).from_gradients(xyz, obs, 0, NG, gdi.GM, gdi.R, frames=frames, components=GOCE, weights=w,
                                                                              block_points=128)
    ne = _check(build(), reference, 'gradients', 4 * MG - 16)
    assert np.array_equal(ne.arc_elimination.ranks, np.full((2, 4), 2)) and _same(build(), ne)


def test_reduced_normals_of_the_line_of_sight(golden):
    """K = 1: a bias, a drift and one period of 93 samples of the link per arc"""
    model = wi.sequence(golden('g27_whitening'), 'ar5', ga.lstsq)
    a, b = (x[:MG] for x in li.loop_pairs())
    rng = np.random.default_rng(2741)
    w = rng.uniform(0.25, 4.0, MG)
    w[rng.choice(MG, 10, replace=False)] = 0.0
    obs = rng.standard_normal(MG) * 1e-6
    basis = ga.lstsq.arc_basis(TWO_ARCS, MG, degree=1, periods=(93,))
    At = ga.engine.los_design(NG, a, b, li.GM, li.R, 0, weights=w)                                                   # [P, M]
    root = np.sqrt(w)[:, None]
    reference = _reference(At[:, None, :], root * obs[:, None], basis, root, model, TWO_ARCS)

    def build():
        return ga.lstsq.ArcParameters(basis, TWO_ARCS, model).from_line_of_sight(a, b, obs, 0, NG, li.GM, li.R, weights=w, block_points=128)
    ne = _check(build(), reference, 'line of sight', MG - 8)
    assert np.array_equal(ne.arc_elimination.ranks, np.full((2, 1), 4)) and _same(build(), ne)


def test_reduced_normals_of_accelerations_in_the_instrument_frame():
    """the general form: a bias and a drift per instrument axis, seen in Earth-fixed axes through the frames (u = 6, one set per arc,
    summed over the three channels); weights per component"""
    xyz, frames = ai.scattered_positions(MG, 2751), gdi.frames(MG, 2752)
    rng = np.random.default_rng(2753)
    w = rng.uniform(0.25, 4.0, (MG, 3))
    w[rng.choice(MG, 10, replace=False), rng.integers(0, 3, 10)] = 0.0
    obs = rng.standard_normal((MG, 3)) * 1e-3
    basis = ga.lstsq.frame_basis(ga.lstsq.arc_basis(TWO_ARCS, MG, degree=1), frames)
    assert basis.shape == (MG, 3, 6)
    At = ga.engine.acceleration_design(NG, xyz, di.GM, di.R, 0, weights=w)
    reference = _reference(At, np.sqrt(w) * obs, basis, np.sqrt(w), None, TWO_ARCS)

    def build():
        return ga.lstsq.ArcParameters(basis, TWO_ARCS).from_accelerations(xyz, obs, 0, NG, di.GM, di.R, weights=w, block_points=128)
    ne = _check(build(), reference, 'instrument frame', 3 * MG - 12)
    assert ne.arc_elimination.ranks.shape == (2,) and np.array_equal(ne.arc_elimination.ranks, [6, 6]) and _same(build(), ne)
    x = np.linalg.solve(*ne.to_array()[:2])
    assert ne.arc_elimination.parameters(x).shape == (2, 6)


# ---- 6: ranks ----------------------------------------------------------------------------------------------------------------------------
def _solution_deviation(A, lbar, units):
    """(x of lstsq of the explicit system, relative deviation of the host's Schur formulation from it)"""
    x = arc.explicit_solution(A, lbar, units)[0]
    N, n = arc.schur(A, lbar, units)[:2]
    return x, np.linalg.norm(np.linalg.solve(N, n) - x) / np.linalg.norm(x)


def test_ranks_of_short_and_empty_arcs():
    """arcs [0, 1, 4, 300] under four parameters per axis: one point determines one direction, an arc of zero weights none.  The
    solution against lstsq of the explicit system, within 100 times the deviation of the host's own Schur formulation"""
    xyz, w, obs, model, _, _ = _acceleration_inputs()
    w = w.copy()
    w[0], w[1:4] = 1.5, 0.0
    basis = ga.lstsq.arc_basis(SHORT_ARCS, MA, degree=1, periods=(93,))
    ne = ga.lstsq.ArcParameters(basis, SHORT_ARCS, model).from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w, block_points=256)
    ranks = ne.arc_elimination.ranks
    assert np.array_equal(ranks, np.repeat([[1], [0], [4], [4]], 3, axis=1)) and ne.arc_elimination.count == 27 and ne.observation_count == 3 * MA - 27
    root = np.sqrt(w)[:, None]
    At = ga.engine.acceleration_design(NA, xyz, di.GM, di.R, 0, weights=w)
    A, lbar, B = _transformed(At, root * obs, basis, root, model, SHORT_ARCS)
    units = arc.explicit_columns(B, arc.bounds_of(SHORT_ARCS, MA), True)
    assert np.array_equal(arc.schur(A, lbar, units)[4].reshape(4, 3), ranks)
    expected, deviation = _solution_deviation(A, lbar, units)
    x = _host(ne.solve())[:, 0]
    rel = np.linalg.norm(x - expected) / np.linalg.norm(expected)
    print('ranks {0}: x against lstsq {1:.2e}, host Schur {2:.2e}'.format(ranks[:, 0].tolist(), rel, deviation))
    assert deviation > 0 and rel <= 100 * deviation
    y = ne.arc_elimination.parameters(x)
    assert y.shape == (4, 3, 4) and np.all(y[1] == 0.0) and np.all(np.isfinite(y))


# ---- 7: closed loop ----------------------------------------------------------------------------------------------------------------------
def test_closed_loop_recovers_the_field_and_the_biases(golden):
    """the noise-free loop of tests/test_gpu_design.py with a known bias and drift per axis and arc added to the accelerations: the
    field and the parameters come back within 10 times the error of numpy.linalg.lstsq of the explicit system on the device's design
    matrix"""
    data = golden('g24_acceleration_design')
    assert float(data['loop_cond']) <= 1e4 and float(data['host_rel_err']) <= 1e-8
    N, min_degree, arcs = di.LOOP['N'], di.LOOP['min_degree'], [0, 250]
    positions = di.loop_positions()
    M = positions.shape[0]
    xyz = ga.engine.to_device(positions)
    gf = ga.gravityfield.PotentialCoefficients(di.GM, di.R)
    gf.anm = di.loop_field()
    g = _host(gf.gravitational_acceleration(xyz, as_tensor=True))
    basis = ga.lstsq.arc_basis(arcs, M, degree=1)
    rng = np.random.default_rng(2871)
    y_true = rng.standard_normal((2, 3, 2)) * np.sqrt(np.mean(g * g))                              # bias and drift of the size of the signal
    index = np.searchsorted(arcs, np.arange(M), side='right') - 1
    obs = g + np.einsum('tj,tkj->tk', basis, y_true[index])
    truth = ga.utilities.ravel_coefficients(gf.anm, min_degree, N)

    At = ga.engine.acceleration_design(N, positions, di.GM, di.R, min_degree)
    A, lbar, B = _transformed(At, obs, basis, None, None, arcs)
    x_host, y_host = arc.explicit_solution(A, lbar, arc.explicit_columns(B, arc.bounds_of(arcs, M), True))
    host_rel_err = np.linalg.norm(x_host - truth) / np.linalg.norm(truth)
    host_y_err = np.linalg.norm(y_host.reshape(2, 3, 2) - y_true) / np.linalg.norm(y_true)

    ne = ga.lstsq.ArcParameters(basis, arcs).from_accelerations(xyz, obs, min_degree, N, di.GM, di.R)
    assert ne.observation_count == 3 * M - 12 and np.array_equal(ne.arc_elimination.ranks, np.full((2, 3), 2))
    solution = _host(ne.solve())[:, 0]
    rel = np.linalg.norm(solution - truth) / np.linalg.norm(truth)
    y = ne.arc_elimination.parameters(solution)
    rel_y = np.linalg.norm(y - y_true) / np.linalg.norm(y_true)
    print('closed loop: field {0:.2e} (host {1:.2e}), parameters {2:.2e} (host {3:.2e})'.format(rel, host_rel_err, rel_y, host_y_err))
    assert 0 < host_rel_err <= 1e-8
    assert rel <= 10 * host_rel_err
    assert y.shape == (2, 3, 2) and rel_y <= 10 * host_rel_err
    biased = ga.lstsq.NormalEquations.from_accelerations(xyz, obs, min_degree, N, di.GM, di.R).solve()
    assert np.linalg.norm(_host(biased)[:, 0] - truth) > 1e6 * host_rel_err * np.linalg.norm(truth)      # without the elimination the bias goes into the field
    discarded = ga.lstsq.ArcParameters(basis, arcs, keep=False).from_accelerations(xyz, obs, min_degree, N, di.GM, di.R)
    assert _same(discarded, ga.lstsq.ArcParameters(basis, arcs).from_accelerations(xyz, obs, min_degree, N, di.GM, di.R))
    with pytest.raises(ValueError, match='keep=True'):
        discarded.arc_elimination.parameters(solution)


# ---- 8: combination ------------------------------------------------------------------------------------------------------------------------
def test_combination_of_reduced_systems(golden):
    """accumulate_normals of a reduced link system and a reduced orbit system against lstsq of the joint explicit system, within 100
    times the deviation of the host's own Schur formulation of the same case; the variance components see the reduced redundancies"""
    model = wi.sequence(golden('g27_whitening'), 'ar5', ga.lstsq)
    a, b = (x[:MG] for x in li.loop_pairs())
    rng = np.random.default_rng(2881)
    link_obs, orbit_obs = rng.standard_normal(MG) * 1e-6, rng.standard_normal((MG, 3)) * 1e-6
    link_basis, orbit_basis = ga.lstsq.arc_basis(TWO_ARCS, MG, degree=1, periods=(93,)), ga.lstsq.arc_basis(TWO_ARCS, MG, degree=1)
    link = ga.lstsq.ArcParameters(link_basis, TWO_ARCS, model).from_line_of_sight(a, b, link_obs, 2, NG, li.GM, li.R, block_points=128)
    orbit = ga.lstsq.ArcParameters(orbit_basis, TWO_ARCS).from_accelerations(a, orbit_obs, 2, NG, li.GM, li.R, block_points=128)
    assert link.observation_count == MG - 8 and orbit.observation_count == 3 * MG - 12
    systems = []
    for At, l, basis, noise in ((ga.engine.los_design(NG, a, b, li.GM, li.R, 2)[:, None, :], link_obs[:, None], link_basis, model),
                                (ga.engine.acceleration_design(NG, a, li.GM, li.R, 2), orbit_obs, orbit_basis, None)):
        A, lbar, B = _transformed(At, l, basis, None, noise, TWO_ARCS)
        systems.append((A, lbar, arc.explicit_columns(B, arc.bounds_of(TWO_ARCS, MG), True)))
    rows = [system[0].shape[0] for system in systems]
    A, lbar = np.vstack([system[0] for system in systems]), np.concatenate([system[1] for system in systems])
    units = [np.vstack((E, np.zeros((rows[1], E.shape[1])))) for E in systems[0][2]] + [np.vstack((np.zeros((rows[0], E.shape[1])), E)) for E in systems[1][2]]
    expected, deviation = _solution_deviation(A, lbar, units)

    factors = [1.0, 1.0]
    combined = ga.lstsq.accumulate_normals([link, orbit], factors)
    assert combined.observation_count == 4 * MG - 20
    x = combined.solve()
    solution = _host(x)[:, 0] if ga.lstsq._is_tensor(x) else x[:, 0]
    rel = np.linalg.norm(solution - expected) / np.linalg.norm(expected)
    print('combination: x against lstsq {0:.2e}, host Schur {1:.2e}'.format(rel, deviation))
    assert deviation > 0 and rel <= 100 * deviation
    estimates = ga.lstsq.compute_variance_factors([link, orbit], combined, x, factors)
    print('variance factors', estimates)
    assert estimates.shape == (2,) and np.all(np.isfinite(estimates))
