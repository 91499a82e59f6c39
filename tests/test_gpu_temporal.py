"""
Time-variable parameters on the GPU: the window expansion kernel (engine.window_expand, shg_window_expand)
exactly, the statement of the model (gravityfield.temporal_design_matrix) against the reference values of the point functionals at
epochs, and the normal equations of lstsq.TemporalParameters against float64 NumPy normals of what the device holds, for their
bitwise contracts, their block pattern, through a closed loop and together with the process-dynamics constraint of the smoother.
"""
import datetime
import functools

import numpy as np
import pytest

import design_inputs as di
import points_at_inputs as pi
import temporal_inputs as ti
import whitening_inputs as wi

import grates_amd as ga

pytestmark = pytest.mark.gpu
ls = ga.lstsq

U = 2.0 ** -53
TOL_AT = 5e-14       # of the fixture's scale: the bound of tests/test_gpu_points_at.py for g32_points_at.npz
TOL_AX = 1e-13       # of max|g|: the bound of tests/test_gpu_design.py for design matrix times coefficients
TOL, TOL_INV = 1e-11, 1e-10                # solution and inverse of a chain: the criteria of tests/test_gpu_lstsq.py
SENTINEL = -7.25
TERMS = 3 * ti.M                           # terms of a dot product over all observations


def _host(t):
    return ga.engine.to_host(t)


# ---- 4: the kernel -----------------------------------------------------------------------------------------------------------------------
def _runs(rng, n, W, E):
    """run tables of n columns: a run of one column first and last where there is room, random cuts between, random slots"""
    cuts = {0, n}
    if n > 1:
        cuts |= {1, n - 1} | set(rng.integers(1, n, min(n // 40 + 1, 12)).tolist())
    begin = np.array(sorted(cuts))
    slot = rng.integers(0, E - W + 1, len(begin) - 1)
    if E > W and len(slot) > 1:
        slot[0], slot[-1] = E - W, 0
    return slot, begin


def _expected(T, factors, slot, begin, E):
    """(S [E, rows, n], inside [E, n]) in torch: factors * T inside the window, +0.0 outside"""
    import torch
    rows, n = T.shape
    W = factors.shape[1]
    column_slot = torch.from_numpy(np.repeat(slot, np.diff(begin))).to(T.device)
    S = torch.zeros((E, rows, n), dtype=torch.float64, device=T.device)
    inside = torch.zeros((E, n), dtype=torch.bool, device=T.device)
    columns = torch.arange(n, device=T.device)
    for j in range(W):
        S[column_slot + j, :, columns] = (factors[:, j] * T).t()
        inside[column_slot + j, columns] = True
    return S, inside


@pytest.mark.parametrize('W,E', [(1, 1), (2, 2), (2, 3), (5, 5), (16, 16), (1, 16)])
def test_window_expand(W, E):
    import torch
    rng = np.random.default_rng(3500 + 17 * W + E)
    for n in (1, 2, 255, 256, 257, 513):
        for rows in (1, 3, 231):
            slot, begin = _runs(rng, n, W, E)
            values = rng.standard_normal((rows, n + 4 + n % 2))                                 # an even row stride
            values[rng.integers(0, rows, 3), rng.integers(0, n + 4, 3)] = 1e308
            values[0, 2] = -1e308                                                          # column 0 of the even slice
            wide = ga.engine.to_device(values)
            factors = ga.engine.to_device(rng.uniform(-2.0, 2.0, (n, W)))
            for offset, pad, guard in ((2, 2 + n % 2, 4), (1, 1 + n % 2, 3)):              # 16-byte layout (even strides) and 8-byte layout
                T = wide[:, offset:offset + n]                                             # a column slice: ldt > n
                lds = n + pad
                slot_stride = rows * lds + (2 if guard == 4 else 1)
                buffer = torch.full((2 * guard + E * slot_stride,), SENTINEL, dtype=torch.float64, device=T.device)
                out = buffer.as_strided((E, rows, n), (slot_stride, lds, 1), guard)
                assert (out.data_ptr() % 16 == 0) == (guard == 4)
                got = ga.engine.window_expand(T, factors, slot, begin, E, out=out)
                assert got is out
                S, inside = _expected(T, factors, slot, begin, E)
                expected = torch.full_like(buffer, SENTINEL)
                expected.as_strided((E, rows, n), (slot_stride, lds, 1), guard).copy_(S)
                label = (W, E, n, rows, offset)
                assert bool((buffer == expected).all()), label                             # the values, the guards and the padding
                outside = ~inside[:, None, :].expand(E, rows, n)
                assert not bool(torch.signbit(out[outside]).any()) and bool((out[outside] == 0.0).all()), label
                first = buffer.clone()
                ga.engine.window_expand(T, factors, slot, begin, E, out=out)
                assert bool((buffer == first).all()) and not bool(torch.signbit(out[outside]).any()), label
            dense = ga.engine.window_expand(T.reshape(rows, 1, n), factors, slot, begin, E)                          # new tensor, T copied
            assert tuple(dense.shape) == (E, rows, 1, n) and dense.is_contiguous() and bool((dense.reshape(E, rows, n) == S).all())
    single = np.arange(257, dtype=np.int64)                                                # runs of one point throughout
    T = ga.engine.to_device(rng.standard_normal((3, 256)))
    factors = ga.engine.to_device(rng.uniform(-2.0, 2.0, (256, W)))
    slot = rng.integers(0, E - W + 1, 256)
    S, _ = _expected(T, factors, slot, single, E)
    assert bool((ga.engine.window_expand(T, factors, slot, single, E) == S).all())


def test_window_expand_refuses_before_the_launch():
    T, factors = ga.engine.to_device(np.ones((2, 4))), ga.engine.to_device(np.ones((4, 2)))
    with pytest.raises(ValueError, match='slot 2, outside'):
        ga.engine.window_expand(T, factors, [2], [0, 4], 3)
    with pytest.raises(ValueError, match='ascend strictly'):
        ga.engine.window_expand(T, factors, [0], [0, 3], 3)
    with pytest.raises(ValueError, match='factors must be'):
        ga.engine.window_expand(T, factors[:3], [0], [0, 4], 3)
    with pytest.raises(ValueError, match='out must be'):
        ga.engine.window_expand(T, factors, [0], [0, 4], 3, out=ga.engine.to_device(np.zeros((3, 2, 5))))


# ---- 5: the statement of the model -------------------------------------------------------------------------------------------------------
def test_temporal_design_matrix_against_the_reference(golden):
    import torch
    data = golden('g32_points_at')
    xyz, ref, scale = data['xyz_series60'], data['g_series60'], float(data['scale_series60'])
    N = pi.CASES['series60'][0]
    series = pi.constituents('series60')[0]
    epochs = [datetime.datetime.fromisoformat(str(s)) for s in data['iso_series60']]
    temporal = ls.TemporalParameters.linear(pi.series_epochs(), epochs)
    design = ga.gravityfield.acceleration_design_matrix(xyz, 0, N, pi.GM, pi.R)
    A = ga.gravityfield.temporal_design_matrix(design, temporal.first, temporal.factors, pi.SERIES_FIELDS)
    assert isinstance(A, np.ndarray) and A.shape == (3 * xyz.shape[0], pi.SERIES_FIELDS * (N + 1) ** 2)
    assert np.array_equal(A, ti.expand(design, temporal.first, temporal.factors, pi.SERIES_FIELDS))
    on_device = ga.gravityfield.temporal_design_matrix(ga.engine.to_device(design), temporal.first, temporal.factors, pi.SERIES_FIELDS, as_tensor=True)
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and np.array_equal(_host(on_device), A)
    x = np.concatenate([ga.utilities.ravel_coefficients(anm, 0, N) for anm in pi.series_coefficients('series60')])
    g = (A @ x).reshape(-1, 3)
    err = np.abs(g - ref).max() / scale
    at = series.gravitational_acceleration_at(xyz, epochs)
    err_at = np.abs(g - at).max() / np.abs(at).max()
    print('A_tv x: {0:.3e} of the scale against the reference, {1:.3e} of max|g| against gravitational_acceleration_at'.format(err, err_at))
    assert err <= TOL_AT and err_at <= TOL_AX


# ---- 6 .. 10, 13: normal equations ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _static():
    """positions, weights and observations of all cases, and the host copy of the device's weighted static design matrix [3 M, P]"""
    xyz, w, obs = ti.positions(), ti.weights(), ti.observations()
    design = ga.gravityfield.acceleration_design_matrix(xyz, ti.MIN_DEGREE, ti.N, ti.GM, ti.R, weights=w)
    return xyz, w, obs, design


def _bounds(N, n, lPl, terms=TERMS):
    """the entry-wise bounds of tests/test_gpu_design.py: 2 K u sqrt(N_ii N_jj), 2 K u sqrt(N_ii l^T P l), 2 K u l^T P l"""
    d = np.sqrt(np.diag(N))
    return 2 * terms * U * np.outer(d, d), 2 * terms * U * d * np.sqrt(lPl), 2 * terms * U * lPl


@functools.lru_cache(maxsize=None)
def _linear_case(B):
    """TemporalParameters.linear over B daily nodes and the float64 NumPy normals of factors * (static design) with their bounds"""
    xyz, w, obs, design = _static()
    temporal = ls.TemporalParameters.linear(ti.node_mjd(B), ti.epochs(B))
    assert set(temporal.first.tolist()) == set(range(B - 1))
    A = ti.expand(design, temporal.first, temporal.factors, B)
    l = (obs * np.sqrt(w)).ravel()
    N, n, lPl = A.T @ A, A.T @ l, float(l @ l)
    return temporal, (N, n, lPl) + _bounds(N, n, lPl)


def _build(temporal, block_points=None, order=None):
    xyz, w, obs, _ = _static()
    if order is not None:
        xyz, w, obs = xyz[order], w[order], obs[order]
    return temporal.from_accelerations(xyz, obs, ti.MIN_DEGREE, ti.N, ti.GM, ti.R, weights=w, block_points=block_points)


def _full(ne):
    """(N [B P, B P] symmetric, n [B P], l^T P l, count) on the host from the upper blocks of the system"""
    upper, n, lPl, count = ne.to_array()
    return np.triu(upper) + np.triu(upper, 1).T, n[:, 0], lPl, count


def _check(ne, reference, label, B, P=ti.P, count=TERMS):
    import torch
    N, n, lPl, bound_N, bound_n, bound_l = reference
    assert isinstance(ne, ls.NormalEquations) and ne.status == 'normal_matrix' and ne.matrix.shape == (B, B)
    assert isinstance(ne.right_hand_side, torch.Tensor) and ne.right_hand_side.is_cuda and tuple(ne.right_hand_side.shape) == (B * P, 1)
    for f in range(B):
        for g in range(B):
            block = ne.matrix.device_block(f, g)
            assert block is None or (g >= f and tuple(block.shape) == (P, P)), (f, g)           # upper blocks only
        diagonal = ne.matrix.device_block(f, f)
        assert diagonal is None or bool((diagonal == diagonal.t()).all()), f                    # exactly symmetric
    got_N, got_n, got_l, got_count = _full(ne)
    assert got_N.shape == N.shape and got_count == count
    print('{0}: N {1:.2f}, n {2:.2f}, lPl {3:.2f} of their bounds'.format(label, (np.abs(got_N - N) / np.maximum(bound_N, 1e-300)).max(),
                                                                          (np.abs(got_n - n) / bound_n).max(), abs(got_l - lPl) / bound_l))
    assert np.all(np.abs(got_N - N) <= bound_N)
    assert np.all(np.abs(got_n - n) <= bound_n)
    assert abs(got_l - lPl) <= bound_l
    return got_N, got_n, got_l


@pytest.mark.parametrize('B', [4, 6])
def test_white_noise_normals_against_numpy(B):
    temporal, reference = _linear_case(B)
    bound_N, bound_n, bound_l = reference[3:]
    base = _check(_build(temporal, 256), reference, 'B {0}, blocks of 256'.format(B), B)
    for block_points in (1, 255, 257, None):
        other = _check(_build(temporal, block_points), reference, 'B {0}, blocks of {1}'.format(B, block_points), B)
        assert np.all(np.abs(other[0] - base[0]) <= bound_N) and np.all(np.abs(other[1] - base[1]) <= bound_n) and abs(other[2] - base[2]) <= bound_l
    ne = _build(temporal, 256)
    assert ne.observation_count == TERMS and isinstance(ne.observation_square_sum, float)
    assert list(ne.matrix._BlockMatrix__row_index) == list(range(0, (B + 1) * ti.P, ti.P))


def test_harmonic_normals_against_numpy():
    """static part, trend and an annual cycle: W = 4 in one run, d/o 2 .. 4"""
    xyz, w, obs, _ = _static()
    epochs = ti.epochs(6) + 365.25 * np.arange(ti.M) / ti.M                                # a year of epochs, so that the cycle is seen
    temporal = ls.TemporalParameters.harmonic(epochs, datetime.datetime(2017, 1, 1), periods=(365.25,))
    assert temporal.field_count == 4
    design = ga.gravityfield.acceleration_design_matrix(xyz, 2, 4, ti.GM, ti.R, weights=w)
    A = ti.expand(design, temporal.first, temporal.factors, 4)
    l = (obs * np.sqrt(w)).ravel()
    N, n, lPl = A.T @ A, A.T @ l, float(l @ l)
    for block_points in (None, 250):
        ne = temporal.from_accelerations(xyz, obs, 2, 4, ti.GM, ti.R, weights=w, block_points=block_points)
        _check(ne, (N, n, lPl) + _bounds(N, n, lPl), 'harmonic, blocks of {0}'.format(block_points), 4, P=21)
        assert all(ne.matrix.is_nonzero(f, g) for f in range(4) for g in range(f, 4))


def test_sum_rule():
    """the factors of linear add up to one, so the sum of all blocks is the static normal matrix, within the bound of the blocks times
    B^2 (one bound per block of the sum)"""
    B = 4
    temporal, _ = _linear_case(B)
    xyz, w, obs, _ = _static()
    static = ls.NormalEquations.from_accelerations(xyz, obs, ti.MIN_DEGREE, ti.N, ti.GM, ti.R, weights=w)
    N0, n0, lPl, _ = static.to_array()
    bound_N, bound_n, _ = _bounds(N0, n0[:, 0], lPl)
    N, n, got_l, _ = _full(_build(temporal))
    total = N.reshape(B, ti.P, B, ti.P).sum(axis=(0, 2))
    print('sum rule: {0:.2f} of the bound'.format((np.abs(total - N0) / (B * B * bound_N)).max()))
    assert np.all(np.abs(total - N0) <= B * B * bound_N)
    assert np.all(np.abs(n.reshape(B, ti.P).sum(axis=0) - n0[:, 0]) <= B * bound_n)
    assert abs(got_l - static.observation_square_sum) <= 2 * TERMS * U * lPl


@pytest.mark.parametrize('kind', ['gradients', 'line_of_sight', 'potentials', 'potential_differences'])
@pytest.mark.parametrize('noise', [False, True])
def test_the_other_kinds_of_observation(kind, noise):
    """the four siblings of from_accelerations (K = 4 with a noise model per component, and K = 1) against NumPy normals of the expanded,
    whitened matrix the device holds, and of_* against that matrix times the solution"""
    import torch
    B, q, P, M = 4, 3, ti.P, ti.M
    temporal, _ = _linear_case(B)
    a, b = ti.pair_positions()
    rng = np.random.default_rng(3581)
    gfm, band = ga.gravityfield, (ti.MIN_DEGREE, ti.N, ti.GM, ti.R)
    if kind == 'gradients':
        components, K = ('xx', 'yy', 'zz', 'xz'), 4
        w = rng.uniform(0.25, 4.0, (M, K))
        design = gfm.gradient_design_matrix(a, *band, components=components, weights=w)
        positions, extra = (a,), dict(components=components)
    elif kind in ('line_of_sight', 'potential_differences'):
        K, w = 1, rng.uniform(0.25, 4.0, M)
        design = (gfm.line_of_sight_design_matrix if kind == 'line_of_sight' else gfm.potential_difference_design_matrix)(a, b, *band, weights=w)
        positions, extra = (a, b), {}
    else:
        K, w = 1, rng.uniform(0.25, 4.0, M)
        design = gfm.potential_design_matrix(a, *band, weights=w)
        positions, extra = (a,), {}
    assert design.shape == (K * M, P)
    obs = rng.standard_normal((M, K) if K > 1 else M)
    arcs = _arcs(temporal.first)
    sequences = [wi.synthetic_sequence(ls, q, 3590 + k) for k in range(K)] if K > 1 else wi.synthetic_sequence(ls, q, 3590)
    At = ga.engine.to_device(np.ascontiguousarray(design.reshape(M, K, P).transpose(2, 1, 0)))                # [P, K, M], times sqrt(w)
    runs = np.flatnonzero(np.concatenate(([True], temporal.first[1:] != temporal.first[:-1])))
    S = ga.engine.window_expand(At.reshape(P * K, M), ga.engine.to_device(temporal.factors), temporal.first[runs], np.append(runs, M), B)
    l = np.sqrt(w) * obs
    if noise:
        taps, stage = ls.whitening_taps(sequences), ls.arc_stages(arcs, M, q)
        S = ga.engine.whiten_rows(S.reshape(B * P * K, M), ga.engine.to_device(taps), torch.from_numpy(stage).to(S.device), channels=taps.shape[0])
        l = ls.decorrelate(l, sequences, arcs=arcs)
    A = _host(S).reshape(B * P, K * M)                                                      # transposed, columns component-major
    l = np.ascontiguousarray(l.reshape(M, K).T).ravel()
    N, n, lPl = A @ A.T, A @ l, float(l @ l)
    bound = ls.TemporalParameters(temporal.first, temporal.factors, B, model=ls.ColouredNoise(sequences, arcs) if noise else None)
    for block_points in (None, 97):
        ne = getattr(bound, 'from_' + kind)(*positions, obs, *band, weights=w, block_points=block_points, **extra)
        _check(ne, (N, n, lPl) + _bounds(N, n, lPl, K * M), '{0}, noise {1}, blocks of {2}'.format(kind, noise, block_points), B, count=K * M)
    x = rng.standard_normal(B * P) * 1e-3
    fit = getattr(bound, 'of_' + kind)(x, *positions, obs, *band, weights=w, block_points=97, **extra)
    expected = (l - x @ A).reshape(K, M).T
    error_bound = 2 * (B * P + 2) * U * (np.abs(l) + np.abs(x) @ np.abs(A)).reshape(K, M).T            # a dot product of B P terms, both sides
    assert fit.whitened.shape == (M, K) and np.all(np.abs(fit.whitened - expected) <= error_bound)


# ---- 7: bitwise contracts ------------------------------------------------------------------------------------------------------------------
def _intervals(B):
    """TemporalParameters.constant arguments over B daily intervals: (edges, epochs), the last node moved inside"""
    epochs = ti.epochs(B + 1)
    epochs[-1] = np.nextafter(epochs[-1], 0.0)
    return ti.node_mjd(B + 1), epochs


@pytest.mark.parametrize('noise', [False, True])
def test_constant_is_the_static_call_per_interval(noise):
    B, block_points = 3, 100
    xyz, w, obs, _ = _static()
    edges, epochs = _intervals(B)
    index = ls.TemporalParameters.constant(edges, epochs).first
    starts = np.flatnonzero(np.concatenate(([True], index[1:] != index[:-1])))
    assert len(starts) == B and np.all(np.diff(np.append(starts, ti.M)) > block_points)     # several blocks each
    sequence = wi.synthetic_sequence(ls, 3, 3511)
    model = ls.ColouredNoise(sequence, starts) if noise else None
    ne = ls.TemporalParameters.constant(edges, epochs, model).from_accelerations(xyz, obs, ti.MIN_DEGREE, ti.N, ti.GM, ti.R, weights=w, block_points=block_points)
    total = 0.0
    for f, (a, b) in enumerate(zip(starts, np.append(starts[1:], ti.M))):
        single = ls.NormalEquations.from_accelerations(xyz[a:b], obs[a:b], ti.MIN_DEGREE, ti.N, ti.GM, ti.R, weights=w[a:b], block_points=block_points,
                                                       noise_model=sequence if noise else None)
        assert bool((ne.matrix.device_block(f, f) == single.matrix.device_block(0, 0)).all()), f
        assert bool((ne.right_hand_side[f * ti.P:(f + 1) * ti.P] == single.right_hand_side).all()), f
        total += single.observation_square_sum
    assert all(not ne.matrix.is_nonzero(f, g) for f in range(B) for g in range(B) if f != g)              # block-diagonal
    assert abs(ne.observation_square_sum - total) <= 2 * TERMS * U * total and ne.observation_count == TERMS


def test_linear_with_unit_factors_is_constant():
    B, block_points = 3, 128
    edges, epochs = _intervals(B)
    constant = ls.TemporalParameters.constant(edges, epochs)
    unit = ls.TemporalParameters(constant.first, np.tile([1.0, 0.0], (ti.M, 1)), B + 1)
    one, two = _build(constant, block_points), _build(unit, block_points)
    for f in range(B):
        assert bool((two.matrix.device_block(f, f) == one.matrix.device_block(f, f)).all()), f
        assert bool((two.right_hand_side[f * ti.P:(f + 1) * ti.P] == one.right_hand_side[f * ti.P:(f + 1) * ti.P]).all()), f
        assert bool((two.matrix.device_block(f, f + 1) == 0.0).all())
    assert bool((two.matrix.device_block(B, B) == 0.0).all()) and bool((two.right_hand_side[B * ti.P:] == 0.0).all())
    assert two.observation_square_sum == one.observation_square_sum


def test_shuffled_points_give_the_bits_of_the_sorted_call():
    B = 4
    temporal, _ = _linear_case(B)
    order = ti.reverse_runs(temporal.first)
    assert np.any(np.diff(temporal.first[order]) < 0)
    shuffled = ls.TemporalParameters(temporal.first[order], temporal.factors[order], B)
    one, two = _build(temporal, 256), _build(shuffled, 256, order)
    for f in range(B):
        for g in range(f, B):
            assert one.matrix.is_nonzero(f, g) == two.matrix.is_nonzero(f, g) == (g - f < 2)
            if g - f < 2:
                assert bool((one.matrix.device_block(f, g) == two.matrix.device_block(f, g)).all()), (f, g)
    assert bool((one.right_hand_side == two.right_hand_side).all()) and one.observation_square_sum == two.observation_square_sum
    scattered = np.random.default_rng(3522).permutation(ti.M)                               # any order: the bits of the call on the stable sort
    resorted = scattered[np.argsort(temporal.first[scattered], kind='stable')]
    three = _build(ls.TemporalParameters(temporal.first[scattered], temporal.factors[scattered], B), 256, scattered)
    four = _build(ls.TemporalParameters(temporal.first[resorted], temporal.factors[resorted], B), 256, resorted)
    assert all(bool((three.matrix.device_block(f, g) == four.matrix.device_block(f, g)).all()) for f in range(B) for g in range(f, min(f + 2, B)))
    assert bool((three.right_hand_side == four.right_hand_side).all()) and three.observation_square_sum == four.observation_square_sum
    xyz, w, obs, _ = _static()
    x = np.random.default_rng(3521).standard_normal(B * ti.P) * 1e-6
    fit = temporal.of_accelerations(x, xyz, obs, ti.MIN_DEGREE, ti.N, ti.GM, ti.R, weights=w, block_points=256)
    back = shuffled.of_accelerations(x, xyz[order], obs[order], ti.MIN_DEGREE, ti.N, ti.GM, ti.R, weights=w[order], block_points=256)
    assert np.array_equal(back.residuals, fit.residuals[order]) and np.array_equal(back.whitened, fit.whitened[order])      # in the order given


# ---- 8, 9: pattern and coloured noise ----------------------------------------------------------------------------------------------------
def _arcs(first):
    """arc starts that cut inside a run and at a run boundary"""
    starts = np.flatnonzero(np.concatenate(([True], first[1:] != first[:-1])))
    return [0, int(starts[1]) + 40, int(starts[2])]


def test_pattern():
    B = 6
    temporal, _ = _linear_case(B)
    white = _build(temporal, 100)
    for f in range(B):
        for g in range(B):
            assert white.matrix.is_nonzero(f, g) == (0 <= g - f < 2), (f, g)
    arcs = _arcs(temporal.first)
    coloured = ls.TemporalParameters(temporal.first, temporal.factors, B, model=ls.ColouredNoise(wi.synthetic_sequence(ls, 3, 3531), arcs))
    for block_points in (100, None):
        ne = _build(coloured, block_points)
        plan = ls.temporal_blocks(temporal.first, 2, 100 if block_points else 10 ** 6, ls.arc_stages(arcs, ti.M, 3))
        pattern = ls.temporal_pattern(plan)
        assert (0, 2) in pattern and (1, 3) not in pattern and (2, 4) in pattern                            # history crosses a run boundary, not an arc's
        for f in range(B):
            for g in range(B):
                assert ne.matrix.is_nonzero(f, g) == ((f, g) in pattern), (block_points, f, g)


@pytest.mark.parametrize('q', [1, 8])
def test_coloured_noise_normals_against_numpy(q):
    """against NumPy normals of the whitened expanded design matrix the device holds: the whole series expanded to all B fields in one
    call and whitened in one call, the method of tests/test_gpu_whitening.py"""
    import torch
    B = 4
    temporal, _ = _linear_case(B)
    xyz, w, obs, _ = _static()
    arcs = _arcs(temporal.first)
    sequences = [wi.synthetic_sequence(ls, q, 3540 + q), wi.synthetic_sequence(ls, q, 3550 + q), wi.synthetic_sequence(ls, q, 3560 + q)]
    taps, stage = ls.whitening_taps(sequences), ls.arc_stages(arcs, ti.M, q)
    taps_d, stage_d = ga.engine.to_device(taps), torch.from_numpy(stage).to(ga.engine.device())
    At = ga.engine.acceleration_design(ti.N, xyz, ti.GM, ti.R, ti.MIN_DEGREE, weights=w)                    # [P, 3, M], times sqrt(w)
    runs = np.flatnonzero(np.concatenate(([True], temporal.first[1:] != temporal.first[:-1])))
    S = ga.engine.window_expand(At.reshape(ti.P * 3, ti.M), ga.engine.to_device(temporal.factors), temporal.first[runs], np.append(runs, ti.M), B)
    whitened = _host(ga.engine.whiten_rows(S.reshape(B * ti.P * 3, ti.M), taps_d, stage_d, channels=3)).reshape(B * ti.P, 3 * ti.M)
    l = np.ascontiguousarray(ls.decorrelate(np.sqrt(w) * obs, sequences, arcs=arcs).T).ravel()
    N, n, lPl = whitened @ whitened.T, whitened @ l, float(l @ l)
    reference = (N, n, lPl) + _bounds(N, n, lPl)
    coloured = ls.TemporalParameters(temporal.first, temporal.factors, B, model=ls.ColouredNoise(sequences, arcs))
    for block_points in (128, 97, None):
        ne = _build(coloured, block_points)
        _check(ne, reference, 'q {0}, blocks of {1}'.format(q, block_points), B)
        again = _build(coloured, block_points)
        assert all(bool((ne.matrix.device_block(f, g) == again.matrix.device_block(f, g)).all()) for f in range(B) for g in range(B)
                   if ne.matrix.is_nonzero(f, g))
    plain = _full(_build(temporal, 128))[0]
    assert np.abs(plain - N).max() > 1e3 * reference[3].max()                                               # the model does change the normals


# ---- 11: closed loop -----------------------------------------------------------------------------------------------------------------------
def test_closed_loop_recovers_the_node_fields():
    B = 4
    xyz = ti.positions()
    epochs = ti.epochs(B)
    fields = ti.node_fields(B)
    series = ga.gravityfield.TimeSeries([pi.field(anm, epoch) for anm, epoch in zip(fields, ti.node_datetimes(B))])
    g = series.gravitational_acceleration_at(xyz, epochs)
    truth = np.concatenate([ga.utilities.ravel_coefficients(anm, ti.MIN_DEGREE, ti.N) for anm in fields])
    temporal = ls.TemporalParameters.linear(ti.node_mjd(B), epochs)
    design = ga.gravityfield.acceleration_design_matrix(xyz, ti.MIN_DEGREE, ti.N, ti.GM, ti.R)
    A = ga.gravityfield.temporal_design_matrix(design, temporal.first, temporal.factors, B)
    host = np.linalg.lstsq(A, g.ravel(), rcond=None)[0]
    host_rel_err = np.linalg.norm(host - truth) / np.linalg.norm(truth)
    scaled = A / np.linalg.norm(A, axis=0)
    assert np.linalg.cond(scaled) <= 1e2 and host_rel_err <= 1e-12
    ne = temporal.from_accelerations(xyz, g, ti.MIN_DEGREE, ti.N, ti.GM, ti.R)
    x = ne.solve()
    solution = _host(x)[:, 0]
    rel = np.linalg.norm(solution - truth) / np.linalg.norm(truth)
    print('closed loop: relative error {0:.2e} (host {1:.2e}, cond {2:.1f})'.format(rel, host_rel_err, np.linalg.cond(scaled)))
    assert rel <= 10 * host_rel_err
    recovered = temporal.fields(solution)
    assert recovered.shape == (B, ti.P)
    again = ga.gravityfield.TimeSeries([pi.field(ga.utilities.unravel_coefficients(row, ti.MIN_DEGREE, ti.N), epoch)
                                        for row, epoch in zip(recovered, ti.node_datetimes(B))])
    fit = temporal.of_accelerations(solution, xyz, g, ti.MIN_DEGREE, ti.N, ti.GM, ti.R)
    expected = g - again.gravitational_acceleration_at(xyz, epochs)
    assert isinstance(fit.residuals, np.ndarray) and fit.residuals.shape == (ti.M, 3)
    err = np.abs(fit.residuals - expected).max() / np.abs(g).max()
    print('post-fit residuals: {0:.2e} of max|g|'.format(err))
    assert err <= TOL_AX and np.array_equal(fit.whitened, fit.residuals)
    square_sum = float(np.sum(fit.whitened ** 2))
    assert abs(fit.arc_square_sums.sum() - square_sum) <= 2 * TERMS * U * square_sum


# ---- 12: the smoother ----------------------------------------------------------------------------------------------------------------------
def test_process_dynamics_constraint():
    """observations at 6 daily nodes plus a P-dimensional AR(1) process between the nodes: solution and sparse inverse against the
    dense NumPy solve and inverse of the accumulated matrix"""
    B = 6
    temporal, _ = _linear_case(B)
    ne = _build(temporal)
    scale = float(np.abs(np.diag(_full(ne)[0])).mean())
    rng = np.random.default_rng(3571)
    spread = rng.uniform(0.5, 2.0, ti.P) / scale
    process = ls.AutoregressiveModelSequence.from_covariance_function([np.diag(spread), np.diag(0.8 * spread)])
    assert process.dimension == ti.P and process.maximum_order == 1
    combined = ls.accumulate_normals([ne, process.normal_equations(B)], [1.0, 1.0])
    assert combined.observation_count == TERMS + B * ti.P
    upper, rhs, _, _ = combined.to_array()
    dense = np.triu(upper) + np.triu(upper, 1).T
    x = combined.solve()
    expected = np.linalg.solve(dense, rhs)
    err = np.abs(x[:, 0:1] - expected).max() / np.abs(expected).max()
    sigma = float(combined.posterior_sigma(x[:, 0:1]))
    combined.compute_covariance(sparse=True)
    inverse = np.linalg.inv(dense)
    worst = 0.0
    for f in range(B):
        for g in range(f, min(f + 2, B)):
            block = combined.matrix[f, g]
            assert block is not None
            worst = max(worst, np.abs(block - inverse[f * ti.P:(f + 1) * ti.P, g * ti.P:(g + 1) * ti.P]).max() / np.abs(inverse).max())
    print('smoother: solution {0:.2e}, sparse inverse {1:.2e}, cond {2:.1e}'.format(err, worst, np.linalg.cond(dense)))
    assert err < TOL and worst < TOL_INV and np.isfinite(sigma) and sigma > 0
    factors = ls.compute_variance_factors([ne, process.normal_equations(B)], combined, x[:, 0:1], [1.0, 1.0])
    assert factors.shape == (2,) and np.all(np.isfinite(factors))
