"""
The design matrix of the gravitational gradient tensor on the GPU (gravityfield.gradient_design_matrix, engine.gradient_design) and
the normal equations built from it (lstsq.NormalEquations.from_gradients): against the mp-oracle columns of
tests/golden/g25_gradient_design.npz (Earth-fixed and in the fixture's instrument frames), against the oracle tensor and the GPU
tensor of a d/o 96 field, for the kernels' contract (entries independent of the batch, the pass, min_degree, the other selected
components; identity frames; weights a row scaling; padding untouched) and through solve / accumulate_normals, closed loop included.
Every test prints its figure before it asserts.
"""
import ctypes
import functools

import numpy as np
import pytest

import acceleration_inputs as ai
import gradient_design_inputs as gdi
import gradient_inputs as gi
import grates_amd as ga

pytestmark = pytest.mark.gpu

GM, R = gdi.GM, gdi.R
GOCE = ('xx', 'yy', 'zz', 'xz')


def _host(t):
    return ga.engine.to_host(t)


def _design(xyz, min_degree, max_degree, **kwargs):
    return ga.gravityfield.gradient_design_matrix(xyz, min_degree, max_degree, GM, R, **kwargs)


def _tolerance(data):
    """5e-14 of max|A| while the recorded restatement error (1.3e-15) leaves it a factor of four, else four times the recorded value"""
    recorded = float(data['restatement_err'])
    return 5e-14 if recorded <= 5e-14 / 4 else 4 * recorded


# ---- 1: fixture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('framed', [False, True], ids=['earth_fixed', 'frames'])
@pytest.mark.parametrize('N,min_degree', [(8, 0), (8, 2), (2, 0), (2, 2)])
def test_matches_the_oracle(golden, N, min_degree, framed):
    import torch
    data = golden('g25_gradient_design')
    xyz, frames = data['xyz'], (data['frames'] if framed else None)
    ref = gdi.rotate_rows(data['A{0}'.format(N)][:, min_degree ** 2:], frames)
    A = _design(xyz, min_degree, N, frames=frames, as_tensor=True)
    assert isinstance(A, torch.Tensor) and A.is_cuda and A.dtype == torch.float64 and tuple(A.shape) == ref.shape
    At = ga.engine.gradient_design(N, xyz, GM, R, min_degree, frames)
    assert At.is_cuda and At.is_contiguous() and tuple(At.shape) == (ref.shape[1], 6, xyz.shape[0])
    assert bool((At.permute(2, 1, 0).reshape(A.shape) == A).all())
    host = _design(xyz, min_degree, N, frames=frames)
    assert isinstance(host, np.ndarray) and host.dtype == np.float64 and np.array_equal(host, _host(A)) and np.all(np.isfinite(host))
    err = np.abs(host - ref).max(axis=1).reshape(-1, 6).max(axis=1) / np.abs(ref).max()        # per point (poles: 0 .. 3, 1 mm: 12)
    print('d/o {0} from {1}, frames {2}: {3:.2e} of max|A| (worst point {4})'.format(N, min_degree, framed, err.max(), err.argmax()))
    assert err.max() <= _tolerance(data), err


# ---- 2: degree edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [0, 1, 2])
@pytest.mark.parametrize('lowest', ['0', 'N'])
def test_degree_edges_against_the_restatement(golden, N, lowest):
    data = golden('g25_gradient_design')
    min_degree = 0 if lowest == '0' else N
    xyz = data['xyz']
    for frames in (None, data['frames']):
        ref = gdi.restatement(xyz, min_degree, N, frames)
        A = _design(xyz, min_degree, N, frames=frames)
        assert A.shape == ref.shape == (120, (N + 1) ** 2 - min_degree ** 2) and np.all(np.isfinite(A))
        err = np.abs(A - ref).max() / np.abs(ref).max()
        print('d/o {0} from {1}, frames {2}: {3:.2e} of max|A|'.format(N, min_degree, frames is not None, err))
        assert err <= _tolerance(data)


# ---- 3: linearity at size ----------------------------------------------------------------------------------------------------------
def test_times_coefficients_is_the_tensor_at_degree_96(golden):
    data = golden('g25_gradient_design')
    bound = max(1e-13, 4 * float(data['ax_err']))
    tag, N = gdi.AX
    degree, kind, seed, _ = gi.CASES[tag]
    g23 = golden('g23_gradients')
    xyz, oracle = g23['xyz_' + tag], g23['T_' + tag]
    gf = ga.gravityfield.PotentialCoefficients(GM, R)
    gf.anm = gi.coefficients(degree, kind, seed)
    x = ga.utilities.ravel_coefficients(gf.anm, 0, N)
    A = _design(xyz, 0, N)
    assert degree == N and A.shape == (6 * xyz.shape[0], 9409)
    scale = np.abs(oracle).max()
    Ax = A @ x
    err = np.abs(Ax - gdi.rotate_tensor(oracle, None).ravel()).max() / scale
    print('A @ x against the oracle tensor, d/o 96: {0:.2e} of max|T| (bound {1:.1e})'.format(err, bound))
    device = gf.gravitational_gradients(xyz)
    err_device = np.abs(Ax - gdi.rotate_tensor(device, None).ravel()).max() / scale
    print('A @ x against the GPU tensor, d/o 96: {0:.2e} of max|T|'.format(err_device))
    assert err <= bound and err_device <= bound


# ---- 4: the kernels' contract --------------------------------------------------------------------------------------------------------
NC, MC = 12, 700


@functools.lru_cache(maxsize=None)
def _contract():
    """700 positions (the special ones first) and frames, their d/o-12 rows [M, 6, P] with frames and Earth-fixed, and weights"""
    xyz = np.vstack((ai.special_positions(), ai.scattered_positions(MC - 13, 2561)))
    frames = gdi.frames(MC, 2562)
    rows = _design(xyz, 0, NC, frames=frames).reshape(MC, 6, -1)
    fixed = _design(xyz, 0, NC).reshape(MC, 6, -1)
    rng = np.random.default_rng(2563)
    w = rng.uniform(0.25, 4.0, (MC, 6))
    w[rng.choice(MC, 20, replace=False), rng.integers(0, 6, 20)] = 0.0
    w[5] = 0.0
    return xyz, frames, rows, fixed, w


@pytest.mark.parametrize('M', [1, 255, 256, 257, 700])
def test_rows_do_not_depend_on_the_batch(M):
    xyz, frames, rows, fixed, _ = _contract()
    for part in (slice(0, M), slice(MC - M, MC)):                                      # other lanes, other workgroups
        assert np.array_equal(_design(xyz[part], 0, NC, frames=frames[part]).reshape(M, 6, -1), rows[part])
        assert np.array_equal(_design(xyz[part], 0, NC).reshape(M, 6, -1), fixed[part])
    flipped = _design(xyz[:M][::-1].copy(), 0, NC, frames=frames[:M][::-1].copy()).reshape(M, 6, -1)
    assert np.array_equal(flipped, rows[:M][::-1])
    assert np.array_equal(_design(xyz[:M], 0, NC, frames=frames[:M]).reshape(M, 6, -1), rows[:M])      # repeated call
    print('M = {0}: rows equal'.format(M))


def test_rows_do_not_depend_on_the_pass():
    """d/o 300 keeps the solid harmonics (degree 302) of 256 points within the 256 MB of a pass: 300 points take two passes
    (min_degree 298 keeps the matrix at 1797 columns)"""
    N, min_degree, M = 300, 298, 300
    assert (256 << 20) // 8 // (2 * (303 * 304 // 2)) == 364 and 364 // 256 * 256 == 256
    xyz = ai.scattered_positions(M, 2571)
    frames = gdi.frames(M, 2572)
    rows = _design(xyz, min_degree, N, frames=frames).reshape(M, 6, -1)
    assert rows.shape == (M, 6, 301 ** 2 - 298 ** 2) and np.all(np.isfinite(rows))
    for first, last in ((0, 256), (256, 300), (255, 257), (100, 300)):
        part = _design(xyz[first:last], min_degree, N, frames=frames[first:last]).reshape(last - first, 6, -1)
        assert np.array_equal(part, rows[first:last]), (first, last)
    w = np.random.default_rng(2573).uniform(0.0, 2.0, (M, 6))
    assert np.array_equal(_design(xyz, min_degree, N, frames=frames, weights=w).reshape(M, 6, -1), rows * np.sqrt(w)[:, :, np.newaxis])
    top = _design(xyz, N, N, frames=frames).reshape(M, 6, -1)                          # min_degree is a row slice here too
    assert np.array_equal(top, rows[:, :, 300 ** 2 - 298 ** 2:])
    print('two passes: rows equal')


def test_min_degree_is_a_row_slice():
    xyz, frames, rows, fixed, _ = _contract()
    for min_degree in (2, 5, NC):
        assert np.array_equal(_design(xyz, min_degree, NC, frames=frames).reshape(MC, 6, -1), rows[:, :, min_degree ** 2:]), min_degree
        assert np.array_equal(_design(xyz, min_degree, NC).reshape(MC, 6, -1), fixed[:, :, min_degree ** 2:]), min_degree
    print('min_degree 2, 5, 12: slices equal')


def test_identity_frames_are_no_frames():
    xyz, _, _, fixed, w = _contract()
    identity = np.tile(np.eye(3), (MC, 1, 1))
    assert np.array_equal(_design(xyz, 0, NC, frames=identity).reshape(MC, 6, -1), fixed)
    assert np.array_equal(_design(xyz, 0, NC, frames=identity, components=GOCE, weights=w[:, :4].copy()),
                          _design(xyz, 0, NC, components=GOCE, weights=w[:, :4].copy()))
    on_device = _design(ga.engine.to_device(xyz), 0, NC, frames=ga.engine.to_device(identity)).reshape(MC, 6, -1)
    assert np.array_equal(on_device, fixed)
    print('identity frames: equal')


@pytest.mark.parametrize('components', [GOCE, ('xy',), ('zz',)], ids=['goce', 'xy', 'zz'])
def test_a_subset_is_its_rows_of_the_full_set(components):
    xyz, frames, rows, fixed, _ = _contract()
    picked = gdi.component_indices(components)
    assert picked == ga.engine.gradient_components(components)
    K = len(picked)
    assert np.array_equal(_design(xyz, 0, NC, frames=frames, components=components).reshape(MC, K, -1), rows[:, picked])
    assert np.array_equal(_design(xyz, 0, NC, components=components).reshape(MC, K, -1), fixed[:, picked])
    reordered = _design(xyz, 0, NC, frames=frames, components=tuple(reversed(components))).reshape(MC, K, -1)
    assert np.array_equal(reordered, rows[:, picked])                                  # any order in, canonical order out
    print('{0}: rows equal'.format(components))


def test_weights_scale_the_rows():
    xyz, frames, rows, fixed, w = _contract()
    per_component = _design(xyz, 0, NC, frames=frames, weights=w).reshape(MC, 6, -1)
    assert np.array_equal(per_component, rows * np.sqrt(w)[:, :, np.newaxis])
    assert np.all(per_component[w == 0.0] == 0.0) and np.count_nonzero(w == 0.0) >= 20                # zero weights: zero rows
    per_point = _design(xyz, 0, NC, frames=frames, weights=w[:, 0].copy()).reshape(MC, 6, -1)
    assert np.array_equal(per_point, rows * np.sqrt(w[:, 0])[:, np.newaxis, np.newaxis])
    assert np.array_equal(_design(xyz, 0, NC, weights=w).reshape(MC, 6, -1), fixed * np.sqrt(w)[:, :, np.newaxis])
    picked = gdi.component_indices(GOCE)                                               # w [M, K] runs over the selected components
    w4 = w[:, [1, 0, 5, 2]].copy()
    subset = _design(xyz, 0, NC, frames=frames, components=GOCE, weights=w4).reshape(MC, 4, -1)
    assert np.array_equal(subset, rows[:, picked] * np.sqrt(w4)[:, :, np.newaxis])
    assert np.all(subset[w4 == 0.0] == 0.0)
    on_device = _design(ga.engine.to_device(xyz), 0, NC, frames=ga.engine.to_device(frames), weights=ga.engine.to_device(w))
    assert np.array_equal(on_device.reshape(MC, 6, -1), per_component)
    assert np.array_equal(_design(xyz, 0, NC, frames=frames, weights=np.ones(MC)).reshape(MC, 6, -1), rows)
    print('weights: rows scaled exactly')


def test_padding_is_untouched():
    import torch
    from grates_amd import _lib
    xyz, frames, _, _, w = _contract()
    M, pad, N = 300, 5, 4
    P, picked = (N + 1) ** 2, gdi.component_indices(GOCE)
    x, f, wd = ga.engine.to_device(xyz[:M]), ga.engine.to_device(frames[:M]), ga.engine.to_device(w[:M, :4])
    out = torch.full((P, 4, M + pad), -7.0, dtype=torch.float64, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call('shg_gradient_design', N, 0, ctypes.c_void_p(x.data_ptr()), M, ctypes.c_void_p(f.data_ptr()), sum(1 << j for j in picked),
              ctypes.c_void_p(wd.data_ptr()), 2, GM, R, ctypes.c_void_p(out.data_ptr()), M + pad, stream)
    got = _host(out)
    assert np.all(got[:, :, M:] == -7.0)
    expected = _design(xyz[:M], 0, N, frames=frames[:M], components=GOCE, weights=w[:M, :4].copy()).reshape(M, 4, P)
    assert np.array_equal(got[:, :, :M].transpose(2, 1, 0), expected)
    print('padding: untouched')


# ---- 5: normal equations -------------------------------------------------------------------------------------------------------------
NN, MN = 8, 300


@functools.lru_cache(maxsize=None)
def _normals_case():
    """300 positions and frames, weights [M, 4] with zeros, observations, and float64 NumPy normals from the host copy of the
    unweighted d/o-8 design matrix of (xx, yy, zz, xz)"""
    xyz = ai.scattered_positions(MN, 2581)
    frames = gdi.frames(MN, 2582)
    rng = np.random.default_rng(2583)
    w = rng.uniform(0.25, 4.0, (MN, 4))
    w[rng.choice(MN, 10, replace=False), rng.integers(0, 4, 10)] = 0.0
    obs = rng.standard_normal((MN, 4)) * 1e-9
    A = _design(xyz, 0, NN, frames=frames, components=GOCE) * np.sqrt(w).reshape(-1, 1)
    l = (obs * np.sqrt(w)).ravel()
    return xyz, frames, w, obs, A.T @ A, A.T @ l, float(l @ l)


def _build(block_points, first=0, last=MN):
    xyz, frames, w, obs = _normals_case()[:4]
    return ga.lstsq.NormalEquations.from_gradients(xyz[first:last], obs[first:last], 0, NN, GM, R, frames=frames[first:last], components=GOCE,
                                                   weights=w[first:last], block_points=block_points)


def _check_normals(ne, label, upper_only=False):
    N, n, lPl = _normals_case()[4:]
    got_N, got_n, got_l, count = ne.to_array()
    assert got_N.shape == N.shape == (81, 81) and got_n.shape == (81, 1) and count == 4 * MN
    difference = np.triu(got_N - N) if upper_only else got_N - N
    err = (np.abs(difference).max() / np.abs(N).max(), np.abs(got_n[:, 0] - n).max() / np.abs(n).max(), abs(got_l - lPl) / lPl)
    print('{0}: N {1:.2e} of max|N|, n {2:.2e} of max|n|, lPl {3:.2e}'.format(label, *err))
    assert max(err) <= 1e-13
    return got_N, got_n, got_l


def test_normals_against_numpy():
    import torch
    ne = _build(256)                                                            # two blocks, the last of 44 points
    assert isinstance(ne, ga.lstsq.NormalEquations) and ne.status == 'normal_matrix'
    assert ne.matrix.shape == (1, 1) and tuple(ne.matrix.device_block(0, 0).shape) == (81, 81)
    assert isinstance(ne.right_hand_side, torch.Tensor) and ne.right_hand_side.is_cuda and tuple(ne.right_hand_side.shape) == (81, 1)
    assert isinstance(ne.observation_square_sum, float) and ne.observation_count == 4 * MN       # zero weights still count
    _check_normals(ne, 'blocks of 256')
    N = ne.matrix.device_block(0, 0)
    assert bool((N == N.t()).all())                                             # exactly symmetric
    again = _build(256)
    assert bool((again.matrix.device_block(0, 0) == N).all()) and bool((again.right_hand_side == ne.right_hand_side).all())
    assert again.observation_square_sum == ne.observation_square_sum


def test_full_tensors_are_accepted():
    """gradients [M, 3, 3]: the selected upper-triangle entries are taken"""
    xyz, frames, w, obs = _normals_case()[:4]
    full = np.full((MN, 3, 3), np.nan)                                          # the entries that are not selected are never read
    for k, j in enumerate(gdi.component_indices(GOCE)):
        full[:, gdi.PAIRS[j][0], gdi.PAIRS[j][1]] = obs[:, k]
    ne = ga.lstsq.NormalEquations.from_gradients(xyz, full, 0, NN, GM, R, frames=frames, components=GOCE, weights=w, block_points=256)
    base = _build(256)
    assert bool((ne.right_hand_side == base.right_hand_side).all()) and ne.observation_square_sum == base.observation_square_sum
    assert bool((ne.matrix.device_block(0, 0) == base.matrix.device_block(0, 0)).all())
    print('[M, 3, 3] observations: equal')


def test_block_sizes_agree():
    base = _check_normals(_build(256), 'blocks of 256')
    for block_points in (None, 100):
        other = _check_normals(_build(block_points), 'blocks of {0}'.format(block_points))
        assert np.abs(other[0] - base[0]).max() <= 1e-13 * np.abs(base[0]).max()
        assert np.abs(other[1] - base[1]).max() <= 1e-13 * np.abs(base[1]).max()
        assert abs(other[2] - base[2]) <= 1e-13 * base[2]


def test_arcs_add_up():
    parts = [_build(256, 0, 130), _build(256, 130, MN)]
    combined = ga.lstsq.accumulate_normals(parts, [1.0, 1.0])
    assert combined.observation_count == 4 * MN
    _check_normals(combined, 'two arcs', upper_only=True)


def test_gradient_and_acceleration_normals_combine():
    xyz = _normals_case()[0]
    rng = np.random.default_rng(2584)
    g = rng.standard_normal((MN, 3)) * 1e-6
    gradients, accelerations = _build(256), ga.lstsq.NormalEquations.from_accelerations(xyz, g, 0, NN, GM, R)
    factors = [1e-24, 1e-12]                                                    # variances of 1 mE^2 and 1 (um/s^2)^2: parts of like size
    combined = ga.lstsq.accumulate_normals([gradients, accelerations], factors)
    assert combined.observation_count == 4 * MN + 3 * MN
    got = combined.to_array()
    a, b = gradients.to_array(), accelerations.to_array()
    for k in range(3):
        expected = a[k] / factors[0] + b[k] / factors[1]
        difference = np.triu(got[k] - expected) if k == 0 else got[k] - expected
        err = np.abs(difference).max() / np.abs(expected).max()
        print('combined, part {0}: {1:.2e}'.format(k, err))
        # matrix: N_a (1 / s_a) + (1 / s_b) N_b, a reciprocal and a product per part (2 u each) and the sum (u), every part at most
        # max|N| (|N_ij| <= max N_ii, and the diagonals add up): 5 u, asked as 8 u; right-hand side and l^T P l are formed as here
        assert err <= 8 * 2.0 ** -53
    x = combined.solve()                                                        # the combined right-hand side is a host array, and so is x
    assert isinstance(x, np.ndarray) and x.shape == (81, 1) and np.all(np.isfinite(x))


# ---- 6: closed loop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['all', 'goce'])
def test_closed_loop_recovers_the_field(golden, name):
    """field -> GPU tensors at 600 points -> rotated into the seeded instrument frames with torch -> normals -> solve -> field.  The
    host solves the same loop through its normals to host_rel_err (8.2e-16 for all six components, 9.0e-16 for xx, yy, zz, xz;
    cond(A) = 8.0 and 8.3); the GPU loop must stay within 10 times that."""
    import torch
    data = golden('g25_gradient_design')
    components = gdi.LOOP_SETS[name]
    host_rel_err = float(data['host_rel_err_' + name])
    assert float(data['loop_cond_' + name]) <= 1e4 and host_rel_err <= 1e-8
    N, min_degree = gdi.LOOP['N'], gdi.LOOP['min_degree']
    xyz, frames = ga.engine.to_device(gdi.loop_positions()), ga.engine.to_device(gdi.loop_frames())
    gf = ga.gravityfield.PotentialCoefficients(GM, R)
    gf.anm = gdi.loop_field()
    T = gf.gravitational_gradients(xyz, as_tensor=True)
    rotated = frames @ T @ frames.transpose(1, 2)
    K = len(components)
    if name == 'all':
        observations = rotated                                                   # [M, 3, 3]
    else:
        observations = torch.stack([rotated[:, gdi.PAIRS[j][0], gdi.PAIRS[j][1]] for j in gdi.component_indices(components)], dim=1)
    ne = ga.lstsq.NormalEquations.from_gradients(xyz, observations, min_degree, N, GM, R, frames=frames, components=components)
    assert ne.observation_count == K * 600
    x = ne.solve()
    truth = ga.utilities.ravel_coefficients(gf.anm, min_degree, N)
    solution = _host(x)[:, 0]
    rel = np.linalg.norm(solution - truth) / np.linalg.norm(truth)
    print('closed loop, {0}: relative error {1:.2e} (host {2:.2e})'.format(components, rel, host_rel_err))
    assert rel <= 10 * host_rel_err
