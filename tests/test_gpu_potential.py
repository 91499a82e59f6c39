"""
The energy-balance observations on the GPU: the gravitational potential at points (PotentialCoefficients / TimeSeries
.gravitational_potential and .potential_difference, engine.potential_points), its design matrix and that of the potential difference of
satellite pairs (gravityfield.potential_design_matrix / potential_difference_design_matrix, engine.potential_design /
potential_difference_design) and the normal equations built from them (lstsq.NormalEquations.from_potentials /
from_potential_differences, bound by ColouredNoise and ArcParameters, and PostFit.of_potentials): against the reference's grid
synthesis of the potential on spheres (tests/golden/g28_potential.npz), against the float64 restatement of the kernel's formulas,
against the acceleration through Euler's identity, for the kernels' contracts (values independent of batch, layout and pass,
reproducible, min_degree a row slice, weights a scaling, pairs swapped and coincident) and through solve, closed loops with and without
one energy constant per arc included.

Rounding errors of a pair's row are proportional to the matrices of the two satellites, not to their difference, so the bounds are
fractions of max|A_pot| (the fixture's pot_scale); the figure relative to max|A_dif| of the 220 km pairs is printed only.
"""
import functools

import numpy as np
import pytest

import acceleration_inputs as ai
import design_inputs as di
import grates_amd as ga
import potential_inputs as pi
import whitening_inputs as wi

pytestmark = pytest.mark.gpu

TOL = 5e-14          # of max|A_pot| (design entries) and of max|V| (forward values); the fixture's restatement_err, 1.2e-15, and
#                      forward_err, 1.9e-15, are below a quarter of it
TOL_AX = 1e-13       # of max|V|: design matrix times coefficients against the forward functional (the fixture's ax_err is 1.2e-15)
TOL_G = 5e-14        # of max|g|: the acceleration suite's bound (tests/test_gpu_acceleration.py)
U = 2.0 ** -53
MAX_EP = 16          # epochs per pass of the point kernel with shared points (Potential::kMaxEP)


def _host(t):
    return ga.engine.to_host(t)


def _field(anm, epoch=None):
    gf = ga.gravityfield.PotentialCoefficients(pi.GM, pi.R)
    gf.anm = anm
    if epoch is not None:
        gf.epoch = epoch
    return gf


def _check_tolerances(data):
    assert float(data['restatement_err']) <= TOL / 4 and float(data['forward_err']) <= TOL / 4 and float(data['ax_err']) <= TOL_AX / 4


def _design(xyz, min_degree, max_degree, **kwargs):
    return ga.gravityfield.potential_design_matrix(xyz, min_degree, max_degree, pi.GM, pi.R, **kwargs)


def _pair_design(a, b, min_degree, max_degree, **kwargs):
    return ga.gravityfield.potential_difference_design_matrix(a, b, min_degree, max_degree, pi.GM, pi.R, **kwargs)


# ---- forward functional ---------------------------------------------------------------------------------------------------------------
def test_forward_matches_reference(golden):
    import torch
    data = golden('g28_potential')
    _check_tolerances(data)
    xyz, ref = data['xyz60'], data['V60']
    gf = _field(pi.v60_field())
    V = gf.gravitational_potential(xyz)
    assert isinstance(V, np.ndarray) and V.dtype == np.float64 and V.shape == ref.shape
    on_device = gf.gravitational_potential(ga.engine.to_device(xyz), as_tensor=True)
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and on_device.dtype == torch.float64 and np.array_equal(_host(on_device), V)
    err = np.abs(V - ref).max() / float(data['V60_scale'])
    print('d/o 60, 413 points: {0:.2e} of max|V|'.format(err))
    assert err <= TOL


@pytest.mark.parametrize('N', [8, 2])
def test_forward_of_unit_fields_is_the_fixture_matrix(golden, N):
    """all (N + 1)^2 unit fields in one batch (81 fields: six passes of 16 epochs, the last partial): row p is column p of A_pot"""
    data = golden('g28_potential')
    _check_tolerances(data)
    batch = np.stack([di.unit_field(n, m, sine, N) for n, m, sine in di.degreewise(0, N)])
    V = _host(ga.engine.potential_points(N, data['xyz'], batch, pi.GM, pi.R))
    ref = data['A_pot{0}'.format(N)]
    assert V.shape == ((N + 1) ** 2, 20) and np.all(np.isfinite(V))
    err = np.abs(V.T - ref).max() / float(data['pot_scale{0}'.format(N)])
    print('d/o {0} unit fields: {1:.2e} of max|A_pot|'.format(N, err))
    assert err <= TOL


def test_forward_degree_zero():
    """N = 0: V = GM C00 / r, one product of the recursion's seed"""
    xyz = np.vstack((ai.special_positions(), ai.scattered_positions(287, 2831)))
    anm = np.array([[1.25]])
    V = _field(anm).gravitational_potential(xyz)
    ref = pi.GM * 1.25 / pi.radius_of(xyz)
    assert V.shape == (300,) and np.abs(V / ref - 1.0).max() <= 8 * U


@functools.lru_cache(maxsize=None)
def _case70():
    """d/o 70 (past the 64-degree LDS stage), 300 points (a full workgroup and a partial one; the special positions first): a static and
    an anomaly field, with their float64 restatement"""
    N = 70
    xyz = np.vstack((ai.special_positions(), ai.scattered_positions(287, 2832)))
    fields = (ai.coefficients(N, 'static', 2833), ai.coefficients(N, 'anomaly', 2834))
    return N, xyz, fields, [pi.forward(xyz, anm) for anm in fields]


@pytest.mark.parametrize('M', [257, 300])
def test_forward_at_degree_70_matches_the_restatement(M):
    N, xyz, fields, ref = _case70()
    for anm, expected, kind in zip(fields, ref, ('static', 'anomaly')):
        V = _field(anm).gravitational_potential(xyz[:M])
        scale = np.abs(expected).max()
        err = np.abs(V - expected[:M]).max() / scale
        print('d/o 70 {0}, {1} points: {2:.2e} of max|V|'.format(kind, M, err))
        assert np.all(np.isfinite(V)) and err <= TOL


@pytest.mark.parametrize('n', [0, 1, 2, 64, 65, 96])
def test_euler_identity_against_the_acceleration(n):
    """V of a field of the single degree n is homogeneous of degree -(n + 1) in x: x . g = -(n + 1) V, with g the GPU acceleration.  The
    bound is the sum of the two suites': each component of g within TOL_G max|g|, so x . g within TOL_G max|g| (|x| + |y| + |z|), and
    (n + 1) V within (n + 1) TOL max|V|.  The point 1 mm off the pole is left out: within 1.5e-8 rad of the axis the reference's
    s = sqrt(1 - t^2), which both kernels follow, is exactly 0, so both evaluate the field on the axis while x keeps its millimetre:
    x g_x / (r g) = 1.6e-10 there is the form's own defect (the float64 restatement and the host acceleration show the same 460 times
    the bound at degree 1), and nothing the identity can test."""
    rng = np.random.default_rng(2840 + n)
    anm = np.zeros((n + 1, n + 1))
    anm[n, :] = rng.standard_normal(n + 1)
    anm[:n, n] = rng.standard_normal(n)
    gf = _field(anm)
    xyz = np.vstack((ai.special_positions()[:12], ai.scattered_positions(88, 2839)))
    V = gf.gravitational_potential(xyz)
    g = _host(gf.gravitational_acceleration(xyz, as_tensor=True))
    defect = np.abs(np.sum(xyz * g, axis=1) + (n + 1) * V)
    bound = TOL_G * np.abs(g).max() * np.abs(xyz).sum(axis=1) + (n + 1) * TOL * np.abs(V).max()
    print('degree {0}: x . g + (n + 1) V is {1:.2f} of its bound'.format(n, (defect / bound).max()))
    assert np.all(np.isfinite(V)) and np.all(defect <= bound)


@functools.lru_cache(maxsize=None)
def _fields40(count=MAX_EP + 3):
    return [_field(ai.coefficients(40, 'anomaly' if k % 2 else 'static', 2850 + k), epoch=k) for k in range(count)]


def test_batches_layouts_and_series_give_the_same_bits():
    """each field alone (EP = 1), batches of 1, 3, 5 (EP = 1, 4, 16, the last two with a partial pass) and MAX_EP + 3 fields (two
    passes), the per-epoch layout, the device series in its order-major layout and a repeated call: the same bits for a field"""
    import torch
    fields = _fields40()
    xyz = np.vstack((ai.special_positions(), ai.scattered_positions(287, 2851)))
    single = torch.stack([f.gravitational_potential(xyz, as_tensor=True) for f in fields])
    assert tuple(single.shape) == (MAX_EP + 3, 300) and bool(single.isfinite().all())
    for count in (1, 3, 5, MAX_EP + 3):
        series = ga.gravityfield.TimeSeries(fields[:count])
        shared = series.gravitational_potential(xyz, as_tensor=True)
        assert tuple(shared.shape) == (count, 300) and bool((shared == single[:count]).all()), count
        assert bool((series.gravitational_potential(xyz, as_tensor=True) == shared).all())           # repeated call
        host = series.gravitational_potential(xyz)
        assert isinstance(host, np.ndarray) and np.array_equal(host, _host(shared))
    three = ga.gravityfield.TimeSeries(fields[:3])
    per_epoch = three.gravitational_potential(np.stack([xyz, xyz[::-1], xyz]), as_tensor=True)
    assert bool((per_epoch[0] == single[0]).all()) and bool((per_epoch[1] == single[1].flip(0)).all()) and bool((per_epoch[2] == single[2]).all())
    batch = ga.gravityfield.TimeSeries(fields).to_coefficient_batch()
    assert bool((ga.engine.potential_points(40, xyz, batch, pi.GM, pi.R) == single).all())
    device = ga.gravityfield.TimeSeries.from_series(batch, range(len(fields)))
    assert device.on_device
    assert bool((device.gravitational_potential(xyz, as_tensor=True) == single).all()) and device.on_device
    assert bool((device.gravitational_potential(np.broadcast_to(xyz, (len(fields), 300, 3)).copy(), as_tensor=True) == single).all())


def test_mixed_constants_fall_back_to_one_call_per_field():
    fields = [_field(ai.coefficients(20, 'static', 2860 + k), epoch=k) for k in range(3)]
    fields[1].GM *= 1.001
    fields[2].R *= 0.999
    xyz = ai.scattered_positions(100, 2861)
    V = ga.gravityfield.TimeSeries(fields).gravitational_potential(xyz)
    for k, f in enumerate(fields):
        assert np.array_equal(V[k], f.gravitational_potential(xyz)), k


def test_potential_difference_is_the_difference_of_two_forward_calls():
    fields = _fields40(3)
    a = np.vstack((ai.special_positions(), ai.scattered_positions(87, 2871)))
    b = a + pi.SEPARATION * np.roll(a, 1, axis=1) / pi.radius_of(a)[:, np.newaxis]
    b[::10] = a[::10]
    for f in fields:
        d = f.potential_difference(a, b)
        assert isinstance(d, np.ndarray) and d.shape == (100,)
        assert np.array_equal(d, f.gravitational_potential(b) - f.gravitational_potential(a))
        assert np.all(d[::10] == 0.0) and np.all(d[1:10] != 0.0)
        assert np.array_equal(_host(f.potential_difference(ga.engine.to_device(a), ga.engine.to_device(b), as_tensor=True)), d)
    series = ga.gravityfield.TimeSeries(list(fields))
    shared = series.potential_difference(a, b)
    assert shared.shape == (3, 100)
    stacked = series.potential_difference(np.stack([a, b, a]), np.stack([b, a, b]))
    for k, f in enumerate(fields):
        assert np.array_equal(shared[k], f.potential_difference(a, b)), k
    assert np.array_equal(stacked[0], shared[0]) and np.array_equal(stacked[1], -shared[1]) and np.array_equal(stacked[2], shared[2])


# ---- design matrices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,min_degree', [(8, 0), (8, 2), (2, 0), (2, 2)])
def test_design_matches_reference(golden, N, min_degree):
    import torch
    data = golden('g28_potential')
    _check_tolerances(data)
    xyz = data['xyz']
    ref = data['A_pot{0}{1}'.format(N, '_min2' if min_degree else '')]
    scale = float(data['pot_scale{0}'.format(N)])
    A = _design(xyz, min_degree, N, as_tensor=True)
    assert isinstance(A, torch.Tensor) and A.is_cuda and A.dtype == torch.float64 and tuple(A.shape) == ref.shape
    At = ga.engine.potential_design(N, xyz, pi.GM, pi.R, min_degree)
    assert At.is_cuda and At.is_contiguous() and tuple(At.shape) == (ref.shape[1], 20) and bool((At.t() == A).all())
    host = _design(xyz, min_degree, N)
    assert isinstance(host, np.ndarray) and np.array_equal(host, _host(A)) and np.all(np.isfinite(host))
    err = np.abs(host - ref).max(axis=1)
    print('d/o {0} from {1}: {2:.2e} of max|A_pot| (worst point {3})'.format(N, min_degree, err.max() / scale, err.argmax()))
    assert err.max() <= TOL * scale, err / scale


@pytest.mark.parametrize('N,min_degree', [(8, 0), (8, 2), (2, 0), (2, 2)])
def test_pair_design_matches_reference(golden, N, min_degree):
    data = golden('g28_potential')
    _check_tolerances(data)
    a, b = data['xyz_a'], data['xyz_b']
    ref = data['A_dif{0}{1}'.format(N, '_min2' if min_degree else '')]
    scale = float(data['pot_scale{0}'.format(N)])
    host = _pair_design(a, b, min_degree, N)
    assert host.shape == ref.shape and np.all(np.isfinite(host))
    assert np.array_equal(_host(ga.engine.potential_difference_design(N, a, b, pi.GM, pi.R, min_degree)).T, host)
    sep = pi.separations()
    assert np.all(host[sep == 0.0] == 0.0)                                          # a == b: an exactly zero row
    err = np.abs(host - ref).max(axis=1)
    far = sep > 100e3
    print('d/o {0} from {1}: {2:.2e} of max|A_pot| (worst pair {3}); {4:.2e} of max|A_dif| at 220 km'.format(
        N, min_degree, err.max() / scale, err.argmax(), err[far].max() / np.abs(ref[far]).max()))
    assert err.max() <= TOL * scale, err / scale


NC, MC = 12, 300


@functools.lru_cache(maxsize=None)
def _contract():
    """300 points and pairs (a: the special positions first; separations of 220 km, 1 km, 1 m and 0 in turn), their d/o-12 design
    matrices [M, P] on the host, weights with zeros among them"""
    a = np.vstack((ai.special_positions(), ai.scattered_positions(MC - 13, 2881)))
    sep = np.array((pi.SEPARATION, 1e3, 1.0, 0.0))[np.arange(MC) % 4]
    d = np.random.default_rng(2882).standard_normal((MC, 3))
    b = a + sep[:, np.newaxis] * d / np.sqrt(np.sum(d * d, axis=1))[:, np.newaxis]
    b[sep == 0.0] = a[sep == 0.0]
    rng = np.random.default_rng(2883)
    w = rng.uniform(0.25, 4.0, MC)
    w[rng.choice(MC, 10, replace=False)] = 0.0
    return a, b, sep, _design(a, 0, NC), _pair_design(a, b, 0, NC), w


@pytest.mark.parametrize('M', [1, 63, 64, 65, 257, 300])
def test_rows_do_not_depend_on_the_batch(M):
    a, b, _, rows, pair_rows, _ = _contract()
    assert rows.shape == pair_rows.shape == (MC, (NC + 1) ** 2) and np.all(np.isfinite(rows)) and np.all(np.isfinite(pair_rows))
    for s in (slice(0, M), slice(MC - M, MC)):                                      # other lanes, other workgroups
        assert np.array_equal(_design(a[s].copy(), 0, NC), rows[s])
        assert np.array_equal(_pair_design(a[s].copy(), b[s].copy(), 0, NC), pair_rows[s])
    assert np.array_equal(_design(a[:M][::-1].copy(), 0, NC), rows[:M][::-1])
    assert np.array_equal(_design(a[:M].copy(), 0, NC), rows[:M])                   # repeated call


def test_min_degree_is_a_row_slice():
    a, b, _, rows, pair_rows, _ = _contract()
    for min_degree in (2, 5, NC):
        assert np.array_equal(_design(a, min_degree, NC), rows[:, min_degree ** 2:]), min_degree
        assert np.array_equal(_pair_design(a, b, min_degree, NC), pair_rows[:, min_degree ** 2:]), min_degree


def test_weights_scale_as_the_last_operation():
    a, b, _, rows, pair_rows, w = _contract()
    root = np.sqrt(w)[:, np.newaxis]
    weighted = _design(a, 0, NC, weights=w)
    assert np.array_equal(weighted, rows * root) and np.all(weighted[w == 0.0] == 0.0) and np.count_nonzero(w == 0.0) >= 10
    assert np.array_equal(_pair_design(a, b, 0, NC, weights=w), pair_rows * root)
    assert np.array_equal(_design(ga.engine.to_device(a), 0, NC, weights=ga.engine.to_device(w)), rows * root)
    assert np.array_equal(_design(a, 0, NC, weights=np.ones(MC)), rows)
    assert np.array_equal(_pair_design(a, b, 0, NC, weights=np.ones(MC)), pair_rows)


def test_padding_of_a_wider_buffer_is_untouched():
    """ldt > M through the C entry points: the columns M .. ldt of a NaN-filled buffer stay NaN, the others are the dense call's"""
    import torch
    from grates_amd import _lib
    a, b, _, rows, pair_rows, w = _contract()
    M, ldt, P = MC, MC + 37, (NC + 1) ** 2
    da, db, dw = (ga.engine.to_device(x) for x in (a, b, w))
    stream = torch.cuda.current_stream().cuda_stream
    root = np.sqrt(w)[:, np.newaxis]
    for weights, scale in ((None, 1.0), (dw, root)):
        wp = None if weights is None else weights.data_ptr()
        for expected, call in ((rows, lambda out: _lib.call('shg_potential_design', NC, 0, da.data_ptr(), M, wp, pi.GM, pi.R, out.data_ptr(), ldt, stream)),
                               (pair_rows, lambda out: _lib.call('shg_potential_difference_design', NC, 0, da.data_ptr(), db.data_ptr(), M, wp, pi.GM, pi.R,
                                                                 out.data_ptr(), ldt, stream))):
            out = torch.full((P, ldt), float('nan'), dtype=torch.float64, device=da.device)
            call(out)
            torch.cuda.synchronize()
            assert bool(out[:, M:].isnan().all())
            assert np.array_equal(_host(out[:, :M]).T, expected * scale)


def test_swapping_the_satellites_negates_bitwise():
    a, b, sep, _, pair_rows, w = _contract()
    assert np.array_equal(_pair_design(b, a, 0, NC), -pair_rows)
    assert np.array_equal(_pair_design(b, a, 0, NC, weights=w), -(pair_rows * np.sqrt(w)[:, np.newaxis]))
    assert np.all(pair_rows[sep == 0.0] == 0.0) and np.all(np.abs(pair_rows[sep > 0.0]).max(axis=1) > 0.0)
    assert np.all(_pair_design(a, a, 0, NC) == 0.0)


def test_pair_design_equals_the_composed_route_at_degree_65():
    """d/o 65, 300 pairs: the fused At against potential_design(b) - potential_design(a) formed in torch.  Both routes read bitwise the
    same harmonics; the fused one rounds the difference and the product with GM / R, the composed one the two products and the
    difference: at most four roundings of values below 2 max|A_pot|, 8 * 2^-52 max|A_pot| in all."""
    N, M = 65, 300
    a_host = np.vstack((ai.special_positions(), ai.scattered_positions(M - 13, 2884)))
    sep = np.where(np.arange(M) % 3 == 0, 1e3, pi.SEPARATION)
    d = np.random.default_rng(2885).standard_normal((M, 3))
    a = ga.engine.to_device(a_host)
    b = ga.engine.to_device(a_host + sep[:, np.newaxis] * d / np.sqrt(np.sum(d * d, axis=1))[:, np.newaxis])
    A_a, A_b = (ga.engine.potential_design(N, x, pi.GM, pi.R) for x in (a, b))
    scale = max(float(A_a.abs().max()), float(A_b.abs().max()))
    composed = A_b - A_a
    fused = ga.engine.potential_difference_design(N, a, b, pi.GM, pi.R)
    assert tuple(fused.shape) == tuple(composed.shape) == ((N + 1) ** 2, M) and bool(fused.isfinite().all())
    err = float((fused - composed).abs().max())
    print('fused against composed, d/o 65: {0:.2f} x 2^-52 max|A_pot| ({1:.2e} of max|A_dif|)'.format(err / scale * 2.0 ** 52,
                                                                                                      err / float(composed.abs().max())))
    assert err <= 8 * 2.0 ** -52 * scale


def test_times_coefficients_is_the_forward_functional_at_degree_96(golden):
    _check_tolerances(golden('g28_potential'))
    N, M = 96, 300
    xyz = np.vstack((ai.special_positions(), ai.scattered_positions(M - 13, 2886)))
    b = np.roll(xyz, 5, axis=0)
    gf = _field(ai.coefficients(N, 'anomaly', 2887))
    x = ga.utilities.ravel_coefficients(gf.anm, 0, N)
    V = gf.gravitational_potential(xyz)
    scale = np.abs(V).max()
    A = _design(xyz, 0, N)
    assert A.shape == (M, 9409)
    err = np.abs(A @ x - V).max() / scale
    print('A @ x against gravitational_potential, d/o 96: {0:.2e} of max|V|'.format(err))
    assert err <= TOL_AX
    assert np.abs(_design(xyz, 2, N) @ x[4:] - V).max() <= TOL_AX * scale          # the field has nothing below degree 2
    # a pair: the bound is that of its two satellites
    err = np.abs(_pair_design(xyz, b, 0, N) @ x - gf.potential_difference(xyz, b)).max() / scale
    print('A_dif @ x against potential_difference, d/o 96: {0:.2e} of max|V|'.format(err))
    assert err <= 2 * TOL_AX


# ---- normal equations -----------------------------------------------------------------------------------------------------------------
N8 = 8


@functools.lru_cache(maxsize=None)
def _normals_case():
    """the 300 points and pairs of _contract at d/o 8 with weights and seeded observations: the weighted design matrices [M, P] as the
    GPU built them, on the host"""
    a, b, _, _, _, w = _contract()
    obs = np.random.default_rng(2888).standard_normal(MC) * 1e-2
    return a, b, w, obs, _design(a, 0, N8, weights=w), _pair_design(a, b, 0, N8, weights=w)


def _check_normals(ne, A, l, label):
    """against float64 NumPy normals of the downloaded design matrix, entry-wise within 2 K 2^-53 sqrt(N_ii N_jj) and its like: the
    standard bound K u |a| |b| of a dot product of length K, once for each side of the comparison"""
    N, n, lPl = A.T @ A, A.T @ l, float(l @ l)
    K = A.shape[0]
    d = np.sqrt(np.diag(N))
    got_N, got_n, got_l, count = ne.to_array()
    assert got_N.shape == N.shape and got_n.shape == (N.shape[0], 1) and count == K
    bound_N, bound_n, bound_l = 2 * K * U * np.outer(d, d), 2 * K * U * d * np.sqrt(lPl), 2 * K * U * lPl
    print('{0}: N {1:.2f}, n {2:.2f}, lPl {3:.2f} of their bounds'.format(label, (np.abs(got_N - N) / bound_N).max(),
                                                                          (np.abs(got_n[:, 0] - n) / bound_n).max(), abs(got_l - lPl) / bound_l))
    assert np.all(np.abs(got_N - N) <= bound_N) and np.all(np.abs(got_n[:, 0] - n) <= bound_n) and abs(got_l - lPl) <= bound_l
    assert np.array_equal(got_N, got_N.T)
    return got_N, got_n, got_l, (bound_N, bound_n, bound_l)


@pytest.mark.parametrize('block_points', [None, 128])
def test_normals_against_numpy(block_points):
    """one block, and blocks of 128 (three, the last of 44 points)"""
    import torch
    a, b, w, obs, A, A_dif = _normals_case()
    l = obs * np.sqrt(w)
    ne = ga.lstsq.NormalEquations.from_potentials(a, obs, 0, N8, pi.GM, pi.R, weights=w, block_points=block_points)
    assert isinstance(ne, ga.lstsq.NormalEquations) and ne.status == 'normal_matrix' and ne.observation_count == MC
    assert tuple(ne.matrix.device_block(0, 0).shape) == (81, 81)
    assert isinstance(ne.right_hand_side, torch.Tensor) and ne.right_hand_side.is_cuda and tuple(ne.right_hand_side.shape) == (81, 1)
    _check_normals(ne, A, l, 'potentials, block_points {0}'.format(block_points))
    pairs = ga.lstsq.NormalEquations.from_potential_differences(a, b, obs, 0, N8, pi.GM, pi.R, weights=w, block_points=block_points)
    assert pairs.observation_count == MC
    _check_normals(pairs, A_dif, l, 'differences, block_points {0}'.format(block_points))


def test_blocks_agree_with_one_block():
    a, b, w, obs, A, A_dif = _normals_case()
    l = obs * np.sqrt(w)
    for build, args, rows in ((ga.lstsq.NormalEquations.from_potentials, (a,), A), (ga.lstsq.NormalEquations.from_potential_differences, (a, b), A_dif)):
        one = _check_normals(build(*args, obs, 0, N8, pi.GM, pi.R, weights=w), rows, l, 'one block')
        blocks = _check_normals(build(*args, obs, 0, N8, pi.GM, pi.R, weights=w, block_points=128), rows, l, 'blocks of 128')
        bound_N, bound_n, bound_l = one[3]
        assert np.all(np.abs(blocks[0] - one[0]) <= bound_N) and np.all(np.abs(blocks[1] - one[1])[:, 0] <= bound_n)
        assert abs(blocks[2] - one[2]) <= bound_l


def _loop_truth():
    gf = _field(pi.loop_field())
    return gf, ga.utilities.ravel_coefficients(gf.anm, pi.LOOP['min_degree'], pi.LOOP['N'])


def _relative_error(x, truth):
    solution = (x if isinstance(x, np.ndarray) else _host(x))[:, 0]
    return np.linalg.norm(solution - truth) / np.linalg.norm(truth), solution


def test_closed_loops_recover_the_field(golden):
    """field -> GPU potentials (potential differences) of 600 points (pairs) -> normals -> solve -> field.  The host solves the same
    loops through its normals to host_rel_err = 7.5e-16 and 1.1e-15 (cond(A) = 2.7 and 3.4, recorded in the fixture); the GPU loops must
    stay within 10 times that."""
    data = golden('g28_potential')
    assert np.all(data['loop_cond'] <= 1e4) and np.all(data['host_rel_err'] <= 1e-8)
    N, min_degree = pi.LOOP['N'], pi.LOOP['min_degree']
    gf, truth = _loop_truth()
    a, b = (ga.engine.to_device(x) for x in pi.loop_pairs()[:2])
    ne = ga.lstsq.NormalEquations.from_potentials(a, gf.gravitational_potential(a, as_tensor=True), min_degree, N, pi.GM, pi.R)
    assert ne.observation_count == 600
    rel, solution = _relative_error(ne.solve(), truth)
    print('closed loop, V: relative error {0:.2e} (host {1:.2e})'.format(rel, float(data['host_rel_err'][0])))
    assert rel <= 10 * float(data['host_rel_err'][0])
    anm = ga.utilities.unravel_coefficients(solution, min_degree, N)
    assert anm.shape == gf.anm.shape and np.abs(anm - gf.anm).max() <= 10 * float(data['host_rel_err'][0]) * np.linalg.norm(truth)
    ne.compute_covariance(sparse=False)
    assert ne.status == 'covariance_matrix' and np.all(ne.matrix.diag() > 0)
    pairs = ga.lstsq.NormalEquations.from_potential_differences(a, b, gf.potential_difference(a, b, as_tensor=True), min_degree, N, pi.GM, pi.R)
    rel, _ = _relative_error(pairs.solve(), truth)
    print('closed loop, V(b) - V(a): relative error {0:.2e} (host {1:.2e})'.format(rel, float(data['host_rel_err'][1])))
    assert rel <= 10 * float(data['host_rel_err'][1])


def _arc_loop():
    """the observations of the arc-constant loop: V of the loop field at 600 points plus the planted constant of each of the 12 arcs"""
    gf, truth = _loop_truth()
    xyz = pi.loop_positions()[0]
    arcs, constants = pi.loop_arcs(), pi.loop_constants()
    obs = gf.gravitational_potential(xyz) + np.repeat(constants, pi.LOOP['arc_length'])
    return gf, truth, xyz, arcs, constants, obs


def test_arc_constants_are_eliminated_and_recovered(golden):
    """The energy constant of an arc is lstsq.arc_basis(arcs, M, degree=0) under ArcParameters.  The field comes back within 10 times the
    host's error of the same loop (1.0e-15; cond 2.7 with the constants projected out).  The constant of an arc is the mean over the arc
    of l - A x: it inherits |A (x^ - x)| <= max_i |A_i| |x^ - x| from the field, the forward values' own TOL max|V| from l, and the
    rounding of two sums of 50 and of P terms of the size of |l| + |A_i| |x|."""
    data = golden('g28_potential')
    host_rel_err = float(data['host_rel_err'][2])
    N, min_degree = pi.LOOP['N'], pi.LOOP['min_degree']
    gf, truth, xyz, arcs, constants, obs = _arc_loop()
    model = ga.lstsq.ArcParameters(ga.lstsq.arc_basis(arcs, 600, degree=0), arcs)
    ne = model.from_potentials(xyz, obs, min_degree, N, pi.GM, pi.R)
    assert ne.observation_count == 600 - 12 and ne.arc_elimination.count == 12 and np.all(ne.arc_elimination.ranks == 1)
    x = ne.solve()
    rel, solution = _relative_error(x, truth)
    print('arc-constant loop: relative error {0:.2e} (host {1:.2e})'.format(rel, host_rel_err))
    assert rel <= 10 * host_rel_err
    estimated = ne.arc_elimination.parameters(x)
    assert estimated.shape == (12, 1, 1)
    row_norm = np.sqrt(np.sum(_design(xyz, min_degree, N) ** 2, axis=1)).max()
    terms = np.abs(obs).max() + row_norm * np.linalg.norm(truth)
    bound = 10 * host_rel_err * np.linalg.norm(truth) * row_norm + TOL * np.abs(obs).max() + (pi.LOOP['arc_length'] + truth.size + 4) * U * terms
    print('arc constants: {0:.2e} off, bound {1:.2e}'.format(np.abs(estimated[:, 0, 0] - constants).max(), bound))
    assert np.all(np.abs(estimated[:, 0, 0] - constants) <= bound)
    # the same pairs' loop under the same model: a constant per arc in V(b) - V(a) (the two satellites' constants differ)
    a, b = pi.loop_pairs()[:2]
    differences = gf.potential_difference(a, b) + np.repeat(constants, pi.LOOP['arc_length'])
    pairs = model.from_potential_differences(a, b, differences, min_degree, N, pi.GM, pi.R)
    px = pairs.solve()
    rel, _ = _relative_error(px, truth)
    print('arc-constant loop of the pairs: relative error {0:.2e}'.format(rel))
    assert rel <= 10 * max(host_rel_err, float(data['host_rel_err'][1]))
    assert np.all(np.abs(pairs.arc_elimination.parameters(px)[:, 0, 0] - constants) <= 2 * bound)


def test_coloured_noise_against_host_whitened_normals():
    """ColouredNoise of order 2 (the 'ar2' process of the whitening fixture) over the 12 arcs of the arc-constant loop: against normals
    formed on the host from the downloaded design matrix and the dense W of the arcs (whitening_inputs.dense_filter).  A whitened entry
    is a sum of at most 3 products and a normal a dot product of 600 of them: entry-wise within 2 (600 + 5) 2^-53 of the same products
    of absolute values, once for each side of the comparison."""
    N, min_degree = pi.LOOP['N'], pi.LOOP['min_degree']
    gf, truth, xyz, arcs, _, _ = _arc_loop()
    obs = gf.gravitational_potential(xyz) + np.random.default_rng(2889).standard_normal(600) * 1e-3
    sequence = ga.lstsq.AutoregressiveModelSequence.from_covariance_function(wi.covariance_function('ar2'))
    ne = ga.lstsq.ColouredNoise(sequence, arcs).from_potentials(xyz, obs, min_degree, N, pi.GM, pi.R)
    W = wi.dense_filter(ga.lstsq.whitening_taps(sequence)[0], ga.lstsq.arc_stages(arcs, 600, 2))
    A = _design(xyz, min_degree, N)
    Aw, lw, Am, lm = W @ A, W @ obs, np.abs(W) @ np.abs(A), np.abs(W) @ np.abs(obs)
    got_N, got_n, got_l, count = ne.to_array()
    c = 2 * (600 + 5) * U
    print('coloured noise: N {0:.3f}, n {1:.3f}, lPl {2:.3f} of their bounds'.format(
        (np.abs(got_N - Aw.T @ Aw) / (c * (Am.T @ Am))).max(), (np.abs(got_n[:, 0] - Aw.T @ lw) / (c * (Am.T @ lm))).max(),
        abs(got_l - float(lw @ lw)) / (c * float(lm @ lm))))
    assert count == 600 and np.all(np.abs(got_N - Aw.T @ Aw) <= c * (Am.T @ Am))
    assert np.all(np.abs(got_n[:, 0] - Aw.T @ lw) <= c * (Am.T @ lm)) and abs(got_l - float(lw @ lw)) <= c * float(lm @ lm)
    # the same noise model under the arc constants: the two bound models agree on what they share
    both = ga.lstsq.ArcParameters(ga.lstsq.arc_basis(arcs, 600, degree=0), arcs, noise_model=sequence).from_potentials(xyz, obs, min_degree, N, pi.GM, pi.R)
    assert both.observation_count == 600 - 12
    rel, _ = _relative_error(both.solve(), truth)
    assert rel < 0.1                                                                 # noise of 1e-3 on a signal of 5e-2: a sanity bound only


def test_normals_add_to_those_of_accelerations(golden):
    """orbit energy and orbit accelerations of one field, same degrees, summed by accumulate_normals, solve to that field: the sum of
    two positive definite matrices is conditioned no worse than the worse of the two, so the bound is 10 times the larger host error"""
    data, orbit = golden('g28_potential'), golden('g24_acceleration_design')
    host_rel_err = max(float(data['host_rel_err'][0]), float(orbit['host_rel_err']))
    N, min_degree = pi.LOOP['N'], pi.LOOP['min_degree']
    assert (N, min_degree) == (di.LOOP['N'], di.LOOP['min_degree'])
    gf, truth = _loop_truth()
    xyz = ga.engine.to_device(pi.loop_positions()[0])
    other = ga.engine.to_device(di.loop_positions())
    energy = ga.lstsq.NormalEquations.from_potentials(xyz, gf.gravitational_potential(xyz, as_tensor=True), min_degree, N, pi.GM, pi.R)
    orbit_ne = ga.lstsq.NormalEquations.from_accelerations(other, gf.gravitational_acceleration(other, as_tensor=True), min_degree, N, pi.GM, pi.R)
    # V is GM / R ~ 6e7 times the coefficients, g GM / R^2 ~ 10: weigh the systems to a common scale as a combination would
    combined = ga.lstsq.accumulate_normals([energy, orbit_ne], [pi.R ** 2, 1.0])
    assert combined.observation_count == 600 + 1800
    rel, _ = _relative_error(combined.solve(), truth)
    print('energy and accelerations: relative error {0:.2e} (host loops {1:.2e})'.format(rel, host_rel_err))
    assert rel <= 10 * host_rel_err


def test_post_fit_of_potentials():
    """PostFit.of_potentials under the arc-constant model with noisy observations: the residuals are l - A x - B y to rounding, the arcs'
    redundancies sum to M - P - arcs when the vectors make the trace estimate exact (sqrt(P) times the unit vectors: their mean
    square is the trace itself), and covariance_function has the documented shape"""
    N, min_degree = pi.LOOP['N'], pi.LOOP['min_degree']
    gf, truth, xyz, arcs, constants, clean = _arc_loop()
    obs = clean + np.random.default_rng(2890).standard_normal(600) * 1e-3
    model = ga.lstsq.ArcParameters(ga.lstsq.arc_basis(arcs, 600, degree=0), arcs)
    ne = model.from_potentials(xyz, obs, min_degree, N, pi.GM, pi.R)
    P = truth.size
    solved = ga.lstsq.accumulate_normals([ne], [1.0])
    x = solved.solve(signs=np.sqrt(P) * np.eye(P))
    x = x if isinstance(x, np.ndarray) else _host(x)
    vectors = solved.monte_carlo_vectors
    vectors = vectors if isinstance(vectors, np.ndarray) else _host(vectors)
    fit = ga.lstsq.PostFit.of_potentials(x, xyz, obs, min_degree, N, pi.GM, pi.R, model=model, vectors=vectors)
    assert isinstance(fit.residuals, np.ndarray) and fit.residuals.shape == fit.whitened.shape == (600, 1)
    assert fit.arc_parameters.shape == (12, 1, 1) and np.array_equal(fit.arcs, arcs) and np.all(fit.ranks == 1)
    assert np.array_equal(fit.arc_observation_counts, np.full(12, 49))
    A = _design(xyz, min_degree, N)
    y = np.repeat(fit.arc_parameters[:, 0, 0], pi.LOOP['arc_length'])
    expected = obs - A @ x[:, 0] - y
    scale = np.abs(obs).max() + np.sqrt(np.sum(A * A, axis=1)).max() * np.linalg.norm(x) + np.abs(y).max()
    err = np.abs(fit.residuals[:, 0] - expected).max()
    print('residuals: {0:.2e} off l - A x - B y, {1:.2e} of the terms'.format(err, err / scale))
    assert err <= 4 * (P + 4) * U * scale
    assert np.abs(fit.whitened - fit.residuals).max() <= 4 * (P + 4) * U * scale     # white noise: W is the identity
    assert np.abs(fit.arc_parameters[:, 0, 0] - constants).max() < 5e-3              # noise of 1e-3 over 50 points, twelve times
    assert abs(fit.arc_square_sums.sum() - float(ne.residual_square_sum(x))) <= 1e-9 * fit.arc_square_sums.sum()
    redundancies = fit.arc_redundancies()
    assert redundancies.shape == (12,) and np.all(redundancies > 0)
    print('redundancies sum to {0:.9f}, M - P - arcs = {1}'.format(redundancies.sum(), 600 - P - 12))
    assert abs(redundancies.sum() - (600 - P - 12)) <= 1e-9 * 600
    function = fit.covariance_function(5)
    assert isinstance(function, list) and len(function) == 6 and all(c.shape == (1, 1) for c in function)
    assert abs(function[0][0, 0] - float(np.sum(fit.residuals ** 2)) / 600) <= 1e-12 * function[0][0, 0]
    per_component = fit.covariance_function(3, per_component=True, biased=False)
    assert len(per_component) == 1 and len(per_component[0]) == 4
