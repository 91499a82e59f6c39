"""
Point functionals of time-variable fields on the GPU, every point at its own epoch (the *_at methods of TimeSeries, Trend, Oscillation
and TimeVariableGravityField, engine.*_points_at, shg_*_points_at): against the reference (tests/golden/g32_points_at.npz), against
the existing [T, M, ...] entry points (one-hot weights exactly, random weights within the roundings of the weighted sum), and for the
kernel's contract: results independent of runs, workgroups, other points, field groups and source layout, reproducible calls,
pairs and the symmetry of the gradient tensor.
"""
import datetime

import numpy as np
import pytest

import acceleration_inputs as ai
import grates_amd as ga
import points_at_inputs as pi

pytestmark = pytest.mark.gpu

TOL = 5e-14          # of the fixture's scale = max_i sum_j |w_ij| |g_j(x_i)|: the TOL of tests/test_gpu_acceleration.py
EPS = 2.0 ** -52

# name: (engine function at epochs, engine function of every field, method stem, Nq - N, components C of the kernel)
FUNCTIONALS = {
    'acceleration': (ga.engine.acceleration_points_at, ga.engine.acceleration_points, 'gravitational_acceleration', 1, 3),
    'potential': (ga.engine.potential_points_at, ga.engine.potential_points, 'gravitational_potential', 0, 1),
    'gradients': (ga.engine.gravitational_gradients_points_at, ga.engine.gravitational_gradients_points, 'gravitational_gradients', 2, 6),
}
C_STEMS = {'acceleration': 'shg_acceleration_points_at', 'potential': 'shg_potential_points_at',
           'gradients': 'shg_gravitational_gradients_points_at'}
TAILS = {'acceleration': (3,), 'potential': (), 'gradients': (3, 3)}


def _host(t):
    return ga.engine.to_host(t)


def _batch(N, count, seed):
    """anm [count, N+1, N+1]: 'anomaly' and 'static' fields in turn"""
    return np.stack([ai.coefficients(N, 'static' if k % 2 else 'anomaly', seed + k) for k in range(count)])


def _series(batch, start=datetime.datetime(2010, 3, 1), step=datetime.timedelta(hours=3)):
    return ga.gravityfield.TimeSeries([pi.field(anm, start + k * step) for k, anm in enumerate(batch)])


def _datetimes(iso):
    return [datetime.datetime.fromisoformat(str(s)) for s in iso]


def _target(tag):
    parts = pi.constituents(tag)
    return parts[0] if len(parts) == 1 else ga.gravityfield.TimeVariableGravityField(parts)


@pytest.mark.parametrize('tag', list(pi.CASES))
def test_matches_reference(golden, tag):
    import torch
    data = golden('g32_points_at')
    xyz, ref, scale = data['xyz_' + tag], data['g_' + tag], float(data['scale_' + tag])
    target = _target(tag)
    for epochs in (_datetimes(data['iso_' + tag]), data['mjd_' + tag]):
        g = target.gravitational_acceleration_at(xyz, epochs)
        assert isinstance(g, np.ndarray) and g.shape == ref.shape and np.all(np.isfinite(g))
        err = np.abs(g - ref).max() / scale
        print('{0} {1}: {2:.3e} of the scale'.format(tag, type(epochs).__name__, err))
        assert err <= TOL, '{0}: {1:.3e} of the scale'.format(tag, err)
        t = target.gravitational_acceleration_at(ga.engine.to_device(xyz), epochs, as_tensor=True)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == ref.shape
        assert np.array_equal(_host(t), g)


@pytest.mark.parametrize('N', [2, 31, 63, 96])
@pytest.mark.parametrize('name', list(FUNCTIONALS))
def test_one_hot_weights_give_the_field(name, N):
    """epochs exactly on the nodes: the value is the existing entry point's value of that field at that point, from a host series and
    from a device series"""
    method = FUNCTIONALS[name][2]
    T, M = 6, 700
    series = _series(_batch(N, T, 400 + N))
    xyz = ai.scattered_positions(M, 500 + N)
    k = np.random.default_rng(600 + N).permutation(np.arange(M) % T)
    nodes = series.epochs()
    epochs = [nodes[j] for j in k]
    full = _host(getattr(series, method)(xyz, as_tensor=True))                                  # [T, M, ...]
    expected = full[k, np.arange(M)]
    got = getattr(series, method + '_at')(xyz, epochs)
    assert got.shape == expected.shape and np.all(got == expected)
    series.to_device()
    assert series.on_device
    got = _host(getattr(series, method + '_at')(xyz, epochs, as_tensor=True))
    assert series.on_device and np.all(got == expected)
    mjd = np.array([ga.utilities._mjd(e) for e in epochs])
    assert np.all(getattr(series, method + '_at')(xyz, mjd) == expected)


@pytest.fixture(scope='module')
def linear_case():
    """20 fields of d/o 20 at 300 points and every field's functionals [B, M, ...] from the existing entry points, computed once"""
    N, B, M = 20, 20, 300
    batch = _batch(N, B, 700)
    xyz = np.vstack((ai.special_positions(), ai.scattered_positions(M - ai.special_positions().shape[0], 701)))
    full = {name: _host(f[1](N, xyz, batch, ai.GM, ai.R)) for name, f in FUNCTIONALS.items()}
    for value in full.values():
        value.setflags(write=False)
    return N, B, M, batch, xyz, full


@pytest.mark.parametrize('W', [1, 2, 3, 4, 5, 12, 13, 16, 17])
@pytest.mark.parametrize('name', list(FUNCTIONALS))
def test_weighted_sum_of_the_fields(linear_case, name, W):
    """random weights, windows at 0, in the middle and at B - W (unsorted): within the two roundings per term on either side plus the
    scale, 2 (W + 2) 2^-52 sum_j |w_ij| |full_j| per component.  The kernel sweeps 2 fields at a time up to W = 2, 4 up to W = 12 (W = 5:
    two sweeps, the sum carried over), then 16 where the functional has that kernel; W = 17 is two calls (16 + 1)"""
    N, B, M, batch, xyz, full = linear_case
    rng = np.random.default_rng(800 + W)
    first = rng.choice(np.array([0, (B - W) // 2, B - W]), M)
    weights = rng.standard_normal((M, W))
    got = _host(FUNCTIONALS[name][0](N, xyz, batch, first, weights, ai.GM, ai.R))
    values = full[name]
    rows = np.arange(M)
    shape = (M,) + (1,) * (values.ndim - 2)
    expected, bound = np.zeros(values.shape[1:]), np.zeros(values.shape[1:])
    for j in range(W):
        term = weights[:, j].reshape(shape) * values[first + j, rows]
        expected += term
        bound += np.abs(term)
    assert got.shape == expected.shape
    excess = (np.abs(got - expected) - 2 * (W + 2) * EPS * bound).max()
    print('{0} W {1}: largest error {2:.3e} of its bound'.format(name, W, (np.abs(got - expected) / np.maximum(2 * (W + 2) * EPS * bound, 1e-300)).max()))
    assert excess <= 0


def _raw(name, N, x, coef, B, run_first, run_begin, w, bpad=None):
    """one shg_*_points_at(_om) call with run tables as given: device tensors x [M, 3], coef, w [M, W]"""
    import torch
    from grates_amd import _lib
    M, W = int(x.shape[0]), int(w.shape[1])
    run_first = np.ascontiguousarray(run_first, dtype=np.int32)
    run_begin = np.ascontiguousarray(run_begin, dtype=np.int32)
    out = torch.full((M,) + TAILS[name], float('nan'), dtype=torch.float64, device=x.device)
    fields = (ga.engine._ptr(coef), B) if bpad is None else (ga.engine._ptr(coef), B, bpad)
    _lib.call(C_STEMS[name] + ('' if bpad is None else '_om'), N, ga.engine._ptr(x), M, *fields, ga.engine._host_ptr(run_first),
              ga.engine._host_ptr(run_begin), len(run_first), ga.engine._ptr(w), W, ai.GM, ai.R, ga.engine._ptr(out), ga.engine._stream())
    return _host(out)


@pytest.mark.parametrize('name', list(FUNCTIONALS))
def test_result_does_not_depend_on_the_partition(name):
    """the same 1 000 points as one run, as runs of 1, 255, 256, 257 and the rest, among other points, from three field groups, from
    both source layouts and twice: the same bits"""
    N, B, M, W = 31, 9, 1000, 2
    batch = ga.engine.to_device(_batch(N, B, 900))
    xyz = ai.scattered_positions(M, 901)
    rng = np.random.default_rng(902)
    weights = rng.uniform(-1.0, 1.0, (M, W))
    x, w = ga.engine.to_device(xyz), ga.engine.to_device(weights)
    one = _raw(name, N, x, batch, B, [3], [0, M], w)
    assert np.all(np.isfinite(one))
    assert np.array_equal(_raw(name, N, x, batch, B, [3], [0, M], w), one)                     # repeated
    cuts = np.cumsum([0, 1, 255, 256, 257])
    assert np.array_equal(_raw(name, N, x, batch, B, [3] * 5, list(cuts) + [M], w), one)
    # among other points with other windows and weights, in an order the engine has to sort
    other = ai.scattered_positions(M, 903)
    mixed_x, mixed_w = np.empty((2 * M, 3)), np.empty((2 * M, W))
    mixed_x[0::2], mixed_x[1::2] = xyz, other
    mixed_w[0::2], mixed_w[1::2] = weights, rng.uniform(-1.0, 1.0, (M, W))
    mixed_first = np.empty(2 * M, dtype=np.int64)
    mixed_first[0::2], mixed_first[1::2] = 3, rng.integers(0, B - W + 1, M)
    mixed = _host(FUNCTIONALS[name][0](N, mixed_x, batch, mixed_first, mixed_w, ai.GM, ai.R))
    assert np.array_equal(mixed[0::2], one)
    # windows over all fields, the last one ending at field 8: one group of fields against at least three, and the series layout
    first = np.sort(rng.integers(0, B - W + 1, M))
    first[-1] = B - W
    order, run_first, run_begin = ga.engine.points_at_plan(first)
    assert order is None and run_first.tolist() == list(range(B - W + 1))
    spread = _raw(name, N, x, batch, B, run_first, run_begin, w)
    om = ga.engine.OrderMajorSeries.from_batch(batch)
    assert om.padded_epochs == 32
    assert np.array_equal(_raw(name, N, x, om.data, B, run_first, run_begin, w, bpad=32), spread)
    Nq, C = N + FUNCTIONALS[name][3], FUNCTIONALS[name][4]
    field_bytes = (Nq + 1) * (Nq + 2) // 2 * 2 * C * 8
    try:
        ga.engine.points_at_set_workspace_limit(4 * field_bytes)     # 4 fields per group, 3 new window starts each: 3 groups for 8 starts
        assert np.array_equal(_raw(name, N, x, batch, B, run_first, run_begin, w), spread)
        assert np.array_equal(_raw(name, N, x, om.data, B, run_first, run_begin, w, bpad=32), spread)
        assert np.array_equal(_host(FUNCTIONALS[name][0](N, xyz, batch, first, weights, ai.GM, ai.R)), spread)
        ga.engine.points_at_set_workspace_limit(W * field_bytes)     # one window per group: 8 groups
        assert np.array_equal(_raw(name, N, x, batch, B, run_first, run_begin, w), spread)
    finally:
        ga.engine.points_at_set_workspace_limit(0)
    assert np.array_equal(_raw(name, N, x, batch, B, run_first, run_begin, w), spread)
    # a point's result depends on its own window only: the one-run values are those of the points with that window
    same = first == 3
    assert same.any() and np.array_equal(spread[same], one[same])


def test_pairs_are_the_difference_of_the_points(golden):
    data = golden('g32_points_at')
    tag = 'model31'
    target = _target(tag)
    a = data['xyz_' + tag]
    b = a + np.random.default_rng(1000).uniform(1e5, 2e5, a.shape)
    epochs = _datetimes(data['iso_' + tag])
    M = a.shape[0]
    g = ga.engine._torch().cat((target.gravitational_acceleration_at(a, epochs, as_tensor=True),
                                target.gravitational_acceleration_at(b, epochs, as_tensor=True)))
    los = target.line_of_sight_acceleration_at(a, b, epochs)
    assert los.shape == (M,) and np.array_equal(los, _host(ga.gravityfield._project_line_of_sight(g, a, b, None)))
    e = np.random.default_rng(1001).standard_normal((M, 3))
    e /= np.sqrt(np.sum(e * e, axis=1))[:, np.newaxis]
    forward = target.line_of_sight_acceleration_at(a, b, epochs, directions=e)
    assert np.array_equal(forward, _host(ga.gravityfield._project_line_of_sight(g, a, b, e)))
    backward = _host(target.line_of_sight_acceleration_at(b, a, data['mjd_' + tag], directions=e, as_tensor=True))
    mjd_forward = target.line_of_sight_acceleration_at(a, b, data['mjd_' + tag], directions=e)
    assert np.array_equal(backward, -mjd_forward) and np.any(forward != 0)
    V = target.gravitational_potential_at(np.vstack((a, b)), epochs + epochs)
    d = target.potential_difference_at(a, b, epochs)
    assert d.shape == (M,) and np.array_equal(d, V[M:] - V[:M])
    assert np.array_equal(target.potential_difference_at(a, b, epochs), -target.potential_difference_at(b, a, epochs))


def test_gradients_are_symmetric_and_trace_free(golden):
    data = golden('g32_points_at')
    tag = 'model31'
    T = _target(tag).gravitational_gradients_at(data['xyz_' + tag], _datetimes(data['iso_' + tag]))
    assert T.shape == (data['xyz_' + tag].shape[0], 3, 3) and np.all(np.isfinite(T))
    assert np.array_equal(T, T.transpose(0, 2, 1))
    trace = np.abs(T[:, 0, 0] + T[:, 1, 1] + T[:, 2, 2]).max()
    print('trace {0:.3e} of max|T|'.format(trace / np.abs(T).max()))
    assert trace <= 1e-12 * np.abs(T).max()                          # xx, yy and zz come from their own sums: a check, not an identity
