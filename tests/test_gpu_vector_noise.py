"""
Vector noise models on the GPU: the kernel of shg_whiten_rows_vector (engine.whiten_rows_vector,
lstsq.decorrelate) against the filter in extended precision within the bound of its FMA chain, bitwise across halo blocks, tile seams
and repeated calls; the kernel of shg_segment_cross_lag_products against exact sums and, on its diagonal, bitwise against
shg_segment_lag_products; the normal equations of every constructor under a lstsq.VectorNoise against extended-precision products of the
dense filter; and the loop residuals -> PostFit.vector_noise -> decorrelate.
"""
import functools

import numpy as np
import pytest

import acceleration_inputs as ai
import arc_inputs as arc
import design_inputs as di
import gradient_design_inputs as gdi
import grates_amd as ga
import rbf_inputs as ri
import temporal_inputs as ti
import vector_noise_reference as vr
import whitening_inputs as wi

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ARCS = [0, 1, 4, 300]                 # an arc of one point, one shorter than q = 5, one that ends inside the first tile
SENTINEL = -7.25
GROUPS = 5
CASES = [(3, 5), (2, 128), (6, 3)]    # (K, q)


def _host(t):
    return t if isinstance(t, np.ndarray) else ga.engine.to_host(t)


def _int32(values):
    import torch
    return torch.from_numpy(np.asarray(values, dtype=np.int32)).to(ga.engine.device())


def _padded(values, ld, fill):
    """device matrix [rows, ld] filled with `fill`, `values` in its first columns; returns the matrix and the view of the values"""
    import torch
    rows, M = values.shape
    full = torch.full((rows, ld), fill, dtype=torch.float64, device=ga.engine.device())
    full[:, :M] = ga.engine.to_device(values)
    return full, full[:, :M]


# ---- 1: the whitening kernel against the filter in extended precision ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(K, q):
    """(taps, stage, X [GROUPS K, M], reference, bound, tile) on the host: M = two tiles and 37 columns, four arcs"""
    tile = ga.engine.whiten_vector_info(K)['tile_columns']
    M = 2 * tile + 37
    taps = ga.lstsq.VectorNoise(vr.synthetic_sequence(ga.lstsq, K, q, 2920 + K)).taps()
    stage = ga.lstsq.arc_stages(ARCS, M, q)
    X = np.random.default_rng(2930 + K).standard_normal((GROUPS * K, M))
    reference, magnitude, n = vr.extended_filter(taps, stage, X.reshape(GROUPS, K, M))
    return taps, stage, X, reference.reshape(GROUPS * K, M), vr.filter_bound(K, n, magnitude).reshape(GROUPS * K, M), tile


@functools.lru_cache(maxsize=None)
def _whole(K, q):
    """the whole-matrix result of a case with leading dimensions M + 4: (Y on the host, the device buffers of X and Y)"""
    taps, stage, X = _case(K, q)[:3]
    M = X.shape[1]
    X_full, X_view = _padded(X, M + 4, float('nan'))                  # a read of the padding of X would poison the result
    Y_full, Y_view = _padded(np.zeros_like(X), M + 4, SENTINEL)
    out = ga.engine.whiten_rows_vector(X_view, ga.engine.to_device(taps), _int32(stage), out=Y_view)
    assert out is Y_view
    return _host(Y_view), X_full, Y_full


@pytest.mark.parametrize('K, q', CASES)
def test_kernel_against_the_extended_filter(K, q):
    """entry-wise within (K (n + 1) + 1) u sum |H| |x|: the K (n + 1) roundings of the kernel's chain, one product and K (n + 1) - 1 FMAs,
    and one unit for the reference (numpy.longdouble sums, whose own error is 2^-11 of that, rounded to float64 once)"""
    taps, stage, X, reference, bound, tile = _case(K, q)
    Y, X_full, Y_full = _whole(K, q)
    M = X.shape[1]
    assert Y.shape == X.shape and np.all(np.isfinite(Y))
    assert bool((Y_full[:, M:] == SENTINEL).all()) and bool(X_full[:, M:].isnan().all())          # the padding of Y is untouched
    ratio = np.abs(Y - reference) / bound
    print('K {0}, q {1}, tile {2}: {3:.3f} of the bound (row, column {4})'.format(
        K, q, tile, ratio.max(), tuple(int(v) for v in np.unravel_index(ratio.argmax(), ratio.shape))))
    assert np.all(np.abs(Y - reference) <= bound)
    assert np.abs(Y - X).max() > 1e6 * bound.max()                                                 # and the filter does something
    tables = ga.engine.to_device(taps), _int32(stage)
    dense = ga.engine.whiten_rows_vector(ga.engine.to_device(X), *tables)
    assert dense.is_contiguous() and np.array_equal(_host(dense), Y)                               # ldx = ldy = M, a new output
    assert np.array_equal(_host(ga.engine.whiten_rows_vector(ga.engine.to_device(X), *tables)), Y) # repeated calls are bitwise equal
    shaped = ga.engine.whiten_rows_vector(ga.engine.to_device(X.reshape(GROUPS, K, M)), *tables)
    assert tuple(shaped.shape) == (GROUPS, K, M) and np.array_equal(_host(shaped).reshape(GROUPS * K, M), Y)
    single = ga.engine.whiten_rows_vector(ga.engine.to_device(X[2 * K:3 * K]), *tables)            # a group does not see the others
    assert np.array_equal(_host(single), Y[2 * K:3 * K])


def test_order_zero_is_the_product_chain_bitwise():
    """q = 0: y[c] = H[0][0][c][0] x[0], then fma(H[0][0][c][c'], x[c'], .) for c' = 1, 2: every fma is the exact sum rounded once"""
    from fractions import Fraction
    K = 3
    taps, stage, X = _case(K, 5)[:3]
    M = 300
    H = np.ascontiguousarray(taps[:1, :1])
    Y = _host(ga.engine.whiten_rows_vector(ga.engine.to_device(X[:, :M]), ga.engine.to_device(H), _int32(np.zeros(M))))
    expected = np.zeros_like(Y)
    for g in range(GROUPS):
        for c in range(K):
            for t in range(M):
                acc = H[0, 0, c, 0] * X[g * K, t]
                for cc in range(1, K):
                    acc = float(Fraction(H[0, 0, c, cc]) * Fraction(X[g * K + cc, t]) + Fraction(acc))
                expected[g * K + c, t] = acc
    assert np.array_equal(Y, expected)


@pytest.mark.parametrize('K, q', CASES)
def test_stage_is_clamped(K, q):
    """a table of garbage gives a finite result and no fault: a negative stage is order 0, one above q or above the column is cut"""
    taps, stage, X = _case(K, q)[:3]
    M = X.shape[1]
    wrong = stage.copy()
    wrong[[10, 11, 400, M - 1]] = -7, 10 ** 6, 2 ** 31 - 1, 10 ** 6
    wrong[[0, 1, 2]] = q, 10 ** 6, -7
    clamped = vr.clamp(wrong, q).astype(np.int32)
    Xd, taps_d = ga.engine.to_device(X), ga.engine.to_device(taps)
    got = ga.engine.whiten_rows_vector(Xd, taps_d, _int32(wrong))
    expected = ga.engine.whiten_rows_vector(Xd, taps_d, _int32(clamped))
    assert bool((got == expected).all()) and bool(got.isfinite().all())


# ---- 2: seams --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K, q', CASES)
def test_block_with_halo_is_bitwise_the_whole(K, q):
    taps, stage, X, _, _, tile = _case(K, q)
    Y, X_full, _ = _whole(K, q)
    M = X.shape[1]
    taps_d, stage_d = ga.engine.to_device(taps), _int32(stage)
    for first in (1, 3, 4, 256, 299, 300, 301, tile, 2 * tile):
        h = int(stage[first])
        block = ga.engine.whiten_rows_vector(X_full[:, first - h:M], taps_d, stage_d[first - h:], skip=h)
        assert tuple(block.shape) == (X.shape[0], M - first)
        assert np.array_equal(_host(block), Y[:, first:]), first
        if h < first:                                       # a longer halo than needed changes nothing either
            longer = ga.engine.whiten_rows_vector(X_full[:, :M], taps_d, stage_d, skip=first)
            assert np.array_equal(_host(longer), Y[:, first:]), first
    Y_full, _ = _padded(np.full_like(X, SENTINEL), M + 4, SENTINEL)
    out = ga.engine.whiten_rows_vector(X_full[:, :M], taps_d, stage_d, skip=M, out=Y_full[:, :0])  # a skip of everything writes nothing
    assert tuple(out.shape) == (X.shape[0], 0) and bool((Y_full == SENTINEL).all())


def test_decorrelate():
    import torch
    K, q = 3, 5
    taps, stage, X = _case(K, q)[:3]
    Y = _whole(K, q)[0]
    noise = ga.lstsq.VectorNoise(vr.synthetic_sequence(ga.lstsq, K, q, 2920 + K))
    values = np.ascontiguousarray(X[:K].T)                                            # [M, 3]: component c is row c
    host = ga.lstsq.decorrelate(values, noise, arcs=ARCS)
    assert isinstance(host, np.ndarray) and host.shape == values.shape and np.array_equal(host, Y[:K].T)
    device = ga.lstsq.decorrelate(ga.engine.to_device(values), noise, arcs=ARCS)
    assert isinstance(device, torch.Tensor) and device.is_cuda and tuple(device.shape) == values.shape and np.array_equal(_host(device), host)
    for bad in (X[:2].T, X[:4].T):                                                    # the engine call refuses rows that are no groups
        with pytest.raises(ValueError, match='are not groups of the 3 components'):
            ga.engine.whiten_rows_vector(ga.engine.to_device(np.ascontiguousarray(bad.T)), ga.engine.to_device(taps), _int32(stage))


# ---- 3: the cross-lag kernel -----------------------------------------------------------------------------------------------------------------
ML = 700
SEGMENTS = [0, 1, 4, 300, 300, 700]   # the arcs of the whitening tests, with an empty segment
INNER = [2, 5, 5, 650]                # columns 0, 1 and 650 .. 699 belong to no segment


@pytest.mark.parametrize('lags', [0, 5, 128])
def test_cross_lag_products(lags):
    K = 3
    X = np.random.default_rng(2950 + lags).standard_normal((K, ML))
    full, view = _padded(X, ML + 4, float('nan'))
    S = ga.engine.segment_cross_lag_products(view, _int32(SEGMENTS), lags)
    assert tuple(S.shape) == (len(SEGMENTS) - 1, lags + 1, K, K) and S.is_contiguous()
    S = _host(S)
    assert np.all(np.isfinite(S))
    scalar = _host(ga.engine.segment_lag_products(view, _int32(SEGMENTS), lags))                           # [K, nseg, lags + 1]
    for c in range(K):
        assert np.array_equal(S[:, :, c, c], scalar[c]), c                                                 # the diagonal, bitwise
    reference, magnitude, pairs = vr.exact_cross(X, SEGMENTS, lags)
    bound = vr.cross_bound(magnitude, pairs)
    ratio = np.abs(S - reference) / np.where(bound > 0, bound, 1.0)
    print('lags {0}: {1:.3f} of the chain bound'.format(lags, ratio.max()))
    assert np.all(np.abs(S - reference) <= bound)
    assert not np.any(S[pairs == 0]) and not np.any(np.signbit(S[pairs == 0]))                              # no pair: exactly +0.0
    assert not np.any(S[3])                                                                                # the empty segment
    if lags:
        assert np.abs(S[4, 1] - S[4, 1].T).max() > 1e6 * bound[4, 1].max()                                 # lag k is not symmetric in (c, c')
    assert np.array_equal(_host(ga.engine.segment_cross_lag_products(view, _int32(SEGMENTS), lags)), S)    # repeated calls are bitwise equal
    # time reversal: S'[s'][k][c][c'] of x'[t] = x[M - 1 - t] is S[s][k][c'][c]; both are within the bound of the exact sums
    reversed_seg = [ML - value for value in SEGMENTS[::-1]]
    R = _host(ga.engine.segment_cross_lag_products(ga.engine.to_device(np.ascontiguousarray(X[:, ::-1])), _int32(reversed_seg), lags))
    assert np.all(np.abs(R[::-1].transpose(0, 1, 3, 2) - S) <= 2 * bound)
    # NaN outside every segment is not read, and a segment gives the same bits wherever the table puts it
    poisoned = X.copy()
    poisoned[:, :2] = np.nan
    poisoned[:, 650:] = np.nan
    inner = _host(ga.engine.segment_cross_lag_products(_padded(poisoned, ML + 4, float('nan'))[1], _int32(INNER), lags))
    assert np.all(np.isfinite(inner)) and not np.any(inner[1])
    alone = _host(ga.engine.segment_cross_lag_products(ga.engine.to_device(np.ascontiguousarray(X[:, 5:650])), _int32([0, 645]), lags))
    assert np.array_equal(inner[2], alone[0])
    garbage = _host(ga.engine.segment_cross_lag_products(view, _int32([-7, 1, 4, 10 ** 6, 300, 700]), lags))   # clamped: [0, 1, 4, 700, 700, 700]
    assert np.array_equal(garbage[:2], S[:2]) and not np.any(garbage[3:]) and np.all(np.isfinite(garbage))


# ---- 4: normal equations ---------------------------------------------------------------------------------------------------------------------
def _reference_normals(rows, l, noise, arcs):
    """(N, n, lPl, bounds) from the transposed design matrix rows [P, K, M] and the observations l [K, M], both as the device holds them
    before the filter (times sqrt(w)): the dense W applied and the three products formed in numpy.longdouble.  The bounds are
    (K M + 2 K (q + 1) + 4) u sqrt(N~_ii N~_jj) with N~ = (|W| |A|)^T (|W| |A|), and alike for n and l^T P l: an entry is a dot product
    of K M terms (K M roundings in any order of summation) of two factors that each carry the K (q + 1) roundings of the filter's
    chain, and 4 more for the two sides' final roundings and the reference's own."""
    P, K, M = rows.shape
    taps, q = noise.taps(), noise.maximum_order
    stage = ga.lstsq.arc_stages(arcs, M, q)
    A, Am, _ = vr.extended_filter(taps, stage, rows, keep=True)
    b, bm, _ = vr.extended_filter(taps, stage, l[np.newaxis], keep=True)
    A, Am, b, bm = A.reshape(P, K * M), Am.reshape(P, K * M), b.reshape(K * M), bm.reshape(K * M)
    factor = (K * M + 2 * K * (q + 1) + 4) * U
    d, e = np.sqrt(np.einsum('ij,ij->i', Am, Am).astype(np.float64)), float(np.sqrt(bm @ bm))
    bounds = factor * np.outer(d, d), factor * d * e, factor * e * e
    return (A @ A.T).astype(np.float64), (A @ b).astype(np.float64), float(b @ b), bounds, A.astype(np.float64), b.astype(np.float64)


def _check(ne, reference, label, count):
    N, n, lPl, (bound_N, bound_n, bound_l) = reference[:4]
    got_N, got_n, got_l, got_count = ne.to_array()
    assert got_N.shape == N.shape and got_n.shape == (N.shape[0], 1) and got_count == count
    print('{0}: N {1:.3f}, n {2:.3f}, lPl {3:.3f} of their bounds'.format(label, (np.abs(got_N - N) / bound_N).max(),
                                                                          (np.abs(got_n[:, 0] - n) / bound_n).max(), abs(got_l - lPl) / bound_l))
    assert np.all(np.abs(got_N - N) <= bound_N)
    assert np.all(np.abs(got_n[:, 0] - n) <= bound_n)
    assert abs(got_l - lPl) <= bound_l
    matrix = ne.matrix.device_block(0, 0)
    assert bool((matrix == matrix.t()).all())                                                      # exactly symmetric
    return ne


def _same(first, second):
    return (bool((first.matrix.device_block(0, 0) == second.matrix.device_block(0, 0)).all()) and bool((first.right_hand_side == second.right_hand_side).all())
            and first.observation_square_sum == second.observation_square_sum and first.observation_count == second.observation_count)


NA, MA = 12, 700


@functools.lru_cache(maxsize=None)
def _noise(K=3):
    """the VectorNoise of the known VAR(2) process of dimension K"""
    return ga.lstsq.VectorNoise(vr.process_sequence(ga.lstsq, K))


@functools.lru_cache(maxsize=None)
def _acceleration_case():
    """700 positions, point weights with zeros, observations, and the reference normals from the plain d/o-12 design matrix"""
    xyz = np.vstack((di.positions(), ai.scattered_positions(MA - 20, 2721)))
    rng = np.random.default_rng(2961)
    w = rng.uniform(0.25, 4.0, MA)
    w[rng.choice(MA, 20, replace=False)] = 0.0
    w[[0, 3, 4, 299, 300]] = 0.0
    obs = rng.standard_normal((MA, 3)) * 1e-3
    At = _host(ga.engine.acceleration_design(NA, xyz, di.GM, di.R, 0, weights=w))                        # [P, 3, M], times sqrt(w)
    l = np.ascontiguousarray((np.sqrt(w)[:, np.newaxis] * obs).T)
    return xyz, w, obs, At, l, _reference_normals(At, l, _noise(), ARCS)


def _build_accelerations(block_points, **kwargs):
    xyz, w, obs = _acceleration_case()[:3]
    return ga.lstsq.NormalEquations.from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w, block_points=block_points, **kwargs)


@pytest.mark.parametrize('block_points', [256, 100, None])
def test_normals_of_accelerations(block_points):
    reference = _acceleration_case()[5]
    ne = _check(_build_accelerations(block_points, noise_model=_noise(), arcs=ARCS), reference, 'blocks of {0}'.format(block_points), 3 * MA)
    assert ne.status == 'normal_matrix' and ne.right_hand_side.is_cuda
    assert _same(_build_accelerations(block_points, noise_model=_noise(), arcs=ARCS), ne)          # two runs are bitwise equal
    xyz, w, obs = _acceleration_case()[:3]
    bound = ga.lstsq.ColouredNoise(_noise(), ARCS).from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w, block_points=block_points)
    assert _same(bound, ne)                                                                        # and so is the bound form
    plain = reference[0] - _host(_build_accelerations(block_points).matrix.device_block(0, 0))
    assert np.abs(plain).max() > 1e3 * reference[3][0].max()                                       # and the model does change the normals
    # the components are coupled: the diagonal of the same model, one scalar sequence per component, gives other normals
    if block_points == 256:
        assert _same(_build_accelerations(256, noise_model=None), _build_accelerations(256))       # no model: nothing changes


NG, MG = 8, 300
TWO_ARCS = [0, 140]
GOCE = ('xx', 'yy', 'zz', 'xz')


def test_normals_of_gradients():
    """K = 4 components; blocks of 128: the second starts an arc's 12 points before the arc ends, the third inside"""
    noise = _noise(4)
    xyz, frames = ai.scattered_positions(MG, 2734), gdi.frames(MG, 2735)
    rng = np.random.default_rng(2962)
    w = rng.uniform(0.25, 4.0, (MG, 4))
    w[rng.choice(MG, 10, replace=False), rng.integers(0, 4, 10)] = 0.0
    obs = rng.standard_normal((MG, 4)) * 1e-9
    At = _host(ga.engine.gradient_design(NG, xyz, gdi.GM, gdi.R, 0, frames=frames, components=GOCE, weights=w))            # [P, 4, M]
    reference = _reference_normals(At, np.ascontiguousarray((np.sqrt(w) * obs).T), noise, TWO_ARCS)

    def build():
        return ga.lstsq.ColouredNoise(noise, TWO_ARCS).from_gradients(xyz, obs, 0, NG, gdi.GM, gdi.R, frames=frames, components=GOCE, weights=w,
                                                                      block_points=128)
    ne = _check(build(), reference, 'gradients', 4 * MG)
    assert _same(build(), ne)


def test_normals_of_radial_basis_parameters():
    c = ri.LOOP
    lon, lat, a_nodes, f_nodes = ri.loop_nodes()
    basis = ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat, a=a_nodes, f=f_nodes),
                                                 ri.shape_factors(ri.degree_factors(c['min_degree'], c['max_degree'])), c['min_degree'],
                                                 c['max_degree'], ri.GM, ri.R)
    a = ri.loop_pairs()[0]
    M, J = a.shape[0], lon.size
    obs = np.random.default_rng(2963).standard_normal((M, 3)) * 1e-3
    A = ga.gravityfield.rbf_acceleration_design_matrix(basis, a)                 # [3 M, J], row 3 i + c, from the kernel of the blocks
    rows = np.ascontiguousarray(A.reshape(M, 3, J).transpose(2, 1, 0))
    arcs = [0, 280]
    reference = _reference_normals(rows, np.ascontiguousarray(obs.T), _noise(), arcs)

    def build():
        return ga.lstsq.RadialBasisParameters(basis, ga.lstsq.ColouredNoise(_noise(), arcs)).from_accelerations(a, obs, block_points=256)
    ne = _check(build(), reference, 'radial basis', 3 * M)
    assert _same(build(), ne)


def test_normals_of_temporal_parameters():
    B = 4
    temporal = ga.lstsq.TemporalParameters.linear(ti.node_mjd(B), ti.epochs(B))
    xyz, w, obs = ti.positions(), ti.weights(), ti.observations()
    arcs = [0, 250]
    At = _host(ga.engine.acceleration_design(ti.N, xyz, ti.GM, ti.R, ti.MIN_DEGREE, weights=w))           # [P, 3, M], times sqrt(w)
    design = np.ascontiguousarray(At.transpose(2, 1, 0)).reshape(3 * ti.M, ti.P)
    expanded = ti.expand(design, temporal.first, temporal.factors, B)                                     # [3 M, B P]: exact products or zeros
    rows = np.ascontiguousarray(expanded.reshape(ti.M, 3, B * ti.P).transpose(2, 1, 0))
    N, n, lPl, (bound_N, bound_n, bound_l) = _reference_normals(rows, np.ascontiguousarray((np.sqrt(w) * obs).T), _noise(), arcs)[:4]
    bound = ga.lstsq.TemporalParameters(temporal.first, temporal.factors, B, model=ga.lstsq.ColouredNoise(_noise(), arcs))
    results = []
    for block_points in (None, 97):
        ne = bound.from_accelerations(xyz, obs, ti.MIN_DEGREE, ti.N, ti.GM, ti.R, weights=w, block_points=block_points)
        worst = 0.0
        for f in range(B):
            for g in range(f, B):
                rows_f, rows_g = slice(f * ti.P, (f + 1) * ti.P), slice(g * ti.P, (g + 1) * ti.P)
                if ne.matrix.is_nonzero(f, g):
                    block = _host(ne.matrix.device_block(f, g))
                    worst = max(worst, (np.abs(block - N[rows_f, rows_g]) / bound_N[rows_f, rows_g]).max())
                    assert np.all(np.abs(block - N[rows_f, rows_g]) <= bound_N[rows_f, rows_g]), (f, g)
                else:
                    assert not np.any(N[rows_f, rows_g]), (f, g)
        side = _host(ne.right_hand_side)[:, 0]
        print('temporal, blocks of {0}: N {1:.3f}, n {2:.3f} of their bounds'.format(block_points, worst, (np.abs(side - n) / bound_n).max()))
        assert np.all(np.abs(side - n) <= bound_n) and abs(ne.observation_square_sum - lPl) <= bound_l and ne.observation_count == 3 * ti.M
        results.append(ne)
    again = bound.from_accelerations(xyz, obs, ti.MIN_DEGREE, ti.N, ti.GM, ti.R, weights=w, block_points=97)
    assert bool((again.right_hand_side == results[1].right_hand_side).all())
    assert all(bool((again.matrix.device_block(f, f) == results[1].matrix.device_block(f, f)).all()) for f in range(B))


def _arc_reference(basis, shared_columns):
    """the reduced system of the acceleration case under ArcParameters(basis): the whitened A~ and l~ of _reference_normals rounded to
    float64, the whitened basis alike, the projection of tests/golden/arc_inputs.py (float64), and bounds: those of the products plus
    the projection's own, arc_inputs.normals_bounds, which tests/test_gpu_arc_parameters.py allows that reference"""
    xyz, w, obs, At, l, reference = _acceleration_case()
    noise = _noise()
    root = np.repeat(np.sqrt(w)[:, np.newaxis], 3, axis=1)
    Bt = np.ascontiguousarray((basis * root[:, :, np.newaxis]).transpose(2, 1, 0))                         # [u, K, M], times sqrt(w)
    Bw = vr.extended_filter(noise.taps(), ga.lstsq.arc_stages(ARCS, MA, noise.maximum_order), Bt)[0]      # whitened as vectors
    A = reference[4].T                                                                                     # [K M, P], rows component-major
    lbar = reference[5]
    Bk = np.ascontiguousarray(Bw.transpose(1, 2, 0))                                                       # [K, M, u]
    units = arc.explicit_columns(Bk, arc.bounds_of(ARCS, MA), False)
    N, n, lPl = arc.projection(A, lbar, units)
    extra = arc.normals_bounds(A, lbar)
    bounds = tuple(own + more for own, more in zip(reference[3], extra))
    return (N, n, lPl, bounds), A, lbar, units


def test_normals_under_arc_parameters_with_a_general_basis():
    """a parameter's K-vector basis function is whitened as a vector: Bt [u, K, M] is u groups"""
    rng = np.random.default_rng(2964)
    shared = ga.lstsq.arc_basis(ARCS, MA, degree=1)
    frames = gdi.frames(MA, 2965)
    basis = ga.lstsq.frame_basis(shared, frames)                                                           # [M, 3, 6]
    reference, A, lbar, units = _arc_reference(basis, None)
    xyz, w, obs = _acceleration_case()[:3]

    def build(block_points):
        return ga.lstsq.ArcParameters(basis, ARCS, _noise()).from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w, block_points=block_points)
    ne = _check(build(256), reference, 'general basis', 3 * MA - int(build(256).arc_elimination.count))
    assert _same(build(256), ne)
    assert np.abs(A.T @ A - reference[0]).max() > 1e3 * reference[3][0].max()                              # the elimination changes the normals


def test_normals_under_arc_parameters_with_the_component_basis():
    """the shared form is refused under a VectorNoise; component_basis gives it as a general basis, and the eliminated parameters are
    those of the dense system [A~ | B~] (numpy.linalg.lstsq), index c u' + j"""
    shared = ga.lstsq.arc_basis(ARCS, MA, degree=1)                                                        # [M, 2]
    xyz, w, obs = _acceleration_case()[:3]
    with pytest.raises(ValueError, match=r'lstsq\.component_basis\(basis, 3\)'):
        ga.lstsq.ArcParameters(shared, ARCS, _noise()).from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w)
    basis = ga.lstsq.component_basis(shared, 3)
    reference, A, lbar, units = _arc_reference(basis, None)
    model = ga.lstsq.ArcParameters(basis, ARCS, _noise())
    ne = _check(model.from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w, block_points=100), reference, 'component basis',
                3 * MA - int(sum(np.linalg.matrix_rank(unit) for unit in units)))
    x = ne.solve()
    y = ne.arc_elimination.parameters(x)
    assert y.shape == (len(ARCS), 6)
    x_host, y_host = arc.explicit_solution(A, lbar, units)
    deviation = arc.solution_bound(A, reference[0], units)
    err_x = np.linalg.norm(_host(x)[:, 0] - x_host) / np.linalg.norm(x_host)
    err_y = np.linalg.norm(y - np.asarray(y_host)) / np.linalg.norm(y_host)
    print('component basis: x {0:.2e}, y {1:.2e} against the dense system; bound {2:.2e}'.format(err_x, err_y, deviation))
    assert err_x <= deviation and err_y <= deviation
    # the post-fit pass and the leverages run on the same model
    fit = ga.lstsq.PostFit.of_accelerations(x, xyz, obs, 0, NA, di.GM, di.R, weights=w, block_points=100, model=model)
    assert np.allclose(fit.arc_parameters, y, rtol=1e-9, atol=1e-12 * np.abs(y).max())
    unsolved = model.from_accelerations(xyz, obs, 0, NA, di.GM, di.R, weights=w, block_points=100)          # solve() left the factor in ne
    assert abs(fit.arc_square_sums.sum() - unsolved.residual_square_sum(x)) <= 1e-9 * fit.arc_square_sums.sum()
    h = fit.leverages(ne)
    assert h.shape == (MA, 3) and np.all(h > -1e-12) and np.all(h < 1 + 1e-12)
    parameters = ne.right_hand_side.shape[0] + int(ne.arc_elimination.count)
    assert abs(h.sum() - parameters) <= 1e-8 * parameters                                                  # the trace of the hat matrix of [A~ | B~]


# ---- 5: the loop -----------------------------------------------------------------------------------------------------------------------------
LOOP_POINTS, LOOP_ARCS = 20000, [0, 3000, 9000, 14000]


def test_post_fit_vector_noise_whitens_the_residuals():
    """noise of the known VAR(2) as observations of a zero field: the residuals of the zero solution are the noise.  vector_noise(2)
    estimates the model, decorrelate with it whitens the series: its cross-covariances at lags 0 .. 5 are I and 0 within the sampling
    error.  An entry of the sample cross-covariance of white noise over n points has the standard deviation 1 / sqrt(n) (sqrt(2 / n) on
    the diagonal of lag 0), and the estimated model deviates from the true one by the same order: 5 / sqrt(n) is a 5-sigma margin on
    the off-diagonal entries, 3.5 sigma on the diagonal of lag 0."""
    B1, B2, Q = vr.process(3)
    x = vr.simulate([B1, B2], Q, LOOP_ARCS, LOOP_POINTS, 2970)
    xyz = ai.scattered_positions(LOOP_POINTS, 2971)
    model = ga.lstsq.ColouredNoise(_noise(), LOOP_ARCS)
    fit = ga.lstsq.PostFit.of_accelerations(np.zeros(9 - 4), xyz, x, 2, 2, di.GM, di.R, model=model)
    assert np.array_equal(fit.residuals, x) and np.array_equal(fit.arcs, LOOP_ARCS)
    lags = fit.cross_covariance_function(5)
    assert len(lags) == 6 and all(lag.shape == (3, 3) for lag in lags) and np.array_equal(lags[0], lags[0].T)
    scalar = fit.covariance_function(5, per_component=True)
    for c in range(3):
        assert all(abs(lags[k][c, c] - scalar[c][k][0, 0]) <= 4 * U * abs(lags[k][c, c]) for k in range(6))   # the diagonal is covariance_function: the same sums of the kernels, added over the arcs on the host
    truth = vr.covariance_function([B1, B2], Q, 5)
    tolerance = 5.0 / np.sqrt(LOOP_POINTS)
    # the convention, E[x_t x_(t+k)^T]: a sample covariance of a coloured series scatters more than one of white noise, by its
    # correlation time (a few points at a spectral radius of 0.8) and the size of Sigma_0; 5 times the white tolerance, of max|Sigma_0|
    scale = np.abs(truth[0]).max()
    assert max(np.abs(lags[k] - truth[k]).max() for k in range(6)) <= 5 * tolerance * scale
    asymmetry = np.abs(truth[1] - truth[1].T).max()
    assert asymmetry > 20 * tolerance * scale                                                              # the process tells the two conventions apart
    assert np.abs(lags[1] - truth[1].T).max() > 0.5 * asymmetry                                            # and the estimate is not the transpose
    unbiased = fit.cross_covariance_function(5, biased=False)
    pairs = np.array([sum(max(length - k, 0) for length in np.diff(LOOP_ARCS + [LOOP_POINTS])) for k in range(6)])
    assert all(np.allclose(unbiased[k] * pairs[k], lags[k] * pairs[0], rtol=1e-14, atol=0) for k in range(6))
    # positive semi-definite as a block sequence: the block Toeplitz matrix of the biased estimate
    assert np.linalg.eigvalsh(vr.block_toeplitz(lags, 6)).min() >= -1e-12 * np.abs(lags[0]).max()
    for bad in (-1, 129, 2.5):
        with pytest.raises(ValueError, match='maximum_lag must be an integer in 0 .. 128'):
            fit.cross_covariance_function(bad)
        with pytest.raises(ValueError, match='maximum_lag must be an integer in 0 .. 128'):
            fit.vector_noise(bad)
    with pytest.raises(ValueError, match="window must be None, 'bartlett', 'parzen'"):
        fit.vector_noise(2, window='hann')
    estimated = fit.vector_noise(2)
    assert isinstance(estimated, ga.lstsq.VectorNoise) and estimated.dimension == 3 and estimated.maximum_order == 2
    tapered = fit.vector_noise(2, window='bartlett')
    assert np.allclose(tapered.sequence.models[0].white_noise_covariance, lags[0])
    white = ga.lstsq.decorrelate(x, estimated, arcs=LOOP_ARCS)
    seg = _int32(LOOP_ARCS + [LOOP_POINTS])
    sums = _host(ga.engine.segment_cross_lag_products(ga.engine.to_device(np.ascontiguousarray(white.T)), seg, 5)).sum(axis=0)
    worst = 0.0
    for k in range(6):
        deviation = np.abs(sums[k] / LOOP_POINTS - (np.eye(3) if k == 0 else 0.0)).max()
        worst = max(worst, deviation)
    print('whitened series: cross-covariances within {0:.4f} of I and 0; allowed {1:.4f}'.format(worst, tolerance))
    assert worst <= tolerance
    coloured = _host(ga.engine.segment_cross_lag_products(ga.engine.to_device(np.ascontiguousarray(x.T)), seg, 1)).sum(axis=0) / LOOP_POINTS
    assert np.abs(coloured[1]).max() > 10 * tolerance                                                      # the series was coloured
    # the estimated model closes the loop: it is accepted where the first one was
    second = ga.lstsq.PostFit.of_accelerations(np.zeros(5), xyz, x, 2, 2, di.GM, di.R, model=ga.lstsq.ColouredNoise(estimated, LOOP_ARCS))
    assert np.array_equal(second.whitened, white)


def _round_trip(sequence, q):
    """the sequence rebuilt from its own covariance function of lags 0 .. q"""
    return ga.lstsq.AutoregressiveModelSequence.from_covariance_function(sequence.covariance_function(q))


def test_round_trip_through_the_covariance_function(golden):
    """deterministic: sequence.covariance_function(q) -> from_covariance_function -> VectorNoise.taps() reproduces the taps, to the
    accuracy the same round trip reaches for the scalar golden ar5, with a factor of 10 as margin"""
    five = wi.sequence(golden('g27_whitening'), 'ar5', ga.lstsq)
    scalar = ga.lstsq.whitening_taps(five)[0]
    back = ga.lstsq.whitening_taps(_round_trip(five, 5))[0]
    measured = np.abs(back - scalar).max() / np.abs(scalar).max()
    sequence = vr.process_sequence(ga.lstsq, 3)
    taps = ga.lstsq.VectorNoise(sequence).taps()
    rebuilt = ga.lstsq.VectorNoise(_round_trip(sequence, 2)).taps()
    err = np.abs(rebuilt - taps).max() / np.abs(taps).max()
    print('round trip: vector {0:.2e}, scalar ar5 {1:.2e} of max|tap|'.format(err, measured))
    assert measured > 0.0 and err <= 10 * measured
