"""
Covariance functions of any lag on the GPU: the kernel of shg_segment_lag_products_long (engine.segment_lag_products_long) against
np.longdouble sums within a derived bound, against the kernel of shg_segment_lag_products, bitwise wherever a segment lies and whatever
`lags` is, under a wrong segment table, and PostFit.covariance_lags / covariance_model against the host's computation from the
residuals and with the loop closed once through ColouredNoise.
"""
import functools

import numpy as np
import pytest

import acceleration_inputs as ai
import arc_inputs as arc
import covariance_noise_inputs as ci
import design_inputs as di
import grates_amd as ga
import lags_long_inputs as ll
import whitening_inputs as wi

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CHUNK = 2048                        # engine.segment_lag_long_info()['chunk'], asserted below: parametrize needs it at collection
QUARTER = CHUNK // 4                # the columns of one wave of a chunk's workgroup
TAIL = 512                          # the last chunk of a segment takes up to this many columns more
SENTINEL = -7.25
TABLES = {'short': (0, 1, 4, 300, 700), 'empty': (3, 3, 70, 650),
          'chunks': (5, 5 + CHUNK - 1, 4 + 2 * CHUNK, 5 + 3 * CHUNK, 8 + 5 * CHUNK)}            # chunk - 1, chunk, chunk + 1, 2 chunk + 3 columns
WIDTHS = {'short': 700, 'empty': 700, 'chunks': 8 + 5 * CHUNK + 7}
LAGS = [0, 1, 15, 16, 17, 128, 129, 255, 256, 257, 1023, 4095]


def _host(t):
    return ga.engine.to_host(t) if ga.lstsq._is_tensor(t) else np.asarray(t)


def _int32(values):
    import torch
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=ga.engine.device())


def _padded(values, pad, fill):
    """device tensor with `pad` more columns than `values` [..., M], filled with `fill`; returns the view of the values"""
    import torch
    full = torch.full(values.shape[:-1] + (values.shape[-1] + pad,), fill, dtype=torch.float64, device=ga.engine.device())
    full[..., :values.shape[-1]] = ga.engine.to_device(values)
    return full[..., :values.shape[-1]]


def _long(X, seg, lags, **kwargs):
    return ga.engine.segment_lag_products_long(X, _int32(seg), lags, **kwargs)


def test_info_matches_the_constants_of_this_file():
    info = ga.engine.segment_lag_long_info()
    assert info == {'chunk': CHUNK, 'tile_lags': 256, 'max_lags': 4095}
    assert np.diff(TABLES['chunks']).tolist() == [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]


# ---- 1: the kernel against exact sums ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_case(name):
    """six rows, NaN outside the segments, and the reference at lags = 4095, computed once per table"""
    seg, width = TABLES[name], WIDTHS[name]
    X = np.random.default_rng(3601 + width).standard_normal((6, width))
    covered = np.zeros(width, dtype=bool)
    for first, last in zip(seg[:-1], seg[1:]):
        covered[first:last] = True
    return (np.where(covered, X, np.nan),) + ll.long_lag_products(X, list(seg), 4095)


@pytest.mark.parametrize('name', list(TABLES))
@pytest.mark.parametrize('lags', LAGS)
def test_kernel_against_exact_sums(lags, name):
    """entry-wise within (n_k + 2) u sum |x_t x_(t+k)|: n_k products, fused or rounded, added in any order (the quarters and chunks are
    partial sums of it), and the rounding of the reference; the zeros the kernel multiplies add nothing.  The padding of the rows and
    every column outside the segments is NaN: a read of it would poison a sum.  Entries without a pair are exactly 0."""
    import torch
    seg = TABLES[name]
    X_nan, reference, magnitude, pairs = _exact_case(name)
    reference, magnitude, pairs = reference[:, :, :lags + 1], magnitude[:, :, :lags + 1], pairs[:, :lags + 1]
    view = _padded(X_nan, 4, float('nan'))
    S = _long(view, seg, lags)
    assert tuple(S.shape) == (6, len(seg) - 1, lags + 1) and S.is_contiguous()
    got = _host(S)
    assert np.all(np.isfinite(got))
    bound = ll.bound(magnitude, pairs)
    ratio = np.abs(got - reference) / np.where(bound > 0, bound, 1.0)
    print('lags {0}, table {1}: {2:.4f} of the bound'.format(lags, name, ratio.max()))
    assert np.all(np.abs(got - reference) <= bound)
    assert np.all(got[:, pairs == 0] == 0.0)
    # views and outputs: the column slice above, the dense matrix, a [2, 3, M] view and a given output are bitwise the same
    dense = ga.engine.to_device(X_nan)
    out = torch.full((6, len(seg) - 1, lags + 1), SENTINEL, dtype=torch.float64, device=S.device)
    assert _long(dense, seg, lags, out=out) is out
    assert np.array_equal(_host(out), got)
    assert np.array_equal(_host(_long(dense.reshape(2, 3, -1), seg, lags)), got.reshape(2, 3, len(seg) - 1, lags + 1))
    assert np.array_equal(_host(_long(view, seg, lags)), got)                                      # and repeated calls are bitwise equal


# ---- 2: against the existing kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(TABLES))
@pytest.mark.parametrize('lags', [5, 128])
def test_kernel_against_the_chain_kernel(lags, name):
    """both are within the bound of the exact sums, so they differ by twice the bound at most; equality is not promised"""
    seg = TABLES[name]
    X_nan, _, magnitude, pairs = _exact_case(name)
    view = _padded(X_nan, 4, float('nan'))
    long, chain = _host(_long(view, seg, lags)), _host(ga.engine.segment_lag_products(view, _int32(seg), lags))
    bound = ll.bound(magnitude[:, :, :lags + 1], pairs[:, :lags + 1])
    ratio = np.abs(long - chain) / np.where(bound > 0, bound, 1.0)
    print('lags {0}, table {1}: {2:.4f} of the bound between the kernels, {3} of {4} entries equal'.format(lags, name, ratio.max(),
                                                                                                         int((long == chain).sum()), long.size))
    assert np.all(np.abs(long - chain) <= 2 * bound)


# ---- 3: locality, bitwise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('length', [1, 3, 4, 5, 15, 16, 17, 255, 256, 257, QUARTER - 1, QUARTER, QUARTER + 1, CHUNK - 1, CHUNK, CHUNK + 1,
                                    CHUNK + TAIL, CHUNK + TAIL + 1, 2 * CHUNK + 3])
def test_a_segment_gives_the_same_bits_wherever_it_lies(length):
    """a K-step has 4 columns, the A operand 16 rows, a tile 256 lags, a wave a quarter of 512 columns, a work item a chunk of 2048, and
    the last chunk of a segment up to 512 more: those and their neighbours are the seams.  The data of one segment at offsets 0, 1, 63
    and 517 of a longer row, alone and between other segments, in a matrix of 1 and of 7 rows, for lags = 4095 and 300; and lag k of a
    call with lags = 4095 is lag k of a call with lags = k"""
    rng = np.random.default_rng(3620 + length)
    x = rng.standard_normal(length)
    alone = ga.engine.to_device(x[None])
    references = {lags: _host(_long(alone, [0, length], lags)) for lags in (4095, 300)}
    assert references[4095].shape == (1, 1, 4096) and np.array_equal(references[4095][..., :301], references[300])
    for k in (0, 1, 16, 255, 256, 1024):
        assert np.array_equal(_host(_long(alone, [0, length], k))[..., k], references[4095][..., k])
    assert np.all(references[4095][0, 0, min(length, 4096):] == 0.0)
    for offset in (0, 1, 63, 517):
        width = offset + length + 130
        row = rng.standard_normal(width)
        row[offset:offset + length] = x
        X7 = rng.standard_normal((7, width))
        X7[3], X7[6] = row, row
        one, seven = ga.engine.to_device(row[None]), ga.engine.to_device(X7)
        single, between = [offset, offset + length], [0, offset, offset + length, width - 7, width]
        for lags, reference in references.items():
            assert np.array_equal(_host(_long(one, single, lags)), reference)
            assert np.array_equal(_host(_long(one, between, lags))[:, 1:2], reference)
            many = _host(_long(seven, between, lags))
            assert np.array_equal(many[3:4, 1:2], reference) and np.array_equal(many[6:7, 1:2], reference)
            assert np.array_equal(_host(_long(seven, single, lags))[[3, 6]], np.concatenate((reference, reference)))


# ---- 4: clamping -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lags', [0, 300, 4095])
@pytest.mark.parametrize('width, wrong', [(700, (-5, 5, 3, 703)), (CHUNK + 700, (-5, 40, 20, CHUNK + 100, 90, CHUNK + 703))])
def test_segment_table_is_clamped(width, wrong, lags):
    """a wrong table gives wrong numbers, not a fault: entries are clamped to 0 .. M and made non-decreasing.  With four columns of
    padding even an unclamped read of the table's M + 3 would stay inside the allocation, and at 1e300 it would show"""
    rows = 6
    X = np.random.default_rng(3630 + width).standard_normal((rows, width))
    view = _padded(X, 4, 1e300)
    right = arc.clamped(wrong, width)
    assert right[0] == 0 and right[-1] == width and np.all(np.diff(right) >= 0) and np.any(np.diff(wrong) < 0)
    got, expected = _long(view, wrong, lags), _long(view, right, lags)
    assert bool((got == expected).all()) and bool(got.isfinite().all())
    empty = np.flatnonzero(np.diff(right) == 0)
    assert empty.size and bool((got[:, empty] == 0).all())
    reference, magnitude, pairs = ll.long_lag_products(X, right, lags)
    assert np.all(np.abs(_host(got) - reference) <= ll.bound(magnitude, pairs))
    extreme = _long(view, [2 ** 31 - 1, -2 ** 31, 5, 2], lags)
    assert bool((extreme == 0).all())                                                              # everything lies behind the first entry


# ---- 5: PostFit ----------------------------------------------------------------------------------------------------------------------------
N, MIN_DEGREE, M = 8, 2, 1650
P = (N + 1) ** 2 - MIN_DEGREE ** 2
ARCS = [0, 1, 4, 300, 900]                                                                        # arcs of 1, 3, 296, 600 and 750 points


@functools.lru_cache(maxsize=None)
def _fit():
    rng = np.random.default_rng(3640)
    xyz = ai.scattered_positions(M, 3641)
    w, obs = rng.uniform(0.25, 4.0, M), rng.standard_normal((M, 3)) * 1e-3
    model = ga.lstsq.ColouredNoise(wi.sequence(wi.fixture(), 'ar5', ga.lstsq), ARCS)
    ne = model.from_accelerations(xyz, obs, MIN_DEGREE, N, di.GM, di.R, weights=w, block_points=512)
    x = _host(ne.solve())[:, 0]
    return ga.lstsq.PostFit.of_accelerations(x, xyz, obs, MIN_DEGREE, N, di.GM, di.R, weights=w, block_points=512, model=model)


@pytest.mark.parametrize('q', [5, 128])
def test_covariance_lags_is_covariance_function_up_to_lag_128(q):
    fit = _fit()
    for biased in (True, False):
        assert np.array_equal(fit.covariance_lags(q, biased=biased), np.array(fit.covariance_function(q, biased=biased)).ravel())
        each = fit.covariance_lags(q, per_component=True, biased=biased)
        assert each.shape == (3, q + 1)
        assert np.array_equal(each, np.array(fit.covariance_function(q, per_component=True, biased=biased)).reshape(3, q + 1))


@functools.lru_cache(maxsize=None)
def _host_covariance(biased):
    return ll.covariance(_host(_fit().residuals), ARCS, 700, biased)


@pytest.mark.parametrize('q', [129, 700])
@pytest.mark.parametrize('biased', [True, False])
def test_covariance_lags_against_the_host(biased, q):
    """the host's np.longdouble sums over fit.residuals, within the bound of the kernel summed over the arcs and divided by the divisor"""
    fit = _fit()
    c, bound, pooled, pooled_bound = (value[..., :q + 1] for value in _host_covariance(biased))
    got, each = fit.covariance_lags(q, biased=biased), fit.covariance_lags(q, per_component=True, biased=biased)
    assert isinstance(got, np.ndarray) and got.shape == (q + 1,) and isinstance(each, np.ndarray) and each.shape == (3, q + 1)
    ratio, each_ratio = np.abs(got - pooled) / pooled_bound, np.abs(each - c) / bound
    print('q {0}, biased {1}: pooled {2:.4f}, per component {3:.4f} of their bounds'.format(q, biased, ratio.max(), each_ratio.max()))
    assert ratio.max() <= 1 and each_ratio.max() <= 1
    assert np.array_equal(got[:130], fit.covariance_lags(129, biased=biased))                     # lag k does not depend on maximum_lag


def test_unbiased_beyond_the_longest_arc_raises():
    fit = _fit()
    assert fit.covariance_lags(749, biased=False).shape == (750,)
    with pytest.raises(ValueError, match='no arc is longer than 750 points: no pair at lag 750'):
        fit.covariance_lags(750, biased=False)
    assert fit.covariance_lags(4095).shape == (4096,) and np.all(fit.covariance_lags(4095)[750:] == 0.0)


def test_covariance_lags_under_temporal_parameters_with_shuffled_epochs():
    """the pass sorts the points by their window and gives the residuals back in the order given: the lags are those of that order"""
    rng = np.random.default_rng(3650)
    xyz, obs = ai.scattered_positions(M, 3651), rng.standard_normal((M, 3)) * 1e-3
    epochs = rng.permutation(np.linspace(0.02, 2.98, M))
    temporal = ga.lstsq.TemporalParameters.linear(np.array([0.0, 1.0, 2.0, 3.0]), epochs)
    fit = temporal.of_accelerations(rng.standard_normal(4 * P) * 1e-6, xyz, obs, MIN_DEGREE, N, di.GM, di.R, block_points=512)
    assert np.array_equal(fit.arcs, [0])
    c, bound, pooled, pooled_bound = ll.covariance(_host(fit.residuals), [0], 700, True)
    got, each = fit.covariance_lags(700), fit.covariance_lags(700, per_component=True)
    print('temporal: pooled {0:.4f}, per component {1:.4f} of their bounds'.format((np.abs(got - pooled) / pooled_bound).max(),
                                                                                  (np.abs(each - c) / bound).max()))
    assert np.all(np.abs(got - pooled) <= pooled_bound) and np.all(np.abs(each - c) <= bound)


# ---- 6: the loop closed once ---------------------------------------------------------------------------------------------------------------
def _arc_filters(c, arcs, count, from_taps):
    """W_a of every arc under the covariance function c_0 .. c_q, as tests/test_gpu_covariance_noise.py builds them: inv(cholesky(Toeplitz))
    of the first min(n_a, q + 1) points and the last of these rows shifted along; from_taps: the same from CovarianceFunction.taps()"""
    q = len(c) - 1
    head = ci.dense_filter(ga.lstsq.CovarianceFunction(c).taps(), np.arange(q + 1)) if from_taps else np.linalg.inv(np.linalg.cholesky(ci.toeplitz(c)))
    filters = []
    for start, end in zip(arcs, list(arcs[1:]) + [count]):
        n = end - start
        W, m = np.zeros((n, n)), min(n, q + 1)
        W[:m, :m] = head[:m, :m]
        for t in range(m, n):
            W[t, t - q:t + 1] = head[q]
        filters.append(W)
    return filters


def _normals(c, arcs, At, l, from_taps):
    A, b = np.empty_like(At), np.empty_like(l)
    for W, start in zip(_arc_filters(c, arcs, At.shape[2], from_taps), arcs):
        A[..., start:start + len(W)] = At[..., start:start + len(W)] @ W.T
        b[..., start:start + len(W)] = l[..., start:start + len(W)] @ W.T
    A, b = A.reshape(At.shape[0], -1), b.ravel()
    return A @ A.T, A @ b, float(b @ b)


def test_the_loop_closed_with_a_long_covariance_model():
    """noise with a known covariance function of 300 lags -> solve -> fit.covariance_model(300, 'parzen') -> ColouredNoise -> normals,
    against NumPy normals of W_a A_a with W_a = inv(cholesky(Toeplitz(model.covariance_function))).  Tolerance: the rule of
    tests/test_gpu_covariance_noise.py, 2 K M u plus ten times the difference of the two host routes, floor 1e-12.
    The estimate against the truth: the scatter is the deviation of the host's own biased estimate on the same noise sample (NumPy,
    before any fit); the device's estimate from the residuals of a fit with P = 77 of 4950 observations lies within twice that."""
    count, K, q, arcs = 1650, 3, 300, [0, 750]
    noise, truth = ll.coloured_noise(count, K, q + 1, 3660)
    xyz, obs = ai.scattered_positions(count, 3661), noise * 1e-3
    white = ga.lstsq.ColouredNoise(ga.lstsq.CovarianceFunction(np.array([1.0])), arcs)
    x = _host(white.from_accelerations(xyz, obs, MIN_DEGREE, N, di.GM, di.R, block_points=512).solve())[:, 0]
    fit = ga.lstsq.PostFit.of_accelerations(x, xyz, obs, MIN_DEGREE, N, di.GM, di.R, block_points=512, model=white)
    estimate = fit.covariance_lags(q) * 1e6
    own = ll.covariance(noise, arcs, q, True)[2]
    scatter, deviation = np.abs(own - truth).max(), np.abs(estimate - truth).max()
    print('estimate: the host on the sample {0:.3e}, the device on the residuals {1:.3e} off the true function (c_0 = 1)'.format(scatter, deviation))
    assert deviation <= 2 * scatter
    model = fit.covariance_model(q, window='parzen')
    assert isinstance(model, ga.lstsq.CovarianceFunction) and model.maximum_order == q
    assert np.array_equal(model.covariance_function, fit.covariance_lags(q) * ga.lstsq.lag_window('parzen', q))
    each = fit.covariance_model(q, per_component=True, window='bartlett')
    assert len(each) == K and all(isinstance(function, ga.lstsq.CovarianceFunction) for function in each)
    c = model.covariance_function
    At, l = _host(ga.engine.acceleration_design(N, xyz, di.GM, di.R, MIN_DEGREE)), np.ascontiguousarray(obs.T)
    (N1, n1, l1), (N2, n2, l2) = _normals(c, arcs, At, l, False), _normals(c, arcs, At, l, True)
    d = np.sqrt(np.diag(N1))
    scale_N, scale_n = np.outer(d, d), d * np.sqrt(l1)
    routes_differ = max(float((np.abs(N1 - N2) / scale_N).max()), float((np.abs(n1 - n2) / scale_n).max()), abs(l1 - l2) / l1)
    slack = 2 * K * count * U + max(10 * routes_differ, 1e-12)
    ne = ga.lstsq.ColouredNoise(model, arcs).from_accelerations(xyz, obs, MIN_DEGREE, N, di.GM, di.R, block_points=512)
    got_N, got_n, got_l, got_count = ne.to_array()
    print('normals under the estimated model: N {0:.3f}, n {1:.3f}, lPl {2:.3f} of the tolerance {3:.2e} (host routes {4:.2e})'.format(
        float((np.abs(got_N - N1) / scale_N).max()) / slack, float((np.abs(got_n[:, 0] - n1) / scale_n).max()) / slack, abs(got_l - l1) / l1 / slack,
        slack, routes_differ))
    assert got_count == K * count
    assert np.all(np.abs(got_N - N1) <= slack * scale_N) and np.all(np.abs(got_n[:, 0] - n1) <= slack * scale_n) and abs(got_l - l1) <= slack * l1
    again = _host(ga.lstsq.ColouredNoise(each, arcs).from_accelerations(xyz, obs, MIN_DEGREE, N, di.GM, di.R, block_points=512).solve())
    assert again.shape == (P, 1) and np.all(np.isfinite(again))
