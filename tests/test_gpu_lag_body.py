"""
GPU tests of the lag body that shg_segment_lag_products and shg_segment_cross_lag_products share (lag_tile of csrc/lags.hip): the
cross call at the smallest shape whose tiles meet every condition that lag_tile is specialised on.  K = 2 rows; lags 6 (G = 2, wave 3
holds one lag of two), 7 (G = 2, every wave full) and 128 (G = 33, wave 3 holds 30 of 33); three segments: one whose first tile of
1024 columns has all its partners inside the segment, followed by a tile of lags + 1 columns; one of exactly one tile that ends with
its segment; one of a single point.  Three columns of NaN behind the last segment belong to none.
"""
import functools

import numpy as np
import pytest

import grates_amd as ga
import vector_noise_reference as vr

pytestmark = pytest.mark.gpu

K = 2
LAGS = [6, 7, 128]


def _segments(lags):
    return [0, 1024 + lags + 1, 2048 + lags + 1, 2048 + lags + 2]


def _int32(values):
    import torch
    return torch.from_numpy(np.asarray(values, dtype=np.int32)).to(ga.engine.device())


def _with_nan(rows):
    """the rows with three columns of NaN behind them, on the device"""
    return ga.engine.to_device(np.concatenate((rows, np.full((rows.shape[0], 3), np.nan)), axis=1))


@functools.lru_cache(maxsize=None)
def _rows(lags):
    return np.random.default_rng(3100 + lags).standard_normal((K, _segments(lags)[-1]))


@pytest.mark.parametrize('lags', LAGS)
def test_identical_rows_are_bitwise_the_scalar_sums(lags):
    """every pair (c, c') of two equal rows runs the chain of the scalar call on that row: all four entries, without a tolerance"""
    seg = _int32(_segments(lags))
    row = _rows(lags)[:1]
    S = ga.engine.to_host(ga.engine.segment_cross_lag_products(_with_nan(np.repeat(row, K, axis=0)), seg, lags))
    scalar = ga.engine.to_host(ga.engine.segment_lag_products(_with_nan(row), seg, lags))[0]                # [nseg, lags + 1]
    assert S.shape == (3, lags + 1, K, K) and np.all(np.isfinite(scalar))
    for c in range(K):
        for cc in range(K):
            assert np.array_equal(S[:, :, c, cc], scalar), (c, cc)


@pytest.mark.parametrize('lags', LAGS)
def test_independent_rows(lags):
    """the diagonal bitwise the scalar call, the rest within the chain bound of the sums in numpy.longdouble, +0.0 where there is no
    pair, and the same bits in a second call"""
    segments = _segments(lags)
    seg, X = _int32(segments), _rows(lags)
    X_d = _with_nan(X)
    S = ga.engine.to_host(ga.engine.segment_cross_lag_products(X_d, seg, lags))
    scalar = ga.engine.to_host(ga.engine.segment_lag_products(X_d, seg, lags))                              # [K, nseg, lags + 1]
    for c in range(K):
        assert np.array_equal(S[:, :, c, c], scalar[c]), c
    reference, magnitude, pairs = vr.exact_cross(X, segments, lags)
    bound = vr.cross_bound(magnitude, pairs)
    ratio = np.abs(S - reference) / np.where(bound > 0, bound, 1.0)
    print('lags {0}: {1:.3f} of the chain bound'.format(lags, ratio.max()))
    assert np.all(np.abs(S - reference) <= bound)
    assert np.all(pairs[:2] > 0) and np.array_equal(pairs[2] > 0, np.arange(lags + 1) == 0)               # the single point pairs with itself only
    assert not np.any(S[pairs == 0]) and not np.any(np.signbit(S[pairs == 0]))                             # no pair: exactly +0.0
    assert np.array_equal(ga.engine.to_host(ga.engine.segment_cross_lag_products(X_d, seg, lags)), S)
