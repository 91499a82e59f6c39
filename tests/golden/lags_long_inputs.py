"""Host references of the tests of shg_segment_lag_products_long and of PostFit.covariance_lags / covariance_model: the lagged
products of segments in np.longdouble with their magnitudes and pair counts, the covariance function from them, and coloured noise with a
known covariance function.  Needs NumPy only."""

import numpy as np

U = 2.0 ** -53


def long_lag_products(X, seg, lags):
    """(S, magnitude [rows, nseg, lags + 1], pairs [nseg, lags + 1]) of the table seg as given (non-decreasing, inside the rows):
    S[r, s, k] = sum_t x_t x_(t+k) over the pairs of segment s as np.longdouble dot products, rounded to double at the end, magnitude the
    same sum of |x_t x_(t+k)|, pairs n_k = max(length - k, 0).  A product of two doubles is rounded to 64 bits and summed pairwise in
    64 bits: 2^-11 of a double's rounding per operation."""
    rows, nseg = X.shape[0], len(seg) - 1
    S, magnitude = np.zeros((rows, nseg, lags + 1)), np.zeros((rows, nseg, lags + 1))
    pairs = np.zeros((nseg, lags + 1), dtype=np.int64)
    for s in range(nseg):
        first, last = int(seg[s]), max(int(seg[s + 1]), int(seg[s]))
        length = last - first
        pairs[s] = np.maximum(length - np.arange(lags + 1), 0)
        x = X[:, first:last].astype(np.longdouble)
        for k in range(min(lags + 1, length)):
            products = x[:, :length - k] * x[:, k:]
            S[:, s, k] = products.sum(axis=1)
            magnitude[:, s, k] = np.abs(products).sum(axis=1)
    return S, magnitude, pairs


def bound(magnitude, pairs):
    """(n_k + 2) 2^-53 sum |x_t x_(t+k)|: n_k products, rounded or fused, added in any order, partial sums included, and the rounding of
    the reference"""
    return (pairs[None] + 2) * U * magnitude


def covariance(residuals, arcs, maximum_lag, biased):
    """(c [K, q + 1], bound [K, q + 1], pooled c [q + 1], pooled bound [q + 1]) of the estimator of PostFit.covariance_lags on
    residuals [M, K]: the sums of long_lag_products and their bounds, summed over the arcs and divided by the divisor d_k = sum_a len_a
    (biased) or sum_a max(len_a - k, 0)"""
    M, K = residuals.shape
    seg = np.append(np.asarray(arcs, dtype=np.int64), M)
    S, magnitude, pairs = long_lag_products(np.ascontiguousarray(residuals.T), seg, maximum_lag)
    d = pairs.sum(axis=0).astype(np.float64)
    if biased:
        d = np.full(maximum_lag + 1, d[0])
    limit = bound(magnitude, pairs).sum(axis=1)
    return S.sum(axis=1) / d, limit / d, S.sum(axis=(0, 1)) / (K * d), limit.sum(axis=0) / (K * d)


def coloured_noise(count, components, length, seed):
    """(noise [count, components], c [length]): white noise filtered with a smooth one-sided window of `length` taps (a moving average),
    whose covariance function c_k = sum_i g_i g_(i+k) is known exactly and is zero from lag `length` on; c_0 = 1"""
    rng = np.random.default_rng(seed)
    g = np.exp(-np.arange(length) / (length / 4.0)) * np.cos(np.arange(length) * (2.0 * np.pi / 93.0)) + 0.3 * (np.arange(length) == 0)
    g /= np.sqrt(g @ g)
    white = rng.standard_normal((count + length - 1, components))
    noise = np.stack([np.convolve(white[:, k], g, mode='valid') for k in range(components)], axis=1)
    c = np.array([g[:length - k] @ g[k:] for k in range(length)])
    return noise, c
