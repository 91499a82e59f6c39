"""Inputs of the covariance-function noise fixture (tests/golden/make_golden_covariance_noise.py -> g33_covariance_noise.npz) and of
the tests that replay it: one stationary covariance function with a slowly decaying periodic part over a white floor, its Toeplitz
matrices, the inverse Cholesky factor in float64 and in np.longdouble, and restatements of the decorrelation filter in np.longdouble
that the tests compare the long-filter kernel with.  Needs NumPy only."""

import os

import numpy as np

ORDER = 40                                            # of the recorded AR models
LENGTHS = (41, 60)                                    # normal_equations(L) is recorded for these


def covariance(count):
    """c_k = 0.5 * 0.9^k + 0.5 * cos(2 pi k / 50) * 0.99^k + 0.1 [k = 0], k = 0 .. count - 1: positive definite, and the white floor
    of 0.1 bounds the condition number of every Toeplitz matrix of it"""
    k = np.arange(count, dtype=np.float64)
    c = 0.5 * 0.9 ** k + 0.5 * np.cos(2.0 * np.pi * k / 50.0) * 0.99 ** k
    c[0] += 0.1
    return c


def covariance_function(count):
    """the lags as [1, 1] arrays: the argument of AutoregressiveModelSequence.from_covariance_function"""
    return [np.array([[value]]) for value in covariance(count)]


def toeplitz(c, dtype=np.float64):
    index = np.arange(len(c))
    return np.asarray(c, dtype=dtype)[np.abs(index[:, None] - index[None, :])]


def inverse_cholesky(S):
    """W = C^-1 of S = C C^T (lower triangular, positive diagonal) in the dtype of S, np.longdouble included: an outer-product
    Cholesky factorisation and a forward substitution on the identity, row operations vectorised"""
    S = np.array(S)
    n = S.shape[0]
    C = np.zeros_like(S)
    for j in range(n):
        C[j, j] = np.sqrt(S[j, j] - np.dot(C[j, :j], C[j, :j]))
        C[j + 1:, j] = (S[j + 1:, j] - C[j + 1:, :j] @ C[j, :j]) / C[j, j]
    V = np.zeros_like(S)                                      # W^T: the products below then run along rows in memory
    for i in range(n):
        V[:i, i] = -(V[:i, :i] @ C[i, :i]) / C[i, i]
        V[i, i] = 1 / C[i, i]
    return V.T.copy()


def dense_filter(taps, stage):
    """W [L, L] of one channel: row t holds h[n][k] at column t - k, k = 0 .. n, n = min(stage[t], t)"""
    L = len(stage)
    W = np.zeros((L, L), dtype=taps.dtype)
    for t in range(L):
        n = min(int(stage[t]), t)
        W[t, t - n:t + 1] = taps[n, n::-1] if n else taps[0, :1]
    return W


def long_filter(taps, stage, x, channels):
    """y [R, L] = W_c x along the last axis in np.longdouble, row r of channel r % channels, and the magnitudes
    sum_k |h_k| |x[t-k]|; taps [C, q + 1, q + 1], stage already clamped to 0 .. min(q, t).  The error of y is below 2^-11 of
    (n + 2) 2^-53 magnitude (64-bit significands)"""
    x = np.asarray(x, dtype=np.float64)
    y, magnitude = np.zeros(x.shape, dtype=np.longdouble), np.zeros(x.shape)
    for c in range(channels):
        W = dense_filter(taps[c].astype(np.longdouble), stage)
        xc = x[c::channels].astype(np.longdouble)
        y[c::channels] = xc @ W.T
        magnitude[c::channels] = (np.abs(xc) @ np.abs(W).T).astype(np.float64)
    return y, magnitude


def random_taps(channels, q, seed):
    """tap tables [channels, q + 1, q + 1] that do not decay with the lag: uniform in +-1 over sqrt(s + 1) in row s, a positive
    first tap, zero beyond the order of the row"""
    rng = np.random.default_rng(seed)
    taps = np.tril(rng.uniform(-1.0, 1.0, (channels, q + 1, q + 1))) / np.sqrt(1.0 + np.arange(q + 1))[None, :, None]
    taps[:, :, 0] = rng.uniform(0.5, 2.0, (channels, q + 1))
    return taps


def fixture():
    """g33_covariance_noise.npz as a dict"""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g33_covariance_noise.npz')) as f:
        return {key: f[key] for key in f.files}
