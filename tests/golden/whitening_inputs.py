"""Inputs of the whitening fixture (tests/golden/make_golden_whitening.py -> g27_whitening.npz) and of the tests that replay it: two
scalar AR processes given by their poles, their covariance functions by the Yule-Walker equations, and restatements of the
decorrelation filter (the dense W of an arc structure in float64, W x in exact rational arithmetic) that the tests compare the kernel
with.  Needs NumPy only."""

import os

import numpy as np

# name: (poles of the AR polynomial, all inside the unit circle: the process is stable; variance of its white noise)
PROCESSES = {
    'ar2': ((0.8 * np.exp(0.6j), 0.8 * np.exp(-0.6j)), 2.5e-3),
    'ar5': ((0.9, 0.7 * np.exp(0.8j), 0.7 * np.exp(-0.8j), 0.5 * np.exp(2.0j), 0.5 * np.exp(-2.0j)), 4.0),
}
LENGTHS = 12                                          # normal_equations(L) is recorded for L = p + 1 and L = LENGTHS


def coefficients(name):
    """phi_1 .. phi_p of x_t = sum_k phi_k x_(t-k) + w_t: prod (1 - pole z^-1) = 1 - sum_k phi_k z^-k"""
    return -np.real(np.poly(PROCESSES[name][0]))[1:]


def order(name):
    return len(PROCESSES[name][0])


def covariance(name, count):
    """gamma_0 .. gamma_(count - 1) of the process: lags 0 .. p from the Yule-Walker equations gamma_k = sum_j phi_j gamma_|k-j| +
    sigma^2 [k = 0] as one linear system, the lags beyond by the recursion"""
    phi, sigma2 = coefficients(name), PROCESSES[name][1]
    p = len(phi)
    system, rhs = np.eye(p + 1), np.zeros(p + 1)
    rhs[0] = sigma2
    for k in range(p + 1):
        for j in range(1, p + 1):
            system[k, abs(k - j)] -= phi[j - 1]
    gamma = list(np.linalg.solve(system, rhs))
    while len(gamma) < count:
        gamma.append(sum(phi[j - 1] * gamma[len(gamma) - j] for j in range(1, p + 1)))
    return np.array(gamma[:count])


def covariance_function(name):
    """lags 0 .. p as [1, 1] arrays: the argument of AutoregressiveModelSequence.from_covariance_function"""
    return [np.array([[value]]) for value in covariance(name, order(name) + 1)]


def toeplitz(name, L):
    gamma = covariance(name, L)
    index = np.arange(L)
    return gamma[np.abs(index[:, None] - index[None, :])]


def dense_filter(taps, stage):
    """W [L, L] of one channel: row t holds h[stage[t]][k] at column t - k, k = 0 .. stage[t]"""
    L = len(stage)
    W = np.zeros((L, L))
    for t in range(L):
        for k in range(int(stage[t]) + 1):
            W[t, t - k] = taps[int(stage[t]), k]
    return W


def exact_filter(taps, stage, x):
    """y [R, L] = W x along the last axis in exact rational arithmetic, rounded to float64 once (half a unit in the last place of
    the entry), and the magnitudes sum_k |h_k| |x[t-k]| that the rounding errors of a float64 evaluation are proportional to.
    taps [q + 1, q + 1] of one channel, or [R, q + 1, q + 1] with those of every row."""
    from fractions import Fraction
    x = np.asarray(x, dtype=np.float64)
    y, magnitude = np.zeros_like(x), np.zeros_like(x)
    for r in range(x.shape[0]):
        h = [[Fraction(value) for value in row] for row in (taps if taps.ndim == 2 else taps[r])]
        xr = [Fraction(value) for value in x[r]]
        for t in range(x.shape[1]):
            terms = [h[int(stage[t])][k] * xr[t - k] for k in range(int(stage[t]) + 1)]
            y[r, t], magnitude[r, t] = float(sum(terms)), float(sum(abs(term) for term in terms))
    return y, magnitude


def fixture():
    """g27_whitening.npz as a dict (for the cached cases of the GPU tests, which cannot take a pytest fixture)"""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g27_whitening.npz')) as f:
        return {key: f[key] for key in f.files}


def sequence(data, name, lstsq):
    """the AutoregressiveModelSequence of `lstsq` (grates_amd.lstsq) from the recorded coefficients and variances of process `name`"""
    models = [lstsq.AutoregressiveModel([np.array([[value]]) for value in data[name + '_coefficients'][s, :s]], np.array([[data[name + '_Q'][s]]]))
              for s in range(order(name) + 1)]
    return lstsq.AutoregressiveModelSequence(models)


def synthetic_sequence(lstsq, q, seed):
    """an AutoregressiveModelSequence of orders 0 .. q with seeded coefficients (decaying with the lag) and variances: taps for the
    kernel tests, not the models of one process"""
    rng = np.random.default_rng(seed)
    models = [lstsq.AutoregressiveModel([np.array([[value]]) for value in rng.uniform(-0.9, 0.9, s) / (1.0 + np.arange(s))],
                                        np.array([[rng.uniform(0.25, 4.0)]])) for s in range(q + 1)]
    return lstsq.AutoregressiveModelSequence(models)
