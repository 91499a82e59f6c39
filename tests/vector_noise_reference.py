"""
NumPy helpers of the vector-noise tests (tests/test_vector_noise_cpu.py, tests/test_gpu_vector_noise.py): known stable VAR processes
with non-symmetric coefficients, their covariance functions Sigma_k = E[x_t x_(t+k)^T] from the Lyapunov equation of the companion
form, the block Yule-Walker systems solved in NumPy (AutoregressiveModelSequence.from_covariance_function needs the device), dense
filters, an extended-precision evaluation of the filter, and the exact cross-lag sums with their chain bound
(tests/test_gpu_lag_body.py too).  No GPU, no file.
"""
import numpy as np

U = 2.0 ** -53


def process(K):
    """(B_1, B_2, Q) of a stable VAR(2) x_t = B_1 x_(t-1) + B_2 x_(t-2) + w_t, cov(w) = Q, of dimension K with non-symmetric
    coefficients: seeded, scaled to a spectral radius of 0.8 of the companion matrix"""
    rng = np.random.default_rng(2900 + K)
    B1, B2 = rng.uniform(-1.0, 1.0, (K, K)), 0.5 * rng.uniform(-1.0, 1.0, (K, K))
    radius = np.abs(np.linalg.eigvals(companion([B1, B2]))).max()
    s = 0.8 / radius                                         # x_t -> s^t x_t scales B_k by s^k and the radius by s
    G = rng.standard_normal((K, K))
    return s * B1, s * s * B2, G @ G.T / K + 0.5 * np.eye(K)


def companion(B):
    K, p = B[0].shape[0], len(B)
    A = np.zeros((K * p, K * p))
    A[:K] = np.hstack(B)
    A[K:, :-K] = np.eye(K * (p - 1))
    return A


def covariance_function(B, Q, lags):
    """[Sigma_0 .. Sigma_lags], Sigma_k = E[x_t x_(t+k)^T] of the stationary process: P = A P A^T + Q_c for the companion form gives
    Gamma(h) = E[x_t x_(t-h)^T] for h < p, the recursion Gamma(h) = sum_k B_k Gamma(h - k) the rest; Sigma_k = Gamma(k)^T"""
    K, p = Q.shape[0], len(B)
    A = companion(B)
    Qc = np.zeros_like(A)
    Qc[:K, :K] = Q
    n = A.shape[0]
    P = np.linalg.solve(np.eye(n * n) - np.kron(A, A), Qc.ravel()).reshape(n, n)
    gamma = {h: P[:K, h * K:(h + 1) * K] for h in range(p)}
    for h in range(1, p):
        gamma[-h] = gamma[h].T
    for h in range(p, lags + 1):
        gamma[h] = sum(B[k - 1] @ gamma[h - k] for k in range(1, p + 1))
    return [np.ascontiguousarray(gamma[k].T) for k in range(lags + 1)]


def yule_walker(Sigma, p):
    """(B_1 .. B_p, Q) of the VAR(p) that matches Sigma_0 .. Sigma_p: sum_k Sigma_(r+1-k) B_k^T = Sigma_(r+1), r = 0 .. p - 1, with
    Sigma_(-k) = Sigma_k^T, and Q = Sigma_0 - sum_k B_k Sigma_k"""
    K = Sigma[0].shape[0]
    if p == 0:
        return [], Sigma[0].copy()
    lag = lambda k: Sigma[k] if k >= 0 else Sigma[-k].T
    T = np.block([[lag(r - c) for c in range(p)] for r in range(p)])
    X = np.linalg.solve(T, np.vstack([Sigma[r + 1] for r in range(p)]))
    B = [X[k * K:(k + 1) * K].T for k in range(p)]
    Q = Sigma[0] - sum(B[k] @ Sigma[k + 1] for k in range(p))
    return B, 0.5 * (Q + Q.T)


def sequence(lstsq, Sigma, q):
    """the AutoregressiveModelSequence of orders 0 .. q of the covariance function Sigma, through the constructors"""
    return lstsq.AutoregressiveModelSequence([lstsq.AutoregressiveModel(*yule_walker(Sigma, s)) for s in range(q + 1)])


def process_sequence(lstsq, K, q=2):
    B1, B2, Q = process(K)
    return sequence(lstsq, covariance_function([B1, B2], Q, q), q)


def synthetic_sequence(lstsq, K, q, seed):
    """orders 0 .. q with seeded coefficients (decaying with the lag) and covariances: taps for the kernel tests, not one process"""
    rng = np.random.default_rng(seed)
    models = []
    for s in range(q + 1):
        G = rng.standard_normal((K, K))
        models.append(lstsq.AutoregressiveModel([rng.uniform(-0.9, 0.9, (K, K)) / (1.0 + k) / K for k in range(s)], G @ G.T / K + 0.25 * np.eye(K)))
    return lstsq.AutoregressiveModelSequence(models)


def block_toeplitz(Sigma, L):
    """Sigma_L [L K, L K], block (i, j) = Sigma_(j-i) for j >= i and its transpose below: the covariance of (x_0, ..., x_(L-1))"""
    return np.block([[Sigma[j - i] if j >= i else Sigma[i - j].T for j in range(L)] for i in range(L)])


def dense_filter(taps, stage):
    """W [L K, L K], point-major (index t K + c): block (t, t - k) = H[stage[t]][k], k = 0 .. stage[t]"""
    L, K = len(stage), taps.shape[2]
    W = np.zeros((L * K, L * K))
    for t in range(L):
        n = int(stage[t])
        for k in range(n + 1):
            W[t * K:(t + 1) * K, (t - k) * K:(t - k + 1) * K] = taps[n, k]
    return W


def clamp(stage, q):
    """n[t] = min(max(stage[t], 0), q, t), as the kernel reads a stage table"""
    stage = np.asarray(stage, dtype=np.int64)
    return np.minimum(np.minimum(np.maximum(stage, 0), q), np.arange(stage.size))


def extended_filter(taps, stage, X, keep=False):
    """(y, magnitude, n) for X [groups, K, M]: y = sum_k H[n][k] x[t-k] in numpy.longdouble (64-bit significand on x86: every product of
    two doubles and the K (n + 1) additions round at 2^-64, 2^-11 of the bound below), rounded to float64 once; magnitude =
    sum_k sum_c' |H| |x|, to which the rounding errors of a float64 evaluation are proportional; n [M] the lags in use.  keep: y and
    magnitude stay numpy.longdouble"""
    q = taps.shape[0] - 1
    n = clamp(stage, q)
    H, Xl = taps.astype(np.longdouble), X.astype(np.longdouble)
    y, magnitude = np.zeros(X.shape, dtype=np.longdouble), np.zeros(X.shape, dtype=np.longdouble)
    for order in np.unique(n):
        columns = np.flatnonzero(n == order)
        for k in range(int(order) + 1):
            y[:, :, columns] += np.einsum('cd,gdt->gct', H[order, k], Xl[:, :, columns - k])
            magnitude[:, :, columns] += np.einsum('cd,gdt->gct', np.abs(H[order, k]), np.abs(Xl[:, :, columns - k]))
    if keep:
        return y, magnitude, n
    return y.astype(np.float64), magnitude.astype(np.float64), n


def filter_bound(K, n, magnitude):
    """(K (n + 1) + 1) u sum |H| |x|: K (n + 1) roundings of the kernel's chain (one product, K (n + 1) - 1 FMAs) and one unit for the
    reference, which is rounded once"""
    return (K * (n[np.newaxis, np.newaxis, :] + 1) + 1) * U * magnitude


def simulate(B, Q, arcs, count, seed, burn=200):
    """x [count, K] of the VAR process, every arc an independent stationary stretch (a burn-in of `burn` points is dropped)"""
    rng = np.random.default_rng(seed)
    K, p = Q.shape[0], len(B)
    C = np.linalg.cholesky(Q)
    bounds = list(arcs) + [count]
    out = np.zeros((count, K))
    for a in range(len(arcs)):
        length = bounds[a + 1] - bounds[a]
        w = rng.standard_normal((length + burn, K)) @ C.T
        x = np.zeros((length + burn, K))
        for t in range(length + burn):
            x[t] = w[t] + sum(B[k] @ x[t - k - 1] for k in range(p) if t - k - 1 >= 0)
        out[bounds[a]:bounds[a + 1]] = x[burn:]
    return out


def exact_cross(X, seg, lags):
    """(S [nseg, lags + 1, K, K], magnitude, pairs [nseg, lags + 1]) in numpy.longdouble, rounded once: its own error is 2^-11 of u"""
    K = X.shape[0]
    Xl = X.astype(np.longdouble)
    nseg = len(seg) - 1
    S, magnitude = np.zeros((nseg, lags + 1, K, K)), np.zeros((nseg, lags + 1, K, K))
    pairs = np.zeros((nseg, lags + 1), dtype=np.int64)
    for s in range(nseg):
        a, b = seg[s], seg[s + 1]
        for k in range(lags + 1):
            if b - a > k:
                left, right = Xl[:, a:b - k], Xl[:, a + k:b]
                S[s, k] = (left @ right.T).astype(np.float64)
                magnitude[s, k] = (np.abs(left) @ np.abs(right).T).astype(np.float64)
                pairs[s, k] = b - a - k
    return S, magnitude, pairs


def cross_bound(magnitude, pairs):
    """(ceil(pairs / 64) + 6 + 1) u sum |x y|: the FMAs of the longest of the 64 chains, the six additions of the butterfly and one unit
    for the reference"""
    return ((pairs + 63) // 64 + 7)[:, :, None, None] * U * magnitude
