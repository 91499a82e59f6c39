"""
Host formulations for the tests of the observation leverages and the Huber reweighting (tests/test_leverage_cpu.py,
tests/test_gpu_leverage.py): the np.longdouble oracle of shg_leverages with the magnitude of its rounding bound, hat diagonals by the
normals route and by a QR of the full model, the planted-outlier problems, and an iteratively reweighted least squares in NumPy.
"""
import numpy as np

GM, R = 3.9860044150e+14, 6.3781363000e+06
RADIUS = 6.8e6


def exact_leverages(Ui, X):
    """(out [cols], magnitude [cols]): out[j] = sum_p (sum_{q <= p} Ui[q, p] X[q, j])^2 in np.longdouble, rounded once, and
    magnitude[j] = sum_p (sum_q |Ui[q, p]| |X[q, j]|)^2 of the first-order rounding bound (3 n + 4) u magnitude"""
    upper = np.triu(np.asarray(Ui, dtype=np.float64))
    Z = upper.astype(np.longdouble).T @ np.asarray(X, dtype=np.float64).astype(np.longdouble)
    magnitude = np.abs(upper).T @ np.abs(X)
    return np.sum(Z * Z, axis=0).astype(np.float64), np.sum(magnitude * magnitude, axis=0)


def sphere_positions(count, seed, radius=RADIUS):
    """count points on a sphere of `radius` metres, uniform in area, from a fixed seed"""
    v = np.random.default_rng(seed).standard_normal((count, 3))
    return radius * v / np.linalg.norm(v, axis=1, keepdims=True)


def hat_by_normals(A, U_factor, Q=None, longest=0):
    """the formula of PostFit.leverages on host arrays: h_i = |q_i|^2 + |U^-T (a_i - D q_i)|^2 for the rows a_i of A [L, P], the upper
    factor U_factor [P, P] and, under arc parameters, Q [L, r] with orthonormal columns (D = A^T Q; `longest` rows in the longest arc:
    the length of the dot products behind D).  Returns (h [L], bound [L]), the bound of the dot products, first order:
    (4 P + r + longest + 4) u sum_p (sum_q |Ui_qp| |a~_iq|)^2 with the magnitudes of the reduction |Q| |D|^T added to |a_i|, the
    inversion of U counted as one more product of length P (its entries are taken as the device inverts them only to rounding)."""
    from scipy.linalg import solve_triangular
    Ui = solve_triangular(U_factor, np.eye(U_factor.shape[0]), lower=False)
    rows, magnitude_rows, q2, r = A, np.abs(A), 0.0, 0
    if Q is not None and Q.shape[1]:
        D = A.T @ Q
        rows = A - Q @ D.T
        magnitude_rows = np.abs(A) + np.abs(Q) @ np.abs(D.T)
        q2, r = np.sum(Q * Q, axis=1), Q.shape[1]
    Z = rows @ np.triu(Ui)
    magnitude = magnitude_rows @ np.abs(np.triu(Ui))
    u = 2.0 ** -53
    return q2 + np.sum(Z * Z, axis=1), (4 * A.shape[1] + r + longest + 4) * u * (np.sum(magnitude * magnitude, axis=1) + q2)


def hat_by_qr(full):
    """the diagonal of the hat matrix of the full model [A B] (columns of zero norm dropped, rank-revealing): the row square sums of the
    orthonormal factor of a pivoted QR, over the columns of the numerical rank"""
    from scipy.linalg import qr
    Qf, Rf, _ = qr(full, mode='economic', pivoting=True)
    diagonal = np.abs(np.diag(Rf))
    rank = int(np.count_nonzero(diagonal > 1e-12 * diagonal[0]))
    return np.sum(Qf[:, :rank] ** 2, axis=1), rank


def orthonormal_arc_columns(units):
    """Q [L, sum of ranks]: an orthonormal basis of the span of every unit E [L, u] (the columns of one arc, or of one component of one
    arc, zero elsewhere), directions with eigenvalues at or below 1e-12 of the largest dropped, as the elimination drops them"""
    columns = []
    for E in units:
        values, vectors = np.linalg.eigh(E.T @ E)
        kept = values > 1e-12 * values[-1] if values[-1] > 0 else np.zeros(len(values), dtype=bool)
        if np.any(kept):
            columns.append(E @ (vectors[:, kept] / np.sqrt(values[kept])))
    return np.hstack(columns) if columns else np.zeros((units[0].shape[0] if units else 0, 0))


# ---- Huber ---------------------------------------------------------------------------------------------------------------------------------
PLANTED = (17, 58, 99, 140, 181)


def robust_problem(orthonormal, seed=4260, k=200, p=6):
    """(l [k], A [k, p], truth [p], planted): unit noise cut at 1.9 sigma (a clean sample beyond 2.5 sigma0 would be flagged rightly, and
    the planted set would no longer be the answer) and five planted errors of 20 to 30 sigma with alternating signs; A has orthonormal
    columns (the one setting in which the reference's formulas are right) or is a general design matrix"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((k, p))
    if orthonormal:
        A = np.linalg.qr(A)[0]
    else:
        A = A * np.array([1.0, 3.0, 0.5, 2.0, 1.5, 0.25])
    truth = rng.standard_normal(p) * (40.0 if orthonormal else 2.0)
    l = A @ truth + clean_noise(rng, k)
    planted = np.array(PLANTED)
    l[planted] += np.array([20.0, -22.5, 25.0, -27.5, 30.0])
    return l, A, truth, planted


def clean_noise(rng, shape, cut=1.9):
    """standard normal samples, those beyond `cut` drawn again until none is left"""
    noise = rng.standard_normal(shape)
    while np.any(np.abs(noise) > cut):
        beyond = np.abs(noise) > cut
        noise[beyond] = rng.standard_normal(int(np.count_nonzero(beyond)))
    return noise


def huber_factors(t, r, factors, threshold, power, redundancy_threshold):
    flagged = np.isfinite(t) & (t > threshold) & (r > redundancy_threshold)
    safe = np.where(flagged, t, threshold)
    return np.where(flagged, (threshold / safe) ** (2 * power), factors), flagged


def irls(l, A, threshold=2.5, power=1.5, redundancy_threshold=1e-4, max_iter=10, base=None, extra=None):
    """Iteratively reweighted least squares with Huber factors in NumPy, every iteration recorded: per iteration solve with the weights
    base * f, r_i = 1 - w_i a_i^T N^-1 a_i, sigma0^2 = sum w e^2 / (k - p), t = sqrt(w) |e| / (sigma0 sqrt(f) sqrt(r)).  extra [k, m]:
    further columns that are estimated along (arc parameters); returns a list of dicts x, factors, flags, sigma0 and the last one."""
    k = len(l)
    base = np.ones(k) if base is None else base
    full = A if extra is None else np.hstack((A, extra))
    factors, flags, history = np.ones(k), np.zeros(k, dtype=bool), []
    for _ in range(max_iter):
        w = base * factors
        rows = full * np.sqrt(w)[:, None]
        h, rank = hat_by_qr(rows)
        solution = np.linalg.lstsq(rows, np.sqrt(w) * l, rcond=None)[0]
        e = np.sqrt(w) * (l - full @ solution)
        r = 1.0 - h
        sigma0 = np.sqrt(e @ e / (k - rank))
        with np.errstate(invalid='ignore', divide='ignore'):
            t = np.where(r > 0, np.abs(e) / (np.sqrt(factors) * sigma0 * np.sqrt(np.where(r > 0, r, 1.0))), np.nan)
        new_factors, new_flags = huber_factors(t, r, factors, threshold, power, redundancy_threshold)
        history.append(dict(x=solution[:A.shape[1]], factors=new_factors, flags=new_flags, sigma0=sigma0, t=t, r=r))
        converged = np.array_equal(new_flags, flags) and np.array_equal(new_factors, factors)
        factors, flags = new_factors, new_flags
        if converged:
            break
    return history
