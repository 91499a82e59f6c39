"""Seeded inputs of the acceleration design matrix fixture (tests/golden/make_golden_acceleration_design.py ->
g24_acceleration_design.npz) and of the tests that replay it, with a float64 NumPy restatement of the formulas of
grates_amd/csrc/design.hip.  Needs NumPy only."""

import numpy as np

import acceleration_inputs as ai

GM, R = ai.GM, ai.R
DEGREES = (8, 2)                                      # design matrices of the fixture (min_degree 0; min_degree 2 is a column slice)
AX = ('static60', 60, 2411)                           # ax_err: positions of this g22 case, degree and seed of the anomaly field
LOOP = {'N': 8, 'min_degree': 2, 'count': 600, 'position_seed': 2421, 'field_seed': 2422}      # closed loop (GPU case 11)


def positions():
    """the special positions of the acceleration fixture (exact poles, 1 mm off a pole, equator, +-0 on the antimeridian, below R)
    and seven scattered ones at heights of -25 .. 500 km"""
    return np.vstack((ai.special_positions(), ai.scattered_positions(7, 2401)))


def parameter_count(min_degree, max_degree):
    return (max_degree + 1) ** 2 - min_degree ** 2


def degreewise(min_degree, max_degree):
    """(n, m, sine) of every entry of the degree-wise coefficient vector C_n0, C_n1, S_n1, C_n2, ..."""
    out = []
    for n in range(min_degree, max_degree + 1):
        out.append((n, 0, 0))
        for m in range(1, n + 1):
            out += [(n, m, 0), (n, m, 1)]
    return out


def unit_field(n, m, sine, max_degree):
    """anm [N+1, N+1] with one coefficient set to 1: C_nm at [n, m], S_nm at [m - 1, n]"""
    anm = np.zeros((max_degree + 1, max_degree + 1))
    if sine:
        anm[m - 1, n] = 1.0
    else:
        anm[n, m] = 1.0
    return anm


def ravel(anm, min_degree, max_degree):
    return np.array([anm[m - 1, n] if sine else anm[n, m] for n, m, sine in degreewise(min_degree, max_degree)])


def unit_field_matrix(acceleration, xyz, min_degree, max_degree):
    """A [3 M, P] column by column from `acceleration(anm) -> g [M, 3]` of unit coefficient fields"""
    columns = [acceleration(unit_field(n, m, sine, max_degree)).ravel() for n, m, sine in degreewise(min_degree, max_degree)]
    return np.stack(columns, axis=1)


def restatement(xyz, min_degree, max_degree, GM=GM, R=R):
    """A [3 M, P] by the formulas of csrc/design.hip in float64 NumPy: solid harmonics of degree N + 1 by the column recursion, then
    one or two products per entry"""
    N1 = max_degree + 1
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r = np.sqrt((x * x + y * y) + z * z)
    th = np.arctan2(np.sqrt(x * x + y * y), z)
    lam = np.arctan2(y, x)
    u, t = R / r, np.cos(th)
    s = np.sqrt(1.0 - t * t)
    Yc, Ys = {}, {}
    pmm, rk = np.ones_like(t), u.copy()
    for k in range(N1 + 1):
        if k == 1:
            pmm = np.sqrt(3.0) * s
        elif k >= 2:
            pmm = np.sqrt((2.0 * k + 1.0) / (2.0 * k)) * s * pmm
        if k >= 1:
            rk = rk * u
        ck, sk = np.cos(k * lam), np.sin(k * lam)
        p1, p2, rad = pmm, np.zeros_like(t), rk
        for n in range(k, N1 + 1):
            if n > k:
                a = np.sqrt((2 * n - 1) / (n - k) * (2 * n + 1) / (n + k))
                b = np.sqrt((2 * n + 1) / (2 * n - 3) * (n - k - 1) / (n - k) * (n + k - 1) / (n + k)) if n > k + 1 else 0.0
                p1, p2 = (a * t) * p1 - b * p2, p1
            pk = p1 * rad
            rad = rad * u
            Yc[n, k], Ys[n, k] = pk * ck, pk * sk
    scale = GM / (2.0 * R * R)
    A = np.zeros((xyz.shape[0], 3, parameter_count(min_degree, max_degree)))
    for col, (n, m, sine) in enumerate(degreewise(min_degree, max_degree)):
        base = np.sqrt((2.0 * n + 1.0) / (2.0 * n + 3.0))
        same, other = (Ys, Yc) if sine else (Yc, Ys)
        sign = 1.0 if sine else -1.0                   # of the y component: +Yc for a sine coefficient, -Ys for a cosine coefficient
        gx = gy = 0.0
        if m >= 1:
            fm = np.sqrt((n - m + 1.0) * (n - m + 2.0)) * base * (np.sqrt(2.0) if m == 1 else 1.0)
            gx = gx + fm * same[n + 1, m - 1]
            gy = gy + sign * fm * other[n + 1, m - 1]
        fp = np.sqrt((n + m + 1.0) * (n + m + 2.0)) * base * (np.sqrt(2.0) if m == 0 else 1.0)
        gx = gx - fp * same[n + 1, m + 1]
        gy = gy + (fp if sine else -fp) * other[n + 1, m + 1]
        f0 = np.sqrt((n - m + 1.0) * (n + m + 1.0)) * base
        A[:, 0, col], A[:, 1, col], A[:, 2, col] = gx * scale, gy * scale, (-2.0 * f0) * same[n + 1, m] * scale
    return A.reshape(-1, A.shape[2])


def loop_positions():
    return ai.scattered_positions(LOOP['count'], LOOP['position_seed'])


def loop_field():
    """anm [9, 9]: the d/o-8 anomaly field of the closed loop (degrees 0 and 1 are zero)"""
    return ai.coefficients(LOOP['N'], 'anomaly', LOOP['field_seed'])
