"""Seeded inputs of the gradient-tensor design matrix fixture (tests/golden/make_golden_gradient_design.py ->
g25_gradient_design.npz) and of the tests that replay it, with a float64 NumPy restatement of the formulas of the second half of
grates_amd/csrc/design.hip.  Needs NumPy only.

The solid harmonics follow design_inputs.restatement (the column recursion, (R/r)^(n+1) carried along) except for the colatitude:
cos and sin enter as z / r and rho / r, the form of the gradient kernels.  design_inputs' s = sqrt(1 - t^2) is exactly 0 at the
fixture's point 1 mm off the pole, which costs the order-1 harmonics there 2e-10 of max|A| against the mp oracle."""

import numpy as np

import acceleration_inputs as ai
import design_inputs as di

GM, R = ai.GM, ai.R
DEGREES = (8, 2)                                      # design matrices of the fixture (min_degree 0; min_degree 2 is a column slice)
COMPONENTS = ('xx', 'xy', 'xz', 'yy', 'yz', 'zz')     # canonical order: bit j of the C ABI's component set
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
FRAME_SEED = 2501
AX = ('anomaly96', 96)                                # ax_err: the g23 case whose positions, field and tensor are used
LOOP = {'N': 8, 'min_degree': 2, 'count': 600, 'position_seed': 2511, 'field_seed': 2512, 'frame_seed': 2513}
LOOP_SETS = {'all': COMPONENTS, 'goce': ('xx', 'yy', 'zz', 'xz')}

parameter_count, degreewise, ravel = di.parameter_count, di.degreewise, di.ravel


def positions():
    """the 20 positions of the acceleration design fixture"""
    return di.positions()


def frames(count, seed=FRAME_SEED):
    """[count, 3, 3] proper rotations (rows = instrument axes): Q of the QR factorisation of seeded Gaussian matrices with the sign of
    the last row chosen for determinant +1; the first is left as the identity"""
    rng = np.random.default_rng(seed)
    out = np.empty((count, 3, 3))
    for i in range(count):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[2] = -q[2]
        out[i] = q
    out[0] = np.eye(3)
    return out


def component_indices(components=None):
    """positions in COMPONENTS of the selected names, ascending"""
    if components is None:
        return list(range(6))
    return sorted(COMPONENTS.index(name) for name in components)


def packed(N2, n, k):
    """packed order-major index of (n, k) at degree N2: order_offset(N2, k) + n - k"""
    return k * (N2 + 1) - (k * (k - 1)) // 2 + n - k


def solid_harmonics(xyz, N2, R=R):
    """Y [2 packed_count(N2), M]: row 2 packed(n, k) is (R/r)^(n+1) P_nk cos(k lon), the next one the same with sin"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r = np.sqrt((x * x + y * y) + z * z)
    lam = np.arctan2(y, x)
    u, t = R / r, z / r
    s = np.sqrt(x * x + y * y) / r
    Y = np.zeros(((N2 + 1) * (N2 + 2), xyz.shape[0]))
    pmm, rk = np.ones_like(t), u.copy()
    for k in range(N2 + 1):
        if k == 1:
            pmm = np.sqrt(3.0) * s
        elif k >= 2:
            pmm = np.sqrt((2.0 * k + 1.0) / (2.0 * k)) * s * pmm
        if k >= 1:
            rk = rk * u
        ck, sk = np.cos(k * lam), np.sin(k * lam)
        p1, p2, rad = pmm, np.zeros_like(t), rk
        for n in range(k, N2 + 1):
            if n > k:
                a = np.sqrt((2 * n - 1) / (n - k) * (2 * n + 1) / (n + k))
                b = np.sqrt((2 * n + 1) / (2 * n - 3) * (n - k - 1) / (n - k) * (n + k - 1) / (n + k)) if n > k + 1 else 0.0
                p1, p2 = (a * t) * p1 - b * p2, p1
            pk = p1 * rad
            rad = rad * u
            Y[2 * packed(N2, n, k)], Y[2 * packed(N2, n, k) + 1] = pk * ck, pk * sk
    return Y


def d_terms(c, term):
    """the acceleration's map D_c (0: x, 1: y, 2: z) of one solid-harmonic coefficient (n, k, kind, value): its terms of degree n + 1
    (the rows of design_inputs.restatement read from the coefficient's side)"""
    n, m, sine, value = term
    base = np.sqrt((2.0 * n + 1.0) / (2.0 * n + 3.0))
    out = []

    def put(k, kind, factor):
        if not (kind == 1 and k == 0):                 # Ys of order 0 is zero
            out.append((n + 1, k, kind, value * factor))

    if c == 2:
        put(m, sine, -2.0 * (np.sqrt((n - m + 1.0) * (n + m + 1.0)) * base))
        return out
    if m >= 1:
        fm = np.sqrt((n - m + 1.0) * (n - m + 2.0)) * base * (np.sqrt(2.0) if m == 1 else 1.0)
        if c == 0:
            put(m - 1, sine, fm)
        else:
            put(m - 1, 1 - sine, fm if sine else -fm)
    fp = np.sqrt((n + m + 1.0) * (n + m + 2.0)) * base * (np.sqrt(2.0) if m == 0 else 1.0)
    if c == 0:
        put(m + 1, sine, -fp)
    else:
        put(m + 1, 1 - sine, fp if sine else -fp)
    return out


def table(min_degree, max_degree):
    """slot [P, 6, 4] (int32, -1: no term) and factor [P, 6, 4]: D_d of D_c (c <= d) of every unit coefficient, terms on one slot merged"""
    N2 = max_degree + 2
    P = parameter_count(min_degree, max_degree)
    slot, factor = np.full((P, 6, 4), -1, dtype=np.int32), np.zeros((P, 6, 4))
    for row, (n, m, sine) in enumerate(degreewise(min_degree, max_degree)):
        for comp, (c, d) in enumerate(PAIRS):
            merged = {}
            for first in d_terms(c, (n, m, sine, 1.0)):
                for n2, k, kind, value in d_terms(d, first):
                    s = 2 * packed(N2, n2, k) + kind
                    merged[s] = merged.get(s, 0.0) + value
            for j, (s, value) in enumerate(merged.items()):
                slot[row, comp, j], factor[row, comp, j] = s, value
    return slot, factor


def evaluate_table(slot, factor, Y, GM=GM, R=R):
    """A [6 M, P] (row 6 i + j) in the Earth-fixed frame: sum of factor * Y[slot] in the order of the table, times GM / (4 R^3)"""
    Yx = np.vstack((Y, np.zeros((1, Y.shape[1]))))
    index = np.where(slot < 0, Y.shape[0], slot)
    value = np.zeros(slot.shape[:2] + (Y.shape[1],))
    for j in range(slot.shape[2]):
        value = value + factor[:, :, j, np.newaxis] * Yx[index[:, :, j]]
    scale = GM / (4.0 * R * R * R)
    return (value * scale).transpose(2, 1, 0).reshape(6 * Y.shape[1], slot.shape[0])


def rotate_rows(A6, frames=None, components=None):
    """[K M, P] (row K i + j): the rows of the Earth-fixed six-component matrix A6 [6 M, P] as F T F^T, selected components only"""
    M, P = A6.shape[0] // 6, A6.shape[1]
    rows = A6.reshape(M, 6, P)
    T = np.empty((M, 3, 3, P))
    for j, (c, d) in enumerate(PAIRS):
        T[:, c, d] = T[:, d, c] = rows[:, j]
    if frames is not None:
        T = np.einsum('iac,icdp,ibd->iabp', frames, T, frames)
    picked = [T[:, PAIRS[j][0], PAIRS[j][1]] for j in component_indices(components)]
    return np.stack(picked, axis=1).reshape(M * len(picked), P)


def restatement(xyz, min_degree, max_degree, frames=None, components=None, GM=GM, R=R):
    """A [K M, P] by the formulas of the kernels in float64 NumPy: solid harmonics of degree N + 2, the table terms, F T F^T"""
    slot, factor = table(min_degree, max_degree)
    A6 = evaluate_table(slot, factor, solid_harmonics(xyz, max_degree + 2, R), GM, R)
    return rotate_rows(A6, frames, components)


def rotate_tensor(T, frames, components=None):
    """observations [M, K] from tensors T [M, 3, 3]: the selected entries of F T F^T"""
    Tr = T if frames is None else np.einsum('iac,icd,ibd->iab', frames, T, frames)
    return np.stack([Tr[:, PAIRS[j][0], PAIRS[j][1]] for j in component_indices(components)], axis=1)


def loop_positions():
    return ai.scattered_positions(LOOP['count'], LOOP['position_seed'])


def loop_field():
    """anm [9, 9]: the d/o-8 anomaly field of the closed loop (degrees 0 and 1 are zero)"""
    return ai.coefficients(LOOP['N'], 'anomaly', LOOP['field_seed'])


def loop_frames():
    return frames(LOOP['count'], LOOP['frame_seed'])
