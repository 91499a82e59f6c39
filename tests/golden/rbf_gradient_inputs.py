"""Seeded inputs of the fixture of the gradient-tensor design matrix with respect to the node values of radial basis functions
(tests/golden/make_golden_rbf_gradients.py -> g30_rbf_gradients.npz) and of the tests that replay it, with a float64 NumPy
restatement of RbfChain<2> (grates_amd/csrc/rbf.h), RbfGradient (rbf.hip) and FrameTensor (observe.h) in the kernel's operation order: the
chain, the closed Hessian, the rotation into the instrument frames, the scaling and the weights.  The kernel has no transcendental
function, so the restatement reproduces it bit for bit.  Needs NumPy only; the basis, the nodes and the points are rbf_inputs'."""

import numpy as np

import acceleration_inputs as ai
import gradient_design_inputs as gdi
import rbf_inputs as ri

GM, R = ri.GM, ri.R
COMPONENTS, PAIRS = gdi.COMPONENTS, gdi.PAIRS
CASES = ri.CASES
FRAME_SEED = 3001
GROWTH_DEGREES = (8, 60, 96, 180)                      # float64 against long double: how the rounding of t near +-1 grows with N
# the high-degree case: flat shape factors (the hardest), points at heights of -25 .. 500 km
N60 = {'min_degree': 2, 'max_degree': 60, 'nodes': 8, 'node_seed': 3011, 'points': 64, 'point_seed': 3012, 'frame_seed': 3013}
N96 = {'min_degree': 2, 'max_degree': 96, 'points': 16}      # the mp column at d/o 96: N60's nodes and its first points, flat factors
# the closed loop: the geometry of rbf_inputs.LOOP in seeded frames, the components of a gradiometer with two weak axes
LOOP_COMPONENTS = ('xx', 'yy', 'zz', 'xz')
LOOP_FRAME_SEED = 3021
LOOP_BIAS_SEED = 3022


def positions(tag):
    """xyz [29, 3]: rbf_inputs.pairs(tag)[0], with the points above a node, antipodal to it and 1 m beside it"""
    return ri.pairs(tag)[0]


def frames(count, seed=FRAME_SEED):
    """[count, 3, 3] seeded proper rotations, the first the identity (gradient_design_inputs.frames)"""
    return gdi.frames(count, seed)


def n60_nodes():
    return ri.scattered_nodes(N60['nodes'], N60['node_seed'])


def n60_positions():
    return ai.scattered_positions(N60['points'], N60['point_seed'])


def n60_frames():
    return gdi.frames(N60['points'], N60['frame_seed'])


def loop_frames():
    return gdi.frames(ri.LOOP['count'], LOOP_FRAME_SEED)


def loop_biases():
    """[12, 4] in -1 .. 1: the planted bias of every arc and component of the closed loop, in units of max|l|"""
    return np.random.default_rng(LOOP_BIAS_SEED).uniform(-1.0, 1.0, (ri.loop_arcs().size, len(LOOP_COMPONENTS)))


def bias_indicator():
    """B [4 * 600, 12 * 4]: row 4 i + c observes the bias of component c of the arc of point i"""
    K, count = len(LOOP_COMPONENTS), ri.LOOP['count']
    B = np.zeros((K * count, ri.loop_arcs().size * K))
    i, c = np.divmod(np.arange(K * count), K)
    B[np.arange(K * count), (i // ri.LOOP['arc_length']) * K + c] = 1.0
    return B


# ---- the restatement of RbfChain<2>, RbfGradient and FrameTensor ---------------------------------------------------------------------------
def degree_table(k, min_degree, dtype=np.float64):
    """(alpha, beta, gamma, d, e, h) [N + 1] each, as rbf_degree_table builds them for RbfDegree<2>: h = (n + 2) e"""
    k = np.asarray(k, dtype=dtype)
    n = np.arange(k.size).astype(dtype)
    one, two = dtype(1.0), dtype(2.0)
    safe = np.maximum(n, one)
    alpha = np.where(n > 0, (two * n - one) / safe, dtype(0.0))
    beta = np.where(n > 0, (n - one) / safe, dtype(0.0))
    gamma = np.where(n > 0, two * n - one, dtype(0.0))
    d = np.where(n < min_degree, dtype(0.0), k * (two * n + one))
    e = (n + one) * d
    return alpha, beta, gamma, d, e, (n + two) * e


def hessians(xyz, nodes, k, min_degree, GM=GM, R=R, dtype=np.float64):
    """(T [M, J, 6], scale [M]): the six unscaled Earth-fixed entries xx, xy, xz, yy, yz, zz of RbfChain<2>.finish for every (point,
    node) pair and GM / (R r^2) as the kernel forms it.  dtype=np.longdouble runs the same operations in extended precision (the
    inputs are the float64 values, converted exactly)."""
    alpha, beta, gamma, d, e, h = degree_table(k, min_degree, dtype)
    xyz, nodes = np.asarray(xyz).astype(dtype), np.asarray(nodes).astype(dtype)
    GM, R = dtype(GM), dtype(R)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r = np.sqrt((x * x + y * y) + z * z)
    xh = np.stack((x / r, y / r, z / r), axis=1)                                        # [M, 3]
    u, rinv = R / r, dtype(1.0) / r
    t = (xh[:, None, 0] * nodes[None, :, 0] + xh[:, None, 1] * nodes[None, :, 1]) + xh[:, None, 2] * nodes[None, :, 2]      # [M, J]
    q = u[:, None] * nodes[None, :, 3]
    qn = q.copy()
    zero = np.zeros_like(t)
    p1, p2, dp1, dp2, ddp1, ddp2 = np.ones_like(t), zero, zero, zero, zero, zero
    sr, srr, st, srt, stt = e[0] * qn, h[0] * qn, zero, zero, zero
    for n in range(1, alpha.size):
        p = (alpha[n] * t) * p1 - beta[n] * p2
        dp = dp2 + gamma[n] * p1
        ddp = ddp2 + gamma[n] * dp1
        p2, p1, dp2, dp1, ddp2, ddp1 = p1, p, dp1, dp, ddp1, ddp
        qn = qn * q
        w = qn * p
        wd = qn * dp
        sr = sr + e[n] * w
        srr = srr + h[n] * w
        st = st + d[n] * wd
        srt = srt + e[n] * wd
        stt = stt + d[n] * (qn * ddp)
    tau = nodes[None, :, :3] - t[:, :, None] * xh[:, None, :]                           # [M, J, 3]
    b, m = sr + t * st, srt + st
    T = np.empty(t.shape + (6,), dtype=dtype)
    for j, (c, dd) in enumerate(PAIRS):
        xx = (xh[:, c] * xh[:, dd])[:, None]
        kk = dtype(1.0) - xx if c == dd else -xx
        T[:, :, j] = ((srr * xx - b * kk) - m * (xh[:, None, c] * tau[:, :, dd] + tau[:, :, c] * xh[:, None, dd])) + stt * (tau[:, :, c] * tau[:, :, dd])
    return T, ((GM / R) * rinv) * rinv


def rotate(T, frames, picked):
    """[M, J, K]: the selected entries of F T F^T in the kernel's order, u_b = T f_b once per b, then f_a . u_b, the sums associated
    (a + b) + c; without frames the selected Earth-fixed entries as they are"""
    if frames is None:
        return T[:, :, picked]
    F = frames[:, None, :, :]                                                           # [M, 1, 3, 3]
    rows = ((0, 1, 2), (1, 3, 4), (2, 4, 5))                                            # the entries of row c of T
    u = [[(T[:, :, rows[c][0]] * F[:, :, b, 0] + T[:, :, rows[c][1]] * F[:, :, b, 1]) + T[:, :, rows[c][2]] * F[:, :, b, 2] for c in range(3)]
         for b in range(3)]
    out = [(F[:, :, a, 0] * u[b][0] + F[:, :, a, 1] * u[b][1]) + F[:, :, a, 2] * u[b][2] for a, b in (PAIRS[j] for j in picked)]
    return np.stack(out, axis=2)


def restatement(nodes, k, min_degree, xyz, frames=None, components=None, weights=None, GM=GM, R=R, dtype=np.float64):
    """A [K M, J] in NumPy, rows as gravityfield.rbf_gradient_design_matrix orders them (row K i + j: the j-th selected component at
    point i): (value * scale) * sqrt(w) with weights None, [M] or [M, K]"""
    picked = gdi.component_indices(components)
    T, scale = hessians(xyz, nodes, k, min_degree, GM, R, dtype)
    value = rotate(T, None if frames is None else np.asarray(frames).astype(dtype), picked) * scale[:, None, None]      # [M, J, K]
    if weights is not None:
        root = np.sqrt(np.asarray(weights).astype(dtype))
        value = value * (root[:, None, :] if root.ndim == 2 else root[:, None, None])
    return value.transpose(0, 2, 1).reshape(-1, nodes.shape[0])


def growth(N, dtype=np.longdouble):
    """max|A_float64 - A_longdouble| / max|A| of the Earth-fixed matrix of the high-degree geometry (N60's nodes and points) with flat
    shape factors in 2 .. N: the rounding of the float64 chain, which grows with the degree through P''_n ~ n^4 near t = +-1"""
    nodes = ri.node_table(*n60_nodes())
    k = ri.degree_factors(N60['min_degree'], N, flat=True)
    A = restatement(nodes, k, N60['min_degree'], n60_positions())
    exact = restatement(nodes, k, N60['min_degree'], n60_positions(), dtype=dtype)
    return float(np.abs(A.astype(dtype) - exact).max() / np.abs(exact).max())
