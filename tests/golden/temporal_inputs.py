"""Seeded inputs of the tests of time-variable parameters (tests/test_temporal_cpu.py, tests/test_gpu_temporal.py): nodes in time,
epochs along the 600 positions of design_inputs.loop_positions(), node fields, observations and weights, with NumPy restatements
of the model (the expanded design matrix) and of the block and slot planner (a point-by-point enumeration).  Needs NumPy only."""

import datetime

import numpy as np

import acceleration_inputs as ai
import design_inputs as di
import points_at_inputs as pi

GM, R = di.GM, di.R
N, MIN_DEGREE = di.LOOP['N'], di.LOOP['min_degree']               # d/o 2 .. 8
P = di.parameter_count(MIN_DEGREE, N)                             # 77
M = di.LOOP['count']                                              # 600
NODE_START = datetime.datetime(2017, 9, 4)                        # MJD 58000; the nodes are one day apart
MAX_SLOTS = 16


def positions():
    return di.loop_positions()


def pair_positions(seed=3331):
    """(a, b) [600, 3] each: a = positions(), b = a + 220 km d with seeded unit vectors d"""
    a = positions()
    d = np.random.default_rng(seed).standard_normal((M, 3))
    return a, a + 220e3 * d / np.sqrt(np.sum(d * d, axis=1))[:, np.newaxis]


def node_datetimes(B):
    return [NODE_START + datetime.timedelta(days=k) for k in range(B)]


def node_mjd(B):
    return np.array([pi.mjd(epoch) for epoch in node_datetimes(B)])


def epochs(B, seed=3301):
    """MJD [600], ascending over the B nodes: the first and the last node exactly, the interior nodes exactly, the rest uniform"""
    nodes = node_mjd(B)
    rng = np.random.default_rng(seed + B)
    inner = rng.uniform(nodes[0], nodes[-1], M - B)
    return np.sort(np.concatenate((nodes, inner)))


def node_fields(B, seed=3311):
    """anm [B, 9, 9]: 'anomaly' fields of consecutive seeds (degrees 0 and 1 are zero)"""
    return np.stack([ai.coefficients(N, 'anomaly', seed + k) for k in range(B)])


def observations(seed=3321):
    return np.random.default_rng(seed).standard_normal((M, 3)) * 1e-3


def weights(seed=3322):
    """per-component weights [600, 3] with zeros"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 4.0, (M, 3))
    w[rng.choice(M, 15, replace=False), rng.integers(0, 3, 15)] = 0.0
    w[7] = 0.0
    return w


def expand(design, first, factors, B):
    """A_tv [K M, B P] of the static design matrix [K M, P] (rows point-major): the rows of point i times factors[i, j] in the columns
    of field first[i] + j, zero elsewhere"""
    points, W = factors.shape
    K, columns = design.shape[0] // points, design.shape[1]
    rows = design.reshape(points, K, columns)
    out = np.zeros((points, K, B, columns))
    for i in range(points):
        for j in range(W):
            out[i, :, first[i] + j] = factors[i, j] * rows[i]
    return out.reshape(points * K, B * columns)


def reverse_runs(first):
    """a permutation of the points that reverses the order of the runs of equal `first` and keeps the order inside a run: a stable
    sort by first[permutation] restores the original order"""
    starts = np.flatnonzero(np.concatenate(([True], first[1:] != first[:-1])))
    bounds = np.concatenate((starts, [len(first)]))
    return np.concatenate([np.arange(bounds[r], bounds[r + 1]) for r in range(len(starts) - 1, -1, -1)])


# ---- the planner, point by point -----------------------------------------------------------------------------------------------------
def stages(arcs, count, q):
    """stage[t] = min(t - start of the arc of t, q)"""
    starts = np.asarray(arcs)
    t = np.arange(count)
    return np.minimum(t - starts[np.searchsorted(starts, t, side='right') - 1], q)


def enumerate_blocks(first, W, block_points, stage):
    """[(start, own, last, field, slots)] of the blocks: a block grows point by point from `own` until it holds block_points points,
    the window start changes (no noise model: stage None), one more point would need more than 16 slots, or a change of the
    window start meets the start of an arc"""
    count, blocks, t = len(first), [], 0
    while t < count:
        start = t - (int(stage[t]) if stage is not None else 0)
        lo, hi = min(first[start:t + 1]), max(first[start:t + 1])
        assert hi - lo + W <= MAX_SLOTS
        u = t + 1
        while u < count and u - t < block_points:
            if stage is None:
                if first[u] != first[t]:
                    break
            elif max(hi, first[u]) - min(lo, first[u]) + W > MAX_SLOTS or (stage[u] == 0 and first[u] != first[u - 1]):
                break
            lo, hi = min(lo, first[u]), max(hi, first[u])
            u += 1
        blocks.append((start, t, u, int(lo), int(hi - lo + W)))
        t = u
    return blocks


def enumerate_support(first, W, stage, own, last, field, e):
    """the owned columns, counted from `own`, at which slot e of the whitened expanded block can be non-zero: column u mixes the
    points u - stage[u] .. u, and one of them must hold field + e in its window"""
    columns = []
    for u in range(own, last):
        history = int(stage[u]) if stage is not None else 0
        if any(first[v] <= field + e < first[v] + W for v in range(u - history, u + 1)):
            columns.append(u - own)
    return columns
