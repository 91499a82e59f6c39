"""
The one route behind every from_* and of_* on the GPU, for all five kinds of observation at the smallest shape that has every seam:
degrees 2 .. 8 (P = 77), 300 points in blocks of 128 (three blocks, the last of 44), arcs [0, 150] under an AR(2) noise model (the
history of a block crosses the seams at 128 and 256), gradients with K = 4 components in frames, the 24 nodes of the radial-basis
fixture b2_8, weights per point.  Every surface of a kind must give the bits of the internal path (_observations and _normals or
_pass), TemporalParameters with one interval those of the static call, and a call that TemporalParameters sorts those of the same
points sorted by the caller.  Everything is compared under ==.
"""
import functools

import numpy as np
import pytest

import gradient_design_inputs as gdi
import grates_amd as ga
import los_inputs as li
import rbf_inputs as ri
import whitening_inputs as wi

pytestmark = pytest.mark.gpu

ls = ga.lstsq
GM, R = ri.GM, ri.R
MIN_DEGREE, N, P, J = 2, 8, 77, 24
M, BLOCK, ARCS = 300, 128, [0, 150]
COMPONENTS = ('xx', 'yy', 'zz', 'xz')
KINDS = ('accelerations', 'gradients', 'line_of_sight', 'potentials', 'potential_differences')
BAND = dict(min_degree=MIN_DEGREE, max_degree=N, GM=GM, R=R)


@functools.lru_cache(maxsize=None)
def _basis():
    lon, lat = ri.case_nodes('b2_8')
    K = ri.shape_factors(ri.degree_factors(MIN_DEGREE, N))
    return ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat), K, MIN_DEGREE, N, GM, R)


@functools.lru_cache(maxsize=None)
def _sequence():
    return wi.synthetic_sequence(ls, 2, 3601)


@functools.lru_cache(maxsize=None)
def _arguments(kind):
    """the per-point arguments, options and weights of the kind's call, by name; weights per point, with zeros"""
    rng = np.random.default_rng(3602 + KINDS.index(kind))
    a, b = (x[:M] for x in li.loop_pairs())
    w = rng.uniform(0.25, 4.0, M)
    w[rng.choice(M, 10, replace=False)] = 0.0
    return {'accelerations': dict(xyz=a, g=rng.standard_normal((M, 3)) * 1e-3),
            'gradients': dict(xyz=a, gradients=rng.standard_normal((M, 4)) * 1e-9, frames=gdi.frames(M, 3603), components=COMPONENTS),
            'line_of_sight': dict(xyz_a=a, xyz_b=b, differences=rng.standard_normal(M) * 1e-6, directions=li.unit_vectors(M, 3604)),
            'potentials': dict(xyz=a, potentials=rng.standard_normal(M)),
            'potential_differences': dict(xyz_a=a, xyz_b=b, differences=rng.standard_normal(M))}[kind], w


def _call(kind):
    arguments, w = _arguments(kind)
    return dict(arguments, weights=w)


def _model(noise):
    return ls.ColouredNoise(_sequence(), ARCS) if noise else None


def _same(first, second):
    """two NormalEquations: the same blocks with the same bits, right-hand side, square sum and count"""
    keys = [(r, c) for r in range(first.matrix.shape[0]) for c in range(first.matrix.shape[1]) if first.matrix.is_nonzero(r, c)]
    return (keys == [(r, c) for r in range(second.matrix.shape[0]) for c in range(second.matrix.shape[1]) if second.matrix.is_nonzero(r, c)]
            and all(bool((first.matrix.device_block(*key) == second.matrix.device_block(*key)).all()) for key in keys)
            and bool((first.right_hand_side == second.right_hand_side).all()) and first.observation_square_sum == second.observation_square_sum
            and first.observation_count == second.observation_count)


def _same_fit(first, second):
    """two PostFit: whitened, residuals and the square sums and counts of the arcs with the same bits"""
    return (np.array_equal(first.whitened, second.whitened) and np.array_equal(first.residuals, second.residuals)
            and np.array_equal(first.arc_square_sums, second.arc_square_sums) and np.array_equal(first.arc_observation_counts, second.arc_observation_counts))


def _solution(count, seed=3605):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(count) * 1e-9, rng.choice([-1.0, 1.0], (count, 2))


@pytest.mark.parametrize('kind', KINDS)
def test_the_bound_model_is_the_internal_path(kind):
    call, band = _call(kind), ga.engine.Band(**BAND)
    bound = ls.ColouredNoise(_sequence(), ARCS)
    ne = getattr(bound, 'from_' + kind)(block_points=BLOCK, **call, **BAND)
    assert ne.observation_count == {'accelerations': 3, 'gradients': 4}.get(kind, 1) * M and ne.matrix.device_block(0, 0).shape == (P, P)
    assert bool((ne.matrix.device_block(0, 0) == ne.matrix.device_block(0, 0).t()).all())              # mirrored exactly
    assert _same(getattr(bound, 'from_' + kind)(block_points=BLOCK, **call, **BAND), ne)                 # two runs are bitwise equal
    internal = ls.NormalEquations._normals(ls._observations(kind, call, band), ls._StochasticModel(_sequence(), ARCS), BLOCK)
    assert _same(internal, ne)
    white = getattr(ls.NormalEquations, 'from_' + kind)(block_points=BLOCK, **call, **BAND)
    assert _same(ls.NormalEquations._normals(ls._observations(kind, call, band), ls._StochasticModel(), BLOCK), white)
    assert not _same(white, ne)                                                                         # the model does something
    if kind == 'accelerations':
        assert _same(ls.NormalEquations.from_accelerations(block_points=BLOCK, noise_model=_sequence(), arcs=ARCS, **call, **BAND), ne)
    arcs = ls.ArcParameters(ls.arc_basis(ARCS, M, degree=1), ARCS, _sequence())
    reduced = getattr(arcs, 'from_' + kind)(block_points=BLOCK, **call, **BAND)
    internal = ls.NormalEquations._normals(ls._observations(kind, call, band), ls._StochasticModel(_sequence(), ARCS, arcs), BLOCK)
    assert _same(internal, reduced) and np.array_equal(internal.arc_elimination.ranks, reduced.arc_elimination.ranks)


@pytest.mark.parametrize('noise', [False, True])
@pytest.mark.parametrize('kind', KINDS)
def test_one_interval_is_the_static_call(kind, noise):
    call = _call(kind)
    temporal = ls.TemporalParameters.constant(np.array([0.0, 1.0]), np.linspace(0.1, 0.9, M), _model(noise))
    assert temporal.field_count == 1
    ne = getattr(temporal, 'from_' + kind)(block_points=BLOCK, **call, **BAND)
    static = getattr(_model(noise) or ls.NormalEquations, 'from_' + kind)(block_points=BLOCK, **call, **BAND)
    assert _same(ne, static)
    x, z = _solution(P)
    fit = getattr(temporal, 'of_' + kind)(x, block_points=BLOCK, vectors=z, **call, **BAND)
    plain = getattr(ls.PostFit, 'of_' + kind)(x, block_points=BLOCK, model=_model(noise), vectors=z, **call, **BAND)
    assert _same_fit(fit, plain) and bool((fit.rows == plain.rows).all())
    assert fit.whitened.shape == (M, {'accelerations': 3, 'gradients': 4}.get(kind, 1)) and np.any(fit.whitened != fit.residuals) == noise


@pytest.mark.parametrize('kind', KINDS)
def test_sorting_is_the_callers_sort(kind):
    """linear interpolation between four nodes, the points given backwards in time: the window starts decrease, the call sorts"""
    arguments, w = _arguments(kind)
    entry = ga.engine.OBSERVATION_KINDS[kind]
    nodes, epochs = np.array([0.0, 1.0, 2.0, 3.0]), np.linspace(2.9, 0.1, M)
    given = ls.TemporalParameters.linear(nodes, epochs)
    order = ga.engine.points_at_plan(given.first)[0]
    assert order is not None and np.any(np.diff(given.first) < 0)
    sorted_call = dict(arguments, weights=w[order], **{name: arguments[name][order] for name in entry.points})
    presorted = ls.TemporalParameters.linear(nodes, epochs[order])
    assert ga.engine.points_at_plan(presorted.first)[0] is None
    ne = getattr(given, 'from_' + kind)(block_points=BLOCK, **dict(arguments, weights=w), **BAND)
    assert ne.matrix.shape == (4, 4) and _same(ne, getattr(presorted, 'from_' + kind)(block_points=BLOCK, **sorted_call, **BAND))
    x, z = _solution(4 * P)
    fit = getattr(given, 'of_' + kind)(x, block_points=BLOCK, vectors=z, **dict(arguments, weights=w), **BAND)
    sorted_fit = getattr(presorted, 'of_' + kind)(x, block_points=BLOCK, vectors=z, **sorted_call, **BAND)
    assert np.array_equal(fit.whitened[order], sorted_fit.whitened) and np.array_equal(fit.residuals[order], sorted_fit.residuals)      # in the order given
    assert bool((fit.rows[:, :, order] == sorted_fit.rows).all())                        # (the square sums of an arc add them in another order)


@pytest.mark.parametrize('noise', [False, True])
@pytest.mark.parametrize('kind', KINDS)
def test_radial_basis_parameters_are_the_internal_path(kind, noise):
    call, band = _call(kind), ga.engine.basis_band(_basis())
    bound = ls.RadialBasisParameters(_basis(), _model(noise))
    ne = getattr(bound, 'from_' + kind)(block_points=BLOCK, **call)
    assert ne.matrix.device_block(0, 0).shape == (J, J)
    internal = ls.NormalEquations._normals(ls._observations(kind, call, band), ls._StochasticModel.of(_model(noise)), BLOCK)
    assert _same(internal, ne)
    x, z = _solution(J)
    fit = getattr(bound, 'of_' + kind)(x, block_points=BLOCK, vectors=z, **call)
    first = call[ga.engine.OBSERVATION_KINDS[kind].points[0]]
    internal = ls.PostFit(x, z, _model(noise), first)._pass(ls._observations(kind, call, band), ls._StochasticModel.of(_model(noise)), BLOCK)
    assert _same_fit(fit, internal) and bool((fit.rows == internal.rows).all())
    plain = getattr(ls.PostFit, 'of_' + kind)(np.zeros(P), block_points=BLOCK, model=_model(noise), **call, **BAND)
    zero = getattr(bound, 'of_' + kind)(np.zeros(J), block_points=BLOCK, **call)
    assert _same_fit(zero, plain)                                                                       # x = 0: the observations under the model, whatever the parameters
