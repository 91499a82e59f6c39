"""
CPU checks of the one table of observation kinds (engine.OBSERVATION_KINDS) behind every from_* and of_*: each of the five kinds,
reached through each of its surfaces -- the from_* of NormalEquations, ColouredNoise, ArcParameters, RadialBasisParameters and
TemporalParameters, the of_* of PostFit, RadialBasisParameters and TemporalParameters -- refuses the same bad call with the same
ValueError, before anything reaches the device; TemporalParameters does so whether it sorts the points or not, and checks once; and the
design-matrix functions of engine raise the messages of the lstsq surfaces, because the checks of a kind exist once.  Inputs: the 29
points of the radial-basis fixture (b2_8), degrees 2 .. 8.
"""
import inspect

import numpy as np
import pytest

import grates_amd as ga
import rbf_gradient_inputs as rg
import rbf_inputs as ri

GM, R = ri.GM, ri.R
TAG, M, P, J = 'b2_8', 29, 77, 24
BAND = dict(min_degree=2, max_degree=8, GM=GM, R=R)
KINDS = ('accelerations', 'gradients', 'line_of_sight', 'potentials', 'potential_differences')
ARCS = [0, 15]


def _basis():
    lon, lat = ri.case_nodes(TAG)
    K = ri.shape_factors(ri.degree_factors(2, 8))
    return ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat), K, 2, 8, GM, R)


def _noise():
    lstsq = ga.lstsq
    return lstsq.AutoregressiveModelSequence([lstsq.AutoregressiveModel((), np.array([[1.0]])),
                                              lstsq.AutoregressiveModel([np.array([[0.5]])], np.array([[0.75]]))])


def _good(kind):
    """the arguments of a good call of the kind, by name and in call order"""
    a, b = ri.pairs(TAG)
    return {'accelerations': dict(xyz=a, g=np.zeros((M, 3))),
            'gradients': dict(xyz=a, gradients=np.zeros((M, 4)), frames=rg.frames(M), components=rg.LOOP_COMPONENTS),
            'line_of_sight': dict(xyz_a=a, xyz_b=b, differences=np.zeros(M), directions=ri.directions(TAG)),
            'potentials': dict(xyz=a, potentials=np.zeros(M)),
            'potential_differences': dict(xyz_a=a, xyz_b=b, differences=np.zeros(M))}[kind]


def _bad_calls(kind):
    """(label, what the bad call changes) for the kind; every one must be refused on the host"""
    entry = ga.engine.OBSERVATION_KINDS[kind]
    good = _good(kind)
    K = {'accelerations': 3, 'gradients': 4}.get(kind, 1)
    bad = [('position shape', {entry.points[0]: np.zeros((5, 2))}),
           ('value count', {entry.observed: good[entry.observed][:M - 1]}),
           ('weight shape', dict(weights=np.ones((M, K + 1)))),
           ('negative weight', dict(weights=-np.ones(M))),
           ('NaN weight', dict(weights=np.full(M, np.nan))),
           ('block_points', dict(block_points=0))]
    if K == 1:
        bad += [('weight column', dict(weights=np.ones((M, 1))))]                      # one value per point: weights [M] only
    if kind == 'gradients':
        bad += [('frames', dict(frames=1.001 * good['frames'])), ('unknown component', dict(components=('xx', 'yx'))),
                ('duplicate component', dict(components=('xx', 'xx')))]
    if kind == 'line_of_sight':
        bad += [('direction', dict(directions=2.0 * good['directions'])), ('coinciding pair', dict(directions=None))]      # pair 26 coincides
    return bad


def _temporal(descending, model=None):
    """three independent fields; descending: the window starts decrease along the points, so a call without a noise model sorts"""
    first = np.arange(M) // 10
    return ga.lstsq.TemporalParameters(first[::-1].copy() if descending else first, np.ones((M, 1)), 3, model)


def _from_surfaces(kind):
    lstsq = ga.lstsq
    name = 'from_' + kind
    bound = lstsq.RadialBasisParameters(_basis())
    return {'NormalEquations': lambda **kw: getattr(lstsq.NormalEquations, name)(**kw, **BAND),
            'ColouredNoise': lambda **kw: getattr(lstsq.ColouredNoise(_noise(), ARCS), name)(**kw, **BAND),
            'ArcParameters': lambda **kw: getattr(lstsq.ArcParameters(lstsq.arc_basis(ARCS, M, degree=0), ARCS), name)(**kw, **BAND),
            'RadialBasisParameters': lambda **kw: getattr(bound, name)(**kw),
            'TemporalParameters': lambda **kw: getattr(_temporal(False), name)(**kw, **BAND),
            'TemporalParameters, sorting': lambda **kw: getattr(_temporal(True), name)(**kw, **BAND),
            'TemporalParameters, coloured': lambda **kw: getattr(_temporal(True, lstsq.ColouredNoise(_noise(), ARCS)), name)(**kw, **BAND)}


def _of_surfaces(kind):
    """{surface: (call, the number of parameters of its solution)}"""
    lstsq = ga.lstsq
    name = 'of_' + kind
    bound = lstsq.RadialBasisParameters(_basis())
    return {'PostFit': (lambda solution, **kw: getattr(lstsq.PostFit, name)(solution, **kw, **BAND), P),
            'RadialBasisParameters': (lambda solution, **kw: getattr(bound, name)(solution, **kw), J),
            'TemporalParameters': (lambda solution, **kw: getattr(_temporal(False), name)(solution, **kw, **BAND), 3 * P),
            'TemporalParameters, sorting': (lambda solution, **kw: getattr(_temporal(True), name)(solution, **kw, **BAND), 3 * P)}


def _message(call, *args, **kwargs):
    with pytest.raises(ValueError) as err:
        call(*args, **kwargs)
    return str(err.value)


@pytest.mark.parametrize('kind', KINDS)
def test_every_surface_refuses_a_bad_call_alike(kind):
    good = _good(kind)
    surfaces, fits = _from_surfaces(kind), _of_surfaces(kind)
    assert len(surfaces) == 7 and len(fits) == 4
    for label, change in _bad_calls(kind):
        arguments = dict(good, **change)
        expected = _message(surfaces['NormalEquations'], **arguments)
        assert expected, label
        for surface, call in surfaces.items():
            assert _message(call, **arguments) == expected, (label, surface)
        for surface, (call, count) in fits.items():
            assert _message(call, np.zeros(count), **arguments) == expected, (label, surface)
    for surface, (call, count) in fits.items():
        expected = 'solution must have shape ({0},) or ({0}, 1), got (5,)'.format(count)
        assert _message(call, np.zeros(5), **good) == expected, surface
        assert _message(call, np.zeros(count), vectors=np.zeros((count + 1, 2)), **good) == 'vectors must have shape ({0}, S), got ({1}, 2)'.format(
            count, count + 1), surface


def test_messages_name_what_was_wrong():
    """the texts themselves, once per check: the comparison above would also pass on a wrong message shared by all"""
    expected = {('accelerations', 'position shape'): 'positions must have shape (M, 3), got (5, 2)',
                ('accelerations', 'value count'): '29 positions but 28 accelerations',
                ('accelerations', 'weight shape'): 'weights must have shape (29,) or (29, 3), got (29, 4)',
                ('gradients', 'value count'): '29 positions but 28 gradients',
                ('gradients', 'weight shape'): 'weights must have shape (29,) or (29, 4), got (29, 5)',
                ('gradients', 'negative weight'): 'weights must be finite and not negative',
                ('gradients', 'duplicate component'): "gradient components must be distinct, got ('xx', 'xx')",
                ('line_of_sight', 'position shape'): 'positions of the first satellite must have shape (M, 3), got (5, 2)',
                ('line_of_sight', 'value count'): '29 pairs but 28 differences',
                ('line_of_sight', 'weight shape'): 'weights must have shape (29,) or (29, 1), got (29, 2)',
                ('line_of_sight', 'NaN weight'): 'weights must be finite and not negative',
                ('line_of_sight', 'coinciding pair'): '1 pairs have both satellites at the same position: their line of sight is undefined, pass directions',
                ('potentials', 'value count'): '29 positions but 28 potentials',
                ('potentials', 'weight column'): 'weights must have shape (29,), got (29, 1)',
                ('potentials', 'block_points'): 'block_points must be positive, got 0',
                ('potential_differences', 'value count'): '29 pairs but 28 differences',
                ('potential_differences', 'weight shape'): 'weights must have shape (29,) or (29, 1), got (29, 2)'}
    seen = {}
    for kind in KINDS:
        for label, change in _bad_calls(kind):
            seen[(kind, label)] = _message(_from_surfaces(kind)['NormalEquations'], **dict(_good(kind), **change))
    for key, text in expected.items():
        assert seen[key] == text, key
    assert seen[('gradients', 'frames')].startswith('frames must have orthonormal rows: |F F^T - I| is ')
    assert seen[('gradients', 'unknown component')].startswith("unknown gradient component 'yx'")
    assert seen[('line_of_sight', 'direction')].startswith('directions must be finite unit vectors: | |e| - 1 | is 1, above')


def test_the_order_of_the_checks_of_a_call():
    """two faults in one call: the earlier check speaks, on every surface (gradients: components, values, weights, frames)"""
    good = _good('gradients')
    faults = [('components', dict(components=('xx', 'yx'))), ('values', dict(gradients=np.zeros((M, 5)))), ('weights', dict(weights=-np.ones(M))),
              ('frames', dict(frames=1.001 * good['frames'])), ('block_points', dict(block_points=0))]
    surfaces = _from_surfaces('gradients')
    for i, (_, early) in enumerate(faults):
        alone = _message(surfaces['NormalEquations'], **dict(good, **early))
        for _, late in faults[i + 1:]:
            for surface, call in surfaces.items():
                assert _message(call, **dict(good, **early, **late)) == alone, surface
    degrees = dict(BAND, min_degree=9)
    for kind in KINDS:                                                                  # the degrees come before the checks of the kind
        entry = ga.engine.OBSERVATION_KINDS[kind]
        call = getattr(ga.lstsq.NormalEquations, 'from_' + kind)
        assert _message(call, **dict(_good(kind), **{entry.points[0]: np.zeros((5, 2))}), **degrees) == 'min_degree 9 must lie between 0 and max_degree 8'


def test_temporal_parameters_check_once(monkeypatch):
    """a call that sorts its points runs the checks of the kind once, on the arguments as given"""
    engine = ga.engine
    calls = {'check_frames': 0, 'check_positions': 0, 'check_observation_weights': 0}
    for name in calls:
        def counted(*args, _name=name, _checked=getattr(engine, name), **kwargs):
            calls[_name] += 1
            return _checked(*args, **kwargs)
        monkeypatch.setattr(engine, name, counted)
    temporal = _temporal(True)
    for build in (lambda: temporal.from_gradients(weights=np.ones(M), **_good('gradients'), **BAND),
                  lambda: temporal.of_gradients(np.zeros(3 * P), weights=np.ones(M), **_good('gradients'), **BAND)):
        for name in calls:
            calls[name] = 0
        try:
            build()
        except RuntimeError as err:                                                     # no device: every check has run by then
            assert 'no GPU visible' in str(err)
        assert calls == {'check_frames': 1, 'check_positions': 1, 'check_observation_weights': 1}
    with pytest.raises(ValueError, match='29 points but the temporal parameters hold the windows of 30'):
        ga.lstsq.TemporalParameters(np.zeros(30, dtype=np.int64), np.ones((30, 1)), 1).from_potentials(**_good('potentials'), **BAND)


def _design_calls(kind):
    """the design-matrix functions of engine that take the kind, as functions of its per-point arguments, options and weights"""
    engine, basis = ga.engine, _basis()
    if kind == 'gradients':
        return [lambda **kw: engine.gradient_design(8, GM=GM, R=R, min_degree=2, **kw), lambda **kw: engine.rbf_gradient_design(basis, **kw)]
    sh = {'accelerations': engine.acceleration_design, 'line_of_sight': engine.los_design, 'potentials': engine.potential_design,
          'potential_differences': engine.potential_difference_design}[kind]
    rbf = {name: given for given, name in engine.RBF_OBSERVATION_KINDS.items()}[kind]

    def node_values(**kw):
        first = kw.pop('xyz') if 'xyz' in kw else kw.pop('xyz_a')
        return engine.rbf_design(rbf, basis, first, **kw)
    return [lambda **kw: sh(8, GM=GM, R=R, min_degree=2, **kw), node_values]


@pytest.mark.parametrize('kind', KINDS)
def test_engine_and_lstsq_share_the_checks_of_a_kind(kind):
    entry = ga.engine.OBSERVATION_KINDS[kind]
    good = _good(kind)
    surface = _from_surfaces(kind)['NormalEquations']
    unobserved = {name: value for name, value in good.items() if name != entry.observed}
    for label, change in _bad_calls(kind):
        if label in ('value count', 'block_points'):                                    # the design matrix has neither
            continue
        expected = _message(surface, **dict(good, **change))
        for design in _design_calls(kind):
            assert _message(design, **dict(unobserved, **change)) == expected, label


def test_the_table_states_the_call_order_of_every_surface():
    engine, lstsq = ga.engine, ga.lstsq
    assert tuple(engine.OBSERVATION_KINDS) == KINDS and sorted(engine.RBF_OBSERVATION_KINDS.values()) == sorted(set(KINDS) - {'gradients'})
    for kind, entry in engine.OBSERVATION_KINDS.items():
        assert entry.observed in entry.points and entry.points[0] in ('xyz', 'xyz_a')
        listed = list(entry.points) + list(entry.options)
        for owner in (lstsq.NormalEquations, lstsq.ColouredNoise, lstsq.ArcParameters, lstsq.RadialBasisParameters, lstsq.TemporalParameters):
            names = [name for name in inspect.signature(getattr(owner, 'from_' + kind)).parameters if name in listed]
            assert names == listed, (kind, owner)
        for owner in (lstsq.PostFit, lstsq.RadialBasisParameters, lstsq.TemporalParameters):
            names = list(inspect.signature(getattr(owner, 'of_' + kind)).parameters)
            assert [name for name in names if name in listed] == listed and 'solution' in names[:2], (kind, owner)
