"""
CPU checks of the gradient-tensor design matrix with respect to the node values of radial basis functions: shg_rbf_gradient_design
rejects bad arguments before any HIP call, the Python layers refuse bad input before anything reaches the device, the new functions
have the parameter lists of their counterparts, and the fixture g30_rbf_gradients.npz is consistent with its inputs and with the
float64 NumPy restatement of the kernel.
"""
import ctypes
import inspect

import numpy as np
import pytest

import grates_amd as ga
import gradient_design_inputs as gdi
import rbf_gradient_inputs as rg
import rbf_inputs as ri

GM, R = ri.GM, ri.R


def _error(lib):
    return lib.shg_last_error().decode()


def _basis(tag='b2_8'):
    min_degree, max_degree = ri.CASES[tag][:2]
    lon, lat = ri.case_nodes(tag)
    K = ri.shape_factors(ri.degree_factors(min_degree, max_degree))
    return ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat), K, min_degree, max_degree, GM, R)


def test_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    shape = (ctypes.c_double * 9)(*([1.0] * 9))

    def call(N=8, min_degree=2, shape=shape, nodes=dummy, J=5, x=dummy, M=10, frames=None, components=63, w=None, wl=0, gm=GM, r=R, At=dummy, ldt=10):
        return lib.shg_rbf_gradient_design(N, min_degree, shape, nodes, J, x, M, frames, components, w, wl, gm, r, At, ldt, None)
    for components in (0, 64, -1):
        assert call(components=components) == -1
        assert 'shg_rbf_gradient_design: components {0}'.format(components) in _error(lib)
    for bad in (dict(N=-1, min_degree=0), dict(min_degree=-1), dict(J=-1), dict(M=-1, ldt=0)):
        assert call(**bad) == -1
        assert 'shg_rbf_gradient_design: negative size' in _error(lib)
    assert call(N=4, min_degree=5) == -1
    assert 'min_degree 5 above N 4' in _error(lib)
    assert call(N=32768) == -1
    assert 'N 32768 is too large' in _error(lib)
    most = ga.engine.rbf_design_info()[3]
    assert call(J=most + 1) == -1
    assert 'above the {0} nodes of one call'.format(most) in _error(lib)
    for wl in (3, -1):
        assert call(w=dummy, wl=wl) == -1
        assert 'weight layout {0}'.format(wl) in _error(lib)
    for gm, r in ((float('nan'), R), (float('inf'), R), (GM, 0.0), (GM, -R), (GM, float('inf')), (GM, float('nan'))):
        assert call(gm=gm, r=r) == -1
        assert 'GM and R must be finite and R positive' in _error(lib)
    assert call(ldt=9) == -1
    assert 'ldt 9 below M 10' in _error(lib)
    assert call(J=1 << 18, M=1 << 21, ldt=1 << 21) == -1                                      # 6 x 2^39 values
    assert 'is too large' in _error(lib)
    for frames in (None, dummy):
        for missing in ('shape', 'nodes', 'x', 'At'):
            assert call(frames=frames, **{missing: None}) == -1
            assert 'shg_rbf_gradient_design: NULL pointer' in _error(lib)
        for wl in (1, 2):
            assert call(frames=frames, w=None, wl=wl) == -1
            assert 'shg_rbf_gradient_design: NULL pointer' in _error(lib)
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(M=0, ldt=0, shape=None, nodes=None, x=None, At=None) == 0
    assert call(J=0, shape=None, nodes=None, x=None, At=None) == 0
    with pytest.raises(_lib.ShgError, match='min_degree 3 above N 2'):
        _lib.call('shg_rbf_gradient_design', 2, 3, shape, dummy, 5, dummy, 10, None, 63, None, 0, GM, R, dummy, 10, None)
    assert 'shg_rbf_gradient_design' in _lib.PROTOTYPES


def test_signatures():
    def names(function):
        return list(inspect.signature(function).parameters)

    def defaults(function):
        return [p.default for p in inspect.signature(function).parameters.values() if p.default is not inspect.Parameter.empty]
    gf, engine, lstsq = ga.gravityfield, ga.engine, ga.lstsq
    assert names(engine.rbf_gradient_design) == ['basis', 'xyz', 'frames', 'components', 'weights']
    assert defaults(engine.rbf_gradient_design) == [None, None, None]
    assert names(engine.rbf_gradient_design_checked) == ['basis', 'x', 'frames', 'picked', 'weights'] and not defaults(engine.rbf_gradient_design_checked)
    assert names(gf.rbf_gradient_design_matrix) == ['basis', 'xyz', 'frames', 'components', 'weights', 'as_tensor']
    assert defaults(gf.rbf_gradient_design_matrix) == [None, None, None, False]
    last = list(inspect.signature(engine.Band).parameters.values())[-1]
    assert (last.name, last.default) == ('basis', None)
    bound = lstsq.RadialBasisParameters
    assert names(bound.from_gradients) == ['self', 'xyz', 'gradients', 'frames', 'components', 'weights', 'block_points']
    assert defaults(bound.from_gradients) == [None, None, None, None]
    assert names(bound.of_gradients) == ['self', 'solution', 'xyz', 'gradients', 'frames', 'components', 'weights', 'block_points', 'vectors']
    assert defaults(bound.of_gradients) == [None, None, None, None, None]
    mine, theirs = gf.RadialBasisFunctions.gravitational_gradients, gf.PotentialCoefficients.gravitational_gradients
    assert names(mine) == names(theirs) == ['self', 'xyz', 'as_tensor'] and defaults(mine) == defaults(theirs) == [False]
    # the four kinds of shg_rbf_design are as they were
    assert engine.RBF_KINDS == ('acceleration', 'line_of_sight', 'potential', 'potential_difference')
    with pytest.raises(ValueError, match='unknown kind'):
        engine.rbf_design('gradients', _basis(), rg.positions('b2_8'))
    assert 'not offered' not in lstsq.RadialBasisParameters.__doc__


def test_python_checks_run_before_the_device():
    basis = _basis('b2_8')
    bound = ga.lstsq.RadialBasisParameters(basis)
    xyz = rg.positions('b2_8')
    M = xyz.shape[0]
    frames = rg.frames(M)
    gf, engine = ga.gravityfield, ga.engine
    for shape in ((5,), (5, 2), (2, 5, 3)):
        bad = np.zeros(shape)
        for route in (lambda x: gf.rbf_gradient_design_matrix(basis, x), lambda x: engine.rbf_gradient_design(basis, x),
                      lambda x: basis.gravitational_gradients(x), lambda x: bound.from_gradients(x, np.zeros((5, 6))),
                      lambda x: bound.of_gradients(np.zeros(24), x, np.zeros((5, 6)))):
            with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
                route(bad)
    for route in (lambda f: gf.rbf_gradient_design_matrix(basis, xyz, f), lambda f: bound.from_gradients(xyz, np.zeros((M, 6)), frames=f),
                  lambda f: bound.of_gradients(np.zeros(24), xyz, np.zeros((M, 6)), frames=f)):
        with pytest.raises(ValueError, match=r'frames must have shape \(29, 3, 3\)'):
            route(frames[:28])
        with pytest.raises(ValueError, match='frames must have orthonormal rows'):
            route(1.001 * frames)
    for route in (lambda c: gf.rbf_gradient_design_matrix(basis, xyz, components=c), lambda c: bound.from_gradients(xyz, np.zeros((M, 2)), components=c)):
        with pytest.raises(ValueError, match='unknown gradient component'):
            route(('xx', 'yx'))
        with pytest.raises(ValueError, match='gradient components must be distinct'):
            route(('xx', 'xx'))
    with pytest.raises(ValueError, match='at least one gradient component expected'):
        gf.rbf_gradient_design_matrix(basis, xyz, components=())
    with pytest.raises(ValueError, match=r'weights must have shape \(29,\) or \(29, 6\)'):
        gf.rbf_gradient_design_matrix(basis, xyz, weights=np.ones((29, 4)))
    with pytest.raises(ValueError, match=r'weights must have shape \(29,\) or \(29, 4\)'):
        gf.rbf_gradient_design_matrix(basis, xyz, components=rg.LOOP_COMPONENTS, weights=np.ones((29, 6)))
    with pytest.raises(ValueError, match='weights must be finite and not negative'):
        bound.from_gradients(xyz, np.zeros((M, 6)), weights=-np.ones(29))
    with pytest.raises(ValueError, match=r'gradients must have shape \(M, 4\) or \(M, 3, 3\)'):
        bound.from_gradients(xyz, np.zeros((M, 6)), components=rg.LOOP_COMPONENTS)
    with pytest.raises(ValueError, match='29 positions but 28 gradients'):
        bound.from_gradients(xyz, np.zeros((28, 3, 3)))
    with pytest.raises(ValueError, match='block_points must be positive'):
        bound.from_gradients(xyz, np.zeros((M, 6)), block_points=0)
    with pytest.raises(ValueError, match=r'solution must have shape \(24,\)'):
        bound.of_gradients(np.zeros(77), xyz, np.zeros((M, 6)))                         # the node count, not the coefficient count
    # an anisotropic basis is refused by every route
    K = ri.shape_factors(ri.degree_factors(2, 8))
    K[3, 5] = np.nextafter(K[3, 5], 1.0)
    lon, lat = ri.case_nodes('b2_8')
    other = ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat), K, 2, 8, GM, R)
    for route in (lambda: gf.rbf_gradient_design_matrix(other, xyz), lambda: engine.rbf_gradient_design(other, xyz, frames),
                  lambda: other.gravitational_gradients(xyz)):
        with pytest.raises(ValueError, match='isotropic'):
            route()


def test_basis_mismatch_is_refused_before_the_device():
    basis = _basis('b2_8')
    xyz = rg.positions('b2_8')
    M = xyz.shape[0]

    def build(**kw):
        return ga.lstsq._observations('gradients', dict(xyz=xyz, gradients=np.zeros((M, 4)), frames=rg.frames(M), components=rg.LOOP_COMPONENTS,
                                                        weights=None), ga.engine.Band(basis=basis, **kw))
    good = dict(min_degree=2, max_degree=8, GM=GM, R=R)
    observations = build(**good)
    assert observations.P == 24 and observations.K == 4 and observations.design_block is None      # nothing uploaded yet
    for name, value, shown in (('min_degree', 3, '3'), ('max_degree', 9, '9'), ('GM', GM * (1 + 1e-15), repr(GM * (1 + 1e-15))), ('R', R + 1.0, repr(R + 1.0))):
        with pytest.raises(ValueError) as err:
            build(**dict(good, **{name: value}))
        own = {'min_degree': '2', 'max_degree': '8', 'GM': repr(GM), 'R': repr(R)}[name]
        assert name in str(err.value) and shown in str(err.value) and own in str(err.value)      # both values are named
    plain = ga.lstsq._observations('gradients', dict(xyz=xyz, gradients=np.zeros((M, 6)), frames=None, components=None, weights=None),
                                   ga.engine.Band(**good))
    assert plain.P == 81 - 4


def test_fixture_geometry(golden):
    data = golden('g30_rbf_gradients')
    for tag, (min_degree, max_degree, count, _) in ri.CASES.items():
        xyz, frames = data['xyz_' + tag], data['frames_' + tag]
        assert xyz.shape == (29, 3) and np.array_equal(xyz, ri.pairs(tag)[0]) and np.array_equal(frames, rg.frames(29))
        assert np.array_equal(frames[0], np.eye(3)) and np.abs(np.einsum('iac,ibc->iab', frames, frames) - np.eye(3)).max() <= 1e-14
        assert np.array_equal(data['lon_' + tag], ri.case_nodes(tag)[0]) and np.array_equal(data['lat_' + tag], ri.case_nodes(tag)[1])
        assert np.array_equal(data['k_' + tag], ri.degree_factors(min_degree, max_degree))
        A = data['A_' + tag]
        assert A.shape == (6 * 29, count) and np.all(np.isfinite(A)) and float(data['scale_' + tag]) == np.abs(A).max()
        T = A.reshape(29, 6, count)
        assert np.abs(T[:, 0] + T[:, 3] + T[:, 5]).max() <= 1e-14 * np.abs(A).max()       # the oracle's tensors are trace-free
    c = rg.N60
    assert np.array_equal(data['xyz_n60'], rg.n60_positions()) and data['xyz_n60'].shape == (c['points'], 3)
    assert np.array_equal(data['lon_n60'], rg.n60_nodes()[0]) and np.array_equal(data['frames_n60'], rg.n60_frames())
    assert np.array_equal(data['k_n60'], ri.degree_factors(2, 60, flat=True)) and np.array_equal(data['k_n96'], ri.degree_factors(2, 96, flat=True))
    assert data['A_n96'].shape == (6 * rg.N96['points'], c['nodes'])
    heights = np.sqrt(np.sum(data['xyz_n60'] ** 2, axis=1)) - R
    assert heights.min() > -50e3 and heights.max() < 501e3
    assert int(data['loop_nodes']) == ri.LOOP['nodes'] and rg.bias_indicator().sum() == 4 * 600


def test_fixture_matches_the_restatement(golden):
    """The recorded scalars are what this machine computes.  Recorded: 5.6e-15, 5.9e-15 and 1.3e-15 of max|A| at bands 0..8, 2..8 and
    2..2 (no point apart: the mp oracle has no loss near the axis), 1.4e-13 at d/o 96, forward 9.6e-15 of max|T|, float64 against long
    double 5.2e-15, 3.8e-14, 1.1e-13 and 3.5e-13 at N = 8, 60, 96 and 180, the composition at d/o 60 5.2e-14, the host loop 3.2e-14 at
    cond(A) 19; the GPU tests take 4 times (the loops: 10 times) these figures as their bounds."""
    data = golden('g30_rbf_gradients')
    for tag, (min_degree, max_degree, _, _) in ri.CASES.items():
        nodes, k, xyz = ri.node_table(data['lon_' + tag], data['lat_' + tag]), data['k_' + tag], data['xyz_' + tag]
        A = rg.restatement(nodes, k, min_degree, xyz)
        err = np.abs(A - data['A_' + tag]).max() / float(data['scale_' + tag])
        print('{0}: restatement {1:.2e} of max|A|'.format(tag, err))
        assert err <= 2 * float(data['restatement_err_' + tag]) <= 4e-14
        # the restatement against itself: the rotation is exact for the identity, a subset is the matching rows, weights scale
        frames = data['frames_' + tag]
        rotated = rg.restatement(nodes, k, min_degree, xyz, frames)
        assert np.all(rotated[:6] == A[:6]) and np.abs(rotated - gdi.rotate_rows(A, frames)).max() <= 16 * 2.0 ** -53 * np.abs(A).max()
        assert np.array_equal(rg.restatement(nodes, k, min_degree, xyz, frames, rg.LOOP_COMPONENTS), rotated.reshape(29, 6, -1)[:, [0, 2, 3, 5]].reshape(116, -1))
        w = np.random.default_rng(3051).uniform(0.1, 10.0, 29)
        assert np.array_equal(rg.restatement(nodes, k, min_degree, xyz, frames, weights=w), rotated * np.repeat(np.sqrt(w), 6)[:, None])
    c = rg.N96
    nodes = ri.node_table(data['lon_n60'], data['lat_n60'])
    err96 = np.abs(rg.restatement(nodes, data['k_n96'], 2, data['xyz_n60'][:c['points']]) - data['A_n96']).max() / float(data['scale_n96'])
    print('n96: restatement {0:.2e}'.format(err96))
    assert err96 <= 2 * float(data['restatement_err_n96']) <= 1e-12
    growth = np.array([rg.growth(N) for N in rg.GROWTH_DEGREES])
    print('float64 against long double: {0}'.format(growth))
    if np.finfo(np.longdouble).eps < 2.0 ** -60:                                        # an extended long double, as where the figures were recorded
        assert np.all(growth <= 2 * data['growth'])
    assert data['growth'].shape == (4,) and np.all(np.diff(data['growth']) > 0) and data['growth'][-1] <= 1e-11
    assert float(data['forward_err']) <= 5e-14 and float(data['composition_err_n60']) <= 1e-12
    assert float(data['host_rel_err']) <= 1e-12 and float(data['loop_cond']) <= 1e3
    assert data['arc_rel_err'].shape == (2,) and np.all(data['arc_rel_err'] <= 1e-12) and float(data['arc_cond']) <= 1e3
