"""
CPU checks of the design matrices with respect to the node values of radial basis functions: shg_rbf_design rejects bad arguments
before any HIP call, shg_rbf_design_info is sane, RadialBasisFunctions.degree_factors tells isotropic shapes from others, the Python
layers refuse bad input before anything reaches the device, RadialBasisFunctions still has the reference's members, and the fixture
g29_radial_basis.npz is consistent with itself and with the float64 NumPy restatement of the kernel.
"""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest

import grates_amd as ga
import rbf_inputs as ri
from conftest import GOLDEN

GM, R = ri.GM, ri.R


def _error(lib):
    return lib.shg_last_error().decode()


def _basis(tag='b2_8', flat=False):
    min_degree, max_degree = ri.CASES[tag][:2]
    lon, lat = ri.case_nodes(tag)
    K = ri.shape_factors(ri.degree_factors(min_degree, max_degree, flat))
    return ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat), K, min_degree, max_degree, GM, R)


def test_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    shape = (ctypes.c_double * 9)(*([1.0] * 9))

    def call(kind=0, N=8, min_degree=2, shape=shape, nodes=dummy, J=5, a=dummy, b=dummy, e=None, M=10, w=None, wl=0, gm=GM, r=R, At=dummy, ldt=10):
        return lib.shg_rbf_design(kind, N, min_degree, shape, nodes, J, a, b, e, M, w, wl, gm, r, At, ldt, None)
    for kind in (-1, 4):
        assert call(kind=kind) == -1
        assert 'shg_rbf_design: kind {0}'.format(kind) in _error(lib)
    for bad in (dict(N=-1, min_degree=0), dict(min_degree=-1), dict(J=-1), dict(M=-1, ldt=0)):
        assert call(**bad) == -1
        assert 'shg_rbf_design: negative size' in _error(lib)
    assert call(N=4, min_degree=5) == -1
    assert 'min_degree 5 above N 4' in _error(lib)
    assert call(N=32768) == -1
    assert 'N 32768 is too large' in _error(lib)
    most = ga.engine.rbf_design_info()[3]
    assert call(J=most + 1) == -1
    assert 'above the {0} nodes of one call'.format(most) in _error(lib)
    for kind, wl in ((0, 3), (0, -1), (1, 2), (2, 2), (3, 2)):
        assert call(kind=kind, w=dummy, wl=wl) == -1
        assert 'weight layout {0}'.format(wl) in _error(lib)
    for gm, r in ((float('nan'), R), (float('inf'), R), (GM, 0.0), (GM, -R), (GM, float('inf')), (GM, float('nan'))):
        assert call(gm=gm, r=r) == -1
        assert 'GM and R must be finite and R positive' in _error(lib)
    assert call(ldt=9) == -1
    assert 'ldt 9 below M 10' in _error(lib)
    assert call(J=1 << 19, M=1 << 21, ldt=1 << 21) == -1                                      # 3 x 2^40 values
    assert 'is too large' in _error(lib)
    for kind in range(4):
        for missing in ('shape', 'nodes', 'a', 'At'):
            assert call(kind=kind, **{missing: None}) == -1
            assert 'shg_rbf_design: NULL pointer' in _error(lib)
        assert call(kind=kind, w=None, wl=1) == -1
        assert 'shg_rbf_design: NULL pointer' in _error(lib)
    for kind in (1, 3):
        assert call(kind=kind, b=None) == -1
        assert 'a pair kind needs the positions of the second satellite' in _error(lib)
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(M=0, ldt=0, shape=None, nodes=None, a=None, b=None, At=None) == 0
    assert call(J=0, shape=None, nodes=None, a=None, b=None, At=None) == 0
    with pytest.raises(_lib.ShgError, match='min_degree 3 above N 2'):
        _lib.call('shg_rbf_design', 0, 2, 3, shape, dummy, 5, dummy, None, None, 10, None, 0, GM, R, dummy, 10, None)


def test_info_is_sane():
    from grates_amd import _lib
    tile, unroll, lanes, most = ga.engine.rbf_design_info()
    assert lanes == 256 and 1 <= unroll <= tile <= 256 and tile % unroll == 0
    assert most == 65535 * tile
    assert _lib.load().shg_rbf_design_info(None) == -1
    assert 'shg_rbf_design_info: NULL pointer' in _error(_lib.load())
    assert 'shg_rbf_design' in _lib.PROTOTYPES and 'shg_rbf_design_info' in _lib.PROTOTYPES


def test_degree_factors_of_isotropic_and_other_shapes():
    for tag in ri.CASES:
        min_degree, max_degree = ri.CASES[tag][:2]
        basis = _basis(tag)
        k = ri.degree_factors(min_degree, max_degree)
        assert np.array_equal(basis.degree_factors, k) and basis.degree_factors.shape == (max_degree + 1,)
        assert (basis.min_degree, basis.max_degree) == (min_degree, max_degree)
        assert np.array_equal(basis.shape_factors, ri.shape_factors(k))
        basis.shape_factors[2, 1] = 7.0                                                 # a copy: the basis keeps its own
        assert np.array_equal(basis.shape_factors, ri.shape_factors(k))
        for name in ('min_degree', 'max_degree', 'shape_factors', 'degree_factors'):
            with pytest.raises(AttributeError):
                setattr(basis, name, 3)
    lon, lat = ri.case_nodes('b2_8')
    for slot in ((3, 5), (0, 8), (5, 2), (8, 8), (8, 0)):                              # S_53 at [m - 1, n] = [2, 5] is (2, 5); a mix of C and S slots
        K = ri.shape_factors(ri.degree_factors(2, 8))
        K[slot] = np.nextafter(K[slot], 1.0)                                            # one slot, one bit
        basis = ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat), K, 2, 8, GM, R)
        with pytest.raises(ValueError, match='to_potential_coefficients_matrix'):
            basis.degree_factors
        with pytest.raises(ValueError, match='isotropic'):
            ga.lstsq.RadialBasisParameters(basis)
        with pytest.raises(ValueError, match='isotropic'):
            ga.gravityfield.rbf_acceleration_design_matrix(basis, ri.positions('b2_8'))
    K = ri.shape_factors(ri.degree_factors(2, 8))
    K[1, 4] = -0.0 if K[1, 4] == 0.0 else -K[1, 4]                                      # S_42: equal in value or not, the bits differ
    with pytest.raises(ValueError, match='degree 4'):
        ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat), K, 2, 8, GM, R).degree_factors
    with pytest.raises(ValueError, match='do not hold degrees'):
        ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat), np.ones((8, 8)), 2, 8, GM, R).degree_factors


def test_basis_mismatch_is_refused_before_the_device():
    basis = _basis('b2_8')
    a, b = ri.pairs('b2_8')
    M = a.shape[0]
    lstsq = ga.lstsq
    Band = ga.engine.Band
    builders = (lambda **kw: lstsq._observations('accelerations', dict(xyz=a, g=np.zeros((M, 3)), weights=None), Band(basis=basis, **kw)),
                lambda **kw: lstsq._observations('line_of_sight', dict(xyz_a=a, xyz_b=b, differences=np.zeros(M), directions=ri.directions('b2_8'),
                                                                       weights=None), Band(basis=basis, **kw)),
                lambda **kw: lstsq._observations('potentials', dict(xyz=a, potentials=np.zeros(M), weights=None), Band(basis=basis, **kw)),
                lambda **kw: lstsq._observations('potential_differences', dict(xyz_a=a, xyz_b=b, differences=np.zeros(M), weights=None),
                                                 Band(basis=basis, **kw)))
    good = dict(min_degree=2, max_degree=8, GM=GM, R=R)
    for build in builders:
        observations = build(**good)
        assert observations.P == 24 and observations.design_block is None               # nothing uploaded yet
        for name, value, shown in (('min_degree', 3, '3'), ('max_degree', 9, '9'), ('GM', GM * (1 + 1e-15), repr(GM * (1 + 1e-15))), ('R', R + 1.0, repr(R + 1.0))):
            with pytest.raises(ValueError) as err:
                build(**dict(good, **{name: value}))
            own = {'min_degree': '2', 'max_degree': '8', 'GM': repr(GM), 'R': repr(R)}[name]
            assert name in str(err.value) and shown in str(err.value) and own in str(err.value)      # both values are named
    plain = lstsq._observations('accelerations', dict(xyz=a, g=np.zeros((M, 3)), weights=None), Band(**good))
    assert plain.P == 81 - 4


def test_python_checks_run_before_the_device():
    basis = _basis('b2_8')
    bound = ga.lstsq.RadialBasisParameters(basis)
    a, b = ri.pairs('b2_8')
    M = a.shape[0]
    gf, engine = ga.gravityfield, ga.engine
    for shape in ((5,), (5, 2), (2, 5, 3)):
        bad = np.zeros(shape)
        for route in (lambda x: gf.rbf_acceleration_design_matrix(basis, x), lambda x: gf.rbf_potential_design_matrix(basis, x),
                      lambda x: basis.gravitational_acceleration(x), lambda x: basis.gravitational_potential(x),
                      lambda x: bound.from_accelerations(x, np.zeros((5, 3))), lambda x: bound.from_potentials(x, np.zeros(5)),
                      lambda x: bound.of_accelerations(np.zeros(24), x, np.zeros((5, 3)))):
            with pytest.raises(ValueError, match=r'positions must have shape \(M, 3\)'):
                route(bad)
        for route in (lambda x: gf.rbf_line_of_sight_design_matrix(basis, x, b), lambda x: gf.rbf_potential_difference_design_matrix(basis, x, b),
                      lambda x: basis.line_of_sight_acceleration(x, b), lambda x: basis.potential_difference(x, b),
                      lambda x: bound.from_line_of_sight(x, b, np.zeros(M)), lambda x: bound.from_potential_differences(x, b, np.zeros(M))):
            with pytest.raises(ValueError, match=r'positions of the first satellite must have shape \(M, 3\)'):
                route(bad)
    with pytest.raises(ValueError, match='29 positions of the first satellite but 28 of the second'):
        gf.rbf_potential_difference_design_matrix(basis, a, b[:28])
    with pytest.raises(ValueError, match='both satellites at the same position'):
        gf.rbf_line_of_sight_design_matrix(basis, a, b)                                 # pair 26 coincides and no directions are given
    with pytest.raises(ValueError, match='directions must be finite unit vectors'):
        gf.rbf_line_of_sight_design_matrix(basis, a, b, directions=2.0 * ri.directions('b2_8'))
    with pytest.raises(ValueError, match=r'weights must have shape \(29,\) or \(29, 3\)'):
        gf.rbf_acceleration_design_matrix(basis, a, weights=np.ones((29, 2)))
    for route in (lambda w: gf.rbf_potential_design_matrix(basis, a, weights=w), lambda w: gf.rbf_potential_difference_design_matrix(basis, a, b, weights=w),
                  lambda w: gf.rbf_line_of_sight_design_matrix(basis, a, b, ri.directions('b2_8'), weights=w),
                  lambda w: bound.from_potentials(a, np.zeros(M), weights=w)):
        with pytest.raises(ValueError, match=r'weights must have shape \(29,\)'):
            route(np.ones((29, 3)))
        with pytest.raises(ValueError, match='weights must be finite and not negative'):
            route(-np.ones(29))
    with pytest.raises(ValueError, match='unknown kind'):
        engine.rbf_design('gradients', basis, a)
    with pytest.raises(ValueError, match='needs the positions of the second satellite'):
        engine.rbf_design('potential_difference', basis, a)
    with pytest.raises(ValueError, match='29 positions but 28 accelerations'):
        bound.from_accelerations(a, np.zeros((28, 3)))
    with pytest.raises(ValueError, match='block_points must be positive'):
        bound.from_accelerations(a, np.zeros((M, 3)), block_points=0)
    with pytest.raises(ValueError, match=r'solution must have shape \(24,\)'):
        bound.of_accelerations(np.zeros(77), a, np.zeros((M, 3)))                       # the node count, not the coefficient count
    with pytest.raises(ValueError, match='model must be None, a ColouredNoise or an ArcParameters'):
        ga.lstsq.RadialBasisParameters(basis, model='white')
    arcs = ga.lstsq.ArcParameters(ga.lstsq.arc_basis([0, 10], 28, degree=0), [0, 10])
    with pytest.raises(ValueError, match=r'the arc basis must have shape \(29, u\)'):
        ga.lstsq.RadialBasisParameters(basis, arcs).from_potentials(a, np.zeros(M))


def test_signatures():
    def names(function):
        return list(inspect.signature(function).parameters)
    gf, engine, lstsq = ga.gravityfield, ga.engine, ga.lstsq
    assert names(engine.rbf_design) == ['kind', 'basis', 'xyz', 'xyz_b', 'directions', 'weights']
    assert names(engine.rbf_design_checked) == ['kind', 'basis', 'a', 'b', 'directions', 'weights']
    assert names(gf.rbf_acceleration_design_matrix) == ['basis', 'xyz', 'weights', 'as_tensor']
    assert names(gf.rbf_line_of_sight_design_matrix) == ['basis', 'xyz_a', 'xyz_b', 'directions', 'weights', 'as_tensor']
    assert names(gf.rbf_potential_design_matrix) == ['basis', 'xyz', 'weights', 'as_tensor']
    assert names(gf.rbf_potential_difference_design_matrix) == ['basis', 'xyz_a', 'xyz_b', 'weights', 'as_tensor']
    assert names(lstsq._observations) == ['kind', 'arguments', 'band']                 # one builder for every kind; the basis is the band's
    last = list(inspect.signature(engine.Band).parameters.values())[-1]
    assert (last.name, last.default) == ('basis', None)
    assert names(lstsq.RadialBasisParameters) == ['basis', 'model']
    tail = ['weights', 'block_points']
    bound, field = lstsq.RadialBasisParameters, gf.PotentialCoefficients
    for kind, first in (('accelerations', ['xyz', 'g']), ('line_of_sight', ['xyz_a', 'xyz_b', 'differences', 'directions']),
                        ('potentials', ['xyz', 'potentials']), ('potential_differences', ['xyz_a', 'xyz_b', 'differences'])):
        assert names(getattr(bound, 'from_' + kind)) == ['self'] + first + tail
        assert names(getattr(bound, 'of_' + kind)) == ['self', 'solution'] + first + tail + ['vectors']
    for name in ('gravitational_acceleration', 'gravitational_potential', 'line_of_sight_acceleration', 'potential_difference'):
        assert names(getattr(gf.RadialBasisFunctions, name)) == names(getattr(field, name))      # the functionals of the coefficients' class


def test_radial_basis_functions_keeps_the_reference_members():
    """every member the reference's class has is still there with its parameters; the new members are additions"""
    with open(os.path.join(GOLDEN, 'g19_api.json')) as f:
        recorded = json.load(f)['modules']['gravityfield']['RadialBasisFunctions']['members']
    cls = ga.gravityfield.RadialBasisFunctions
    assert len(recorded) >= 7
    for name, record in recorded.items():
        assert hasattr(cls, name), name
        member = inspect.getattr_static(cls, name)
        if isinstance(record, str):
            assert isinstance(member, property) and ('+setter' in record) <= (member.fset is not None), name
        elif record:
            own = list(inspect.signature(getattr(cls, name)).parameters)
            assert own[:len(record)] == [prm[0] for prm in record], name
    added = {'min_degree', 'max_degree', 'shape_factors', 'degree_factors', 'gravitational_acceleration', 'gravitational_potential',
             'line_of_sight_acceleration', 'potential_difference'}
    assert added <= set(dir(cls)) and not added & set(recorded)
    for name in ('min_degree', 'max_degree', 'shape_factors', 'degree_factors'):
        assert isinstance(inspect.getattr_static(cls, name), property) and inspect.getattr_static(cls, name).fset is None
    copy = _basis().copy()
    assert np.array_equal(copy.degree_factors, _basis().degree_factors) and (copy.min_degree, copy.max_degree) == (2, 8)


def test_node_table_matches_the_package_geometry():
    """rbf_inputs.node_table spells out utilities.colatitude and geocentric_radius: the same bits"""
    for lon, lat, a, f in ((*ri.case_nodes('b2_8'), ri.A, ri.F), ri.loop_nodes()):
        nodes = ri.node_table(lon, lat, a, f)
        colat, radius = ga.utilities.colatitude(lat, a, f), ga.utilities.geocentric_radius(lat, a, f)
        assert np.array_equal(nodes[:, 3], R / radius)
        assert np.array_equal(nodes[:, :3], np.stack((np.sin(colat) * np.cos(lon), np.sin(colat) * np.sin(lon), np.cos(colat)), axis=1))
        assert np.abs(np.sqrt(np.sum(nodes[:, :3] ** 2, axis=1)) - 1.0).max() < 4e-16
    lon, lat, a, f = ri.loop_nodes()
    assert lon.size == 48 and np.allclose(R / ri.node_table(lon, lat, a, f)[:, 3], R - 10e3, rtol=1e-15)


def test_fixture_geometry(golden):
    data = golden('g29_radial_basis')
    for tag, (min_degree, max_degree, count, _) in ri.CASES.items():
        a, b, e = data['xyz_a_' + tag], data['xyz_b_' + tag], data['e_' + tag]
        assert np.array_equal(a, ri.pairs(tag)[0]) and np.array_equal(b, ri.pairs(tag)[1]) and np.array_equal(e, ri.directions(tag))
        assert a.shape == (29, 3) and data['lon_' + tag].shape == (count,)
        assert np.array_equal(data['lon_' + tag], ri.case_nodes(tag)[0]) and np.array_equal(data['lat_' + tag], ri.case_nodes(tag)[1])
        k = data['k_' + tag]
        assert np.array_equal(k, ri.degree_factors(min_degree, max_degree)) and np.all(k[:min_degree] == 0.0) and np.all(k[min_degree:] > 0.0)
        nodes = ri.node_table(data['lon_' + tag], data['lat_' + tag])
        xh = a / np.sqrt(np.sum(a * a, axis=1))[:, None]
        t = xh[20:] @ nodes[:3, :3].T                                                    # the nine special points against the first three nodes
        for j in range(3):
            assert abs(t[3 * j, j] - 1.0) <= 2.3e-16 and abs(t[3 * j + 1, j] + 1.0) <= 2.3e-16             # above, antipodal
            assert 0.0 < 1.0 - t[3 * j + 2, j] < 2e-14                                                   # 1 m beside: t = 1 - 1e-14
        sep = np.sqrt(np.sum((b - a) ** 2, axis=1))
        assert np.array_equal(sep == 0.0, ri.separations() == 0.0) and np.count_nonzero(sep == 0.0) == 1
        assert np.abs(np.sqrt(np.sum(e * e, axis=1)) - 1.0).max() <= 1e-15
        assert data['A_acc_' + tag].shape == (87, count) and data['A_los_' + tag].shape == data['A_pot_' + tag].shape == data['A_dif_' + tag].shape == (29, count)
        assert np.all(data['A_dif_' + tag][sep == 0.0] == 0.0) and np.all(data['A_los_' + tag][sep == 0.0] == 0.0)
    assert data['A_acc_n96'].shape == (900, 8) and np.array_equal(data['xyz_n96'], ri.n96_positions())
    assert np.array_equal(data['k_n96'], ri.degree_factors(2, 96, flat=True))
    heights = np.sqrt(np.sum(ri.loop_positions()[0] ** 2, axis=1)) - R
    assert heights.min() > 249e3 and heights.max() < 501e3 and np.unique(np.round(heights)).size == 8


def test_fixture_matches_the_restatement(golden):
    """The recorded scalars are what this machine computes.  Recorded: 1e-14 of max|A| at most off the axis at d/o 8 and 2 (4e-10 at
    the point 1 mm off it, the reference's own loss), 1.1e-13 at d/o 96, forward 6.7e-15 and 4.3e-15, host loops 1.7e-14, 1.3e-14 and
    6.2e-14 at cond(A) 19, 19 and 51; the GPU tests take 4 times (the loops: 10 times) these figures as their bounds."""
    data = golden('g29_radial_basis')
    for tag, (min_degree, max_degree, _, _) in ri.CASES.items():
        nodes, k = ri.node_table(data['lon_' + tag], data['lat_' + tag]), data['k_' + tag]
        a, b, e = data['xyz_a_' + tag], data['xyz_b_' + tag], data['e_' + tag]
        scales = {'acc': data['acc_scale_' + tag], 'los': data['acc_scale_' + tag], 'pot': data['pot_scale_' + tag], 'dif': data['pot_scale_' + tag]}
        for i, kind in enumerate(ri.KINDS):
            rows = ri.point_errors(ri.restatement(kind, nodes, k, min_degree, a, b, e), data['A_{0}_{1}'.format(kind, tag)]) / float(scales[kind])
            off_axis, axis = np.delete(rows, ri.NEAR_AXIS).max(), rows[ri.NEAR_AXIS]
            print('{0} {1}: restatement {2:.2e}, at the point 1 mm off the axis {3:.2e}'.format(tag, kind, off_axis, axis))
            assert off_axis <= 2 * data['restatement_err_' + tag][i] and axis <= 2 * data['axis_err_' + tag][i]
        assert np.all(data['restatement_err_' + tag] <= 2e-14) and np.all(data['axis_err_' + tag] <= 1e-9)
        # the family against itself, in NumPy: the pair kinds are made of the single-point values
        Va, ga_ = ri.chains(a, nodes, k, min_degree)
        Vb, gb = ri.chains(b, nodes, k, min_degree)
        assert np.array_equal(ri.restatement('dif', nodes, k, min_degree, a, b), Vb - Va)
        assert np.array_equal(ri.restatement('dif', nodes, k, min_degree, b, a), -(Vb - Va))
    err96 = np.abs(ri.restatement('acc', ri.node_table(data['lon_n96'], data['lat_n96']), data['k_n96'], 2, data['xyz_n96']) - data['A_acc_n96']).max()
    err96 /= float(data['acc_scale_n96'])
    print('n96: restatement {0:.2e}'.format(err96))
    assert err96 <= 2 * float(data['restatement_err_n96']) <= 1e-12
    assert data['forward_err'].shape == (2,) and np.all(data['forward_err'] <= 5e-14)
    assert data['host_rel_err'].shape == data['loop_cond'].shape == (3,)
    assert np.all(data['host_rel_err'] <= 1e-12) and np.all(data['loop_cond'] <= 100.0) and abs(data['loop_cond'][0] - 19.0) < 0.1
