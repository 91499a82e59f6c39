"""
The node values of radial basis functions as parameters, on the GPU: the design matrices of shg_rbf_design (gravityfield.rbf_*_design_matrix,
engine.rbf_design), the forward functionals of RadialBasisFunctions and the normal equations and post-fit pass of
lstsq.RadialBasisParameters: against the reference's conversion to spherical harmonics (tests/golden/g29_radial_basis.npz), against the
spherical harmonic design matrices times to_potential_coefficients_matrix on the GPU (the check that needs no reference), for the
kernel's contracts at its seams (values independent of the batch, the node count, the place in the batch and ldt; weights a scaling;
reproducible; pairs made of the single-point values) and through solve, closed loops on planted node values included.

The bounds against the fixture are 4 times the figures its generator recorded for the float64 restatement (rbf_inputs.restatement: the
kernel has no transcendental function, so it follows the restatement to the last bits), the closed loops 10 times the host's.
"""
import ctypes
import functools

import numpy as np
import pytest

import grates_amd as ga
import rbf_inputs as ri
import whitening_inputs as wi

pytestmark = pytest.mark.gpu

GM, R = ri.GM, ri.R
U = 2.0 ** -53
KIND_NAMES = dict(zip(ri.KINDS, ga.engine.RBF_KINDS))


def _host(t):
    return t if isinstance(t, np.ndarray) else ga.engine.to_host(t)


def _basis(lon, lat, k, min_degree, a=ri.A, f=ri.F):
    return ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat, a=a, f=f), ri.shape_factors(k), min_degree, k.size - 1, GM, R)


def _matrix(kind, basis, a, b=None, e=None, **kwargs):
    """A [K M, J] of `kind` (one of rbf_inputs.KINDS) through the public design matrix functions"""
    gf = ga.gravityfield
    if kind == 'acc':
        return gf.rbf_acceleration_design_matrix(basis, a, **kwargs)
    if kind == 'los':
        return gf.rbf_line_of_sight_design_matrix(basis, a, b, e, **kwargs)
    if kind == 'pot':
        return gf.rbf_potential_design_matrix(basis, a, **kwargs)
    return gf.rbf_potential_difference_design_matrix(basis, a, b, **kwargs)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', sorted(ri.CASES))
def test_design_matrices_match_the_reference(golden, tag):
    data = golden('g29_radial_basis')
    min_degree = ri.CASES[tag][0]
    basis = _basis(data['lon_' + tag], data['lat_' + tag], data['k_' + tag], min_degree)
    a, b, e = data['xyz_a_' + tag], data['xyz_b_' + tag], data['e_' + tag]
    scales = {'acc': data['acc_scale_' + tag], 'los': data['acc_scale_' + tag], 'pot': data['pot_scale_' + tag], 'dif': data['pot_scale_' + tag]}
    failures = []
    for i, kind in enumerate(ri.KINDS):
        A, ref = _matrix(kind, basis, a, b, e), data['A_{0}_{1}'.format(kind, tag)]
        assert isinstance(A, np.ndarray) and A.shape == ref.shape and np.all(np.isfinite(A))
        rows = ri.point_errors(A, ref) / float(scales[kind])
        off_axis, axis = np.delete(rows, ri.NEAR_AXIS).max(), rows[ri.NEAR_AXIS]
        bound, axis_bound = 4 * data['restatement_err_' + tag][i], 4 * data['axis_err_' + tag][i]
        restated = np.abs(A - ri.restatement(kind, ri.node_table(data['lon_' + tag], data['lat_' + tag]), data['k_' + tag], min_degree, a, b, e)).max()
        print('{0} {1}: {2:.2e} of max|A| (bound {3:.2e}); 1 mm off the axis {4:.2e} (bound {5:.2e}); {6:.2e} from the restatement'.format(
            tag, kind, off_axis, bound, axis, axis_bound, restated / float(scales[kind])))
        if not (off_axis <= bound and axis <= axis_bound and restated == 0.0):     # the kernel follows the restatement to the last bit
            failures.append(kind)
    assert not failures


def test_degree_96_matches_the_reference(golden):
    data = golden('g29_radial_basis')
    basis = _basis(data['lon_n96'], data['lat_n96'], data['k_n96'], ri.N96['min_degree'])
    A = ga.gravityfield.rbf_acceleration_design_matrix(basis, data['xyz_n96'])
    err = np.abs(A - data['A_acc_n96']).max() / float(data['acc_scale_n96'])
    print('d/o 96, 300 points, 8 nodes: {0:.2e} of max|A_acc| (bound {1:.2e})'.format(err, 4 * float(data['restatement_err_n96'])))
    assert A.shape == (900, 8) and err <= 4 * float(data['restatement_err_n96'])


# ---- the check that needs no reference ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forward_case():
    c = ri.FORWARD
    basis = _basis(*ri.forward_nodes(), ri.degree_factors(c['min_degree'], c['max_degree']), c['min_degree'])
    basis.values = ri.forward_values()
    return basis, ri.forward_positions()


def test_columns_are_the_spherical_harmonic_columns_times_the_transformation():
    """A_rbf = A_sh(min_degree .. max_degree) F with F = to_potential_coefficients_matrix(), both sides from the GPU.  The bound: an
    entry of A_sh is within 5e-14 of max|A_sh| (the bound of its own suites), F (Legendre functions of degree 12 and powers of R / r)
    within 1e-14 of its entries, the product adds (P + 2) 2^-53 = 2e-14 and A_rbf itself is within 2e-14 (the fixture): 1e-13 of
    S = max|A_sh| max_j sum_p |F_pj|, the size of the sums that cancel down to A_rbf."""
    basis, xyz = _forward_case()
    c = ri.FORWARD
    F = basis.to_potential_coefficients_matrix()
    assert F.shape == ((c['max_degree'] + 1) ** 2 - c['min_degree'] ** 2, c['nodes'])
    for kind, design in (('acc', ga.gravityfield.acceleration_design_matrix), ('pot', ga.gravityfield.potential_design_matrix)):
        A_sh = design(xyz, c['min_degree'], c['max_degree'], GM, R, as_tensor=True)
        composed = _host(ga.engine.gemm(A_sh, ga.engine.to_device(F)))
        A = _matrix(kind, basis, xyz)
        scale = float(A_sh.abs().max().item()) * np.abs(F).sum(axis=0).max()
        err = np.abs(A - composed).max()
        print('{0}: {1:.2e} of S, {2:.2e} of max|A_rbf| (S / max|A_rbf| = {3:.1f})'.format(kind, err / scale, err / np.abs(A).max(), scale / np.abs(A).max()))
        assert A.shape == composed.shape and err <= 1e-13 * scale


def test_forward_functionals_match_the_spherical_harmonic_route(golden):
    """rbf.gravitational_acceleration and .gravitational_potential against the GPU functionals of rbf.to_potential_coefficients() (K is
    zero below degree 2, so the conversion holds the band and nothing else)"""
    import torch
    data = golden('g29_radial_basis')
    basis, xyz = _forward_case()
    field = basis.to_potential_coefficients()
    for i, name in enumerate(('gravitational_acceleration', 'gravitational_potential')):
        mine, theirs = getattr(basis, name)(xyz), _host(getattr(field, name)(xyz, as_tensor=True))
        assert isinstance(mine, np.ndarray) and mine.shape == theirs.shape == ((300, 3) if i == 0 else (300,))
        on_device = getattr(basis, name)(ga.engine.to_device(xyz), as_tensor=True)
        assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and np.array_equal(_host(on_device), mine)
        err = np.abs(mine - theirs).max() / np.abs(theirs).max()
        print('{0}: {1:.2e} of the largest value (bound {2:.2e})'.format(name, err, 4 * float(data['forward_err'][i])))
        assert err <= 4 * float(data['forward_err'][i])
    a, b = xyz[:150], xyz[150:]
    g, V = basis.gravitational_acceleration(xyz), basis.gravitational_potential(xyz)
    d = b - a
    e = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    los, dif = basis.line_of_sight_acceleration(a, b), basis.potential_difference(a, b)
    assert los.shape == dif.shape == (150,)
    # sums over 40 nodes of entries that agree within 4 ulp of max|A_acc| (see test_pairs_are_made_of_the_single_point_values)
    assert np.abs(los - ri.project(e, g[150:], g[:150])).max() <= 4 * float(data['forward_err'][0]) * np.abs(g).max()
    assert np.abs(dif - (V[150:] - V[:150])).max() <= 4 * float(data['forward_err'][1]) * np.abs(V).max()


# ---- seams and contracts ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seam_case():
    """band 2..8, T + U + 1 nodes, 700 pairs (two full workgroups and a partial one), explicit lines of sight"""
    tile, unroll = ga.engine.rbf_design_info()[:2]
    J = tile + unroll + 1
    lon, lat = ri.scattered_nodes(J, 2941)
    a = ri.ai.scattered_positions(700, 2942)
    d = np.random.default_rng(2943).standard_normal(a.shape)
    d = d / np.sqrt(np.sum(d * d, axis=1))[:, None]
    return lon, lat, ri.degree_factors(2, 8), a, a + ri.SEPARATION * d, d


def _seam_basis(J):
    lon, lat, k = _seam_case()[:3]
    return _basis(lon[:J], lat[:J], k, 2)


def _rows(kind, J, a, b, e, weights=None):
    """At [J, K, M] (K = 1 kept as an axis) on the host"""
    At = ga.engine.rbf_design(KIND_NAMES[kind], _seam_basis(J), a, b if kind in ('los', 'dif') else None, e if kind == 'los' else None, weights)
    return _host(At).reshape(J, -1, a.shape[0])


@pytest.mark.parametrize('kind', ri.KINDS)
def test_entries_do_not_depend_on_the_batch(kind):
    """M in {1, 255, 256, 257, 700} and J in {1, T - 1, T, T + 1, T + U + 1}: the entries of a point and a node are the same bits
    whatever the batch, the node count and the place of the point in the batch; two runs are bit-identical"""
    tile, unroll = ga.engine.rbf_design_info()[:2]
    lon, lat, k, a, b, e = _seam_case()
    full = _rows(kind, tile + unroll + 1, a, b, e)
    assert np.all(np.isfinite(full)) and np.all(np.abs(full).max(axis=(1, 2)) > 0)
    assert np.array_equal(full, _rows(kind, tile + unroll + 1, a, b, e))
    for J in (1, tile - 1, tile, tile + 1, tile + unroll + 1):
        for M in (1, 255, 256, 257, 700):
            assert np.array_equal(_rows(kind, J, a[:M], b[:M], e[:M]), full[:J, :, :M]), (J, M)
    for first, last in ((699, 700), (256, 700), (300, 557), (1, 258)):
        assert np.array_equal(_rows(kind, tile + 1, a[first:last], b[first:last], e[first:last]), full[:tile + 1, :, first:last]), (first, last)
    order = np.random.default_rng(2944).permutation(700)
    assert np.array_equal(_rows(kind, tile + unroll + 1, a[order], b[order], e[order]), full[:, :, order])


@pytest.mark.parametrize('kind', ri.KINDS)
def test_leading_dimension_beyond_the_points(kind):
    """ldt > M through the C entry point: the same bits, and the entries from M to ldt of a row are not touched"""
    import torch
    from grates_amd import _lib
    tile = ga.engine.rbf_design_info()[0]
    J, M, ldt = tile + 1, 257, 300
    lon, lat, k, a, b, e = _seam_case()
    basis = _seam_basis(J)
    shape, nodes = ga.engine.rbf_node_table(basis)
    K = 3 if kind == 'acc' else 1
    da, db, de = (ga.engine.to_device(x[:M]) for x in (a, b, e))
    out = torch.full((J, K, ldt), 7.0, dtype=torch.float64, device=da.device)
    _lib.call('shg_rbf_design', ri.KINDS.index(kind), 8, 2, ctypes.c_void_p(shape.ctypes.data), ctypes.c_void_p(nodes.data_ptr()), J,
              ctypes.c_void_p(da.data_ptr()), ctypes.c_void_p(db.data_ptr()), ctypes.c_void_p(de.data_ptr()), M, None, 0, GM, R,
              ctypes.c_void_p(out.data_ptr()), ldt, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    out = _host(out)
    assert np.array_equal(out[:, :, :M], _rows(kind, J, a[:M], b[:M], e[:M])) and np.all(out[:, :, M:] == 7.0)


@pytest.mark.parametrize('kind', ri.KINDS)
def test_weights_scale_the_rows(kind):
    """a weighted matrix is bitwise the unweighted one times sqrt(w), a zero weight gives a zero row"""
    tile = ga.engine.rbf_design_info()[0]
    lon, lat, k, a, b, e = _seam_case()
    J, M = tile + 1, 300
    a, b, e = a[:M], b[:M], e[:M]
    plain = _rows(kind, J, a, b, e)
    rng = np.random.default_rng(2945)
    w = rng.uniform(0.1, 10.0, M)
    w[[0, 17, 256, 299]] = 0.0
    weighted = _rows(kind, J, a, b, e, w)
    assert np.array_equal(weighted, plain * np.sqrt(w)[None, None, :]) and np.all(weighted[:, :, w == 0.0] == 0.0)
    assert np.all(np.abs(weighted[:, :, w > 0.0]).max(axis=(0, 1)) > 0)
    if kind == 'acc':
        w3 = rng.uniform(0.1, 10.0, (M, 3))
        w3[5, 1] = w3[256] = 0.0
        weighted = _rows(kind, J, a, b, e, w3)
        assert np.array_equal(weighted, plain * np.sqrt(w3).T[None, :, :]) and np.all(weighted[:, 1, 5] == 0.0) and np.all(weighted[:, :, 256] == 0.0)
        assert np.all(weighted[:, 0, 5] != 0.0)


def test_pairs_are_made_of_the_single_point_values():
    tile, unroll = ga.engine.rbf_design_info()[:2]
    lon, lat, k, a, b, e = _seam_case()
    J = tile + unroll + 1
    acc_a, acc_b = _rows('acc', J, a, None, None), _rows('acc', J, b, None, None)
    pot_a, pot_b = _rows('pot', J, a, None, None), _rows('pot', J, b, None, None)
    dif, los = _rows('dif', J, a, b, None), _rows('los', J, a, b, e)
    # the potential difference is bitwise the difference of the potential kind's rows; swapping negates it exactly
    assert np.array_equal(dif, pot_b - pot_a) and np.array_equal(_rows('dif', J, b, a, None), -dif)
    # the line of sight: the projected difference of the acceleration kind's rows within 4 ulp of max|A_acc| (NumPy and the kernel
    # round the same three products and two sums: the allowance is for nothing but the order of evaluation of a host library)
    d = acc_b - acc_a
    projected = (e[:, 0] * d[:, 0] + e[:, 1] * d[:, 1]) + e[:, 2] * d[:, 2]
    scale = max(np.abs(acc_a).max(), np.abs(acc_b).max())
    err = np.abs(los[:, 0] - projected).max()
    print('line of sight against the projected difference: {0:.2f} ulp of max|A_acc|'.format(err / (scale * 2 * U)))
    assert err <= 4 * (2 * U) * scale
    # explicit directions negate with the swap; the default e = (b - a) / |b - a| is the explicit one and does not
    assert np.array_equal(_rows('los', J, b, a, e), -los)
    implicit = _host(ga.engine.rbf_design('line_of_sight', _seam_basis(J), a, b))
    assert np.array_equal(implicit, _host(ga.engine.rbf_design('line_of_sight', _seam_basis(J), b, a)))
    unit = (b - a) / np.sqrt(((b - a)[:, 0] ** 2 + (b - a)[:, 1] ** 2) + (b - a)[:, 2] ** 2)[:, None]
    assert np.abs(implicit - _rows('los', J, a, b, unit)[:, 0]).max() <= 4 * (2 * U) * scale
    # coincident satellites: exact zeros (the line of sight then needs explicit directions)
    assert np.all(_rows('dif', J, a, a, None) == 0.0) and np.all(_rows('los', J, a, a, e) == 0.0)


# ---- closed loops -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loop():
    """(basis with the planted values, the field of its conversion, a, b): the observations come from the spherical harmonic route"""
    c = ri.LOOP
    lon, lat, a_nodes, f_nodes = ri.loop_nodes()
    basis = _basis(lon, lat, ri.degree_factors(c['min_degree'], c['max_degree']), c['min_degree'], a_nodes, f_nodes)
    basis.values = ri.loop_values()
    a, b = ri.loop_pairs()
    return basis, basis.to_potential_coefficients(), a, b


def _relative_error(solution, truth):
    x = _host(solution)[:, 0]
    return np.linalg.norm(x - truth) / np.linalg.norm(truth), x


def test_closed_loop_of_accelerations(golden):
    data = golden('g29_radial_basis')
    basis, field, a, _ = _loop()
    truth = ri.loop_values()
    xyz = ga.engine.to_device(a)
    ne = ga.lstsq.RadialBasisParameters(basis).from_accelerations(xyz, field.gravitational_acceleration(xyz, as_tensor=True))
    assert ne.observation_count == 1800 and ne.right_hand_side.shape == (48, 1)
    rel, x = _relative_error(ne.solve(), truth)
    print('closed loop, accelerations: relative error {0:.2e} (host {1:.2e}, cond(A) {2:.0f})'.format(rel, data['host_rel_err'][0], data['loop_cond'][0]))
    assert rel <= 10 * float(data['host_rel_err'][0])
    # the chain closes: the solved values on a grid are the planted field's
    solved = basis.copy()
    solved.values = x
    grid = ga.grid.GeographicGrid(30, 30)
    mine, planted = solved.to_grid(grid, 'potential').values, basis.to_grid(grid, 'potential').values
    assert np.abs(mine - planted).max() <= 10 * float(data['host_rel_err'][0]) * np.abs(planted).max() * np.sqrt(48)


def test_closed_loop_of_accelerations_and_line_of_sight(golden):
    """orbit and link of one field summed by accumulate_normals: the sum of two positive definite matrices is conditioned no worse
    than the worse of the two, and the host solved the stacked system (host_rel_err[1])"""
    data = golden('g29_radial_basis')
    basis, field, a, b = _loop()
    truth = ri.loop_values()
    bound = ga.lstsq.RadialBasisParameters(basis)
    orbit = bound.from_accelerations(a, field.gravitational_acceleration(a))
    link = bound.from_line_of_sight(a, b, field.line_of_sight_acceleration(a, b))
    alone, _ = _relative_error(link.solve(), truth)
    combined = ga.lstsq.accumulate_normals([orbit, bound.from_line_of_sight(a, b, field.line_of_sight_acceleration(a, b))], [1.0, 1.0])
    assert combined.observation_count == 1800 + 600
    rel, _ = _relative_error(combined.solve(), truth)
    print('closed loop, accelerations and line of sight: relative error {0:.2e} (host {1:.2e}); the link alone {2:.2e}'.format(
        rel, data['host_rel_err'][1], alone))
    assert rel <= 10 * float(data['host_rel_err'][1])


def test_closed_loop_of_potentials_with_arc_constants(golden):
    """from_potentials under ArcParameters(arc_basis(degree=0)): the node values within 10 times the host's error, the planted constant
    of every arc within that error times the size of the observations (a constant takes up what the model misses, at their scale)"""
    data = golden('g29_radial_basis')
    basis, field, a, _ = _loop()
    truth, arcs, constants = ri.loop_values(), ri.loop_arcs(), ri.loop_constants()
    obs = field.gravitational_potential(a) + np.repeat(constants, ri.LOOP['arc_length'])
    model = ga.lstsq.ArcParameters(ga.lstsq.arc_basis(arcs, 600, degree=0), arcs)
    ne = ga.lstsq.RadialBasisParameters(basis, model).from_potentials(a, obs)
    assert ne.observation_count == 600 - 12 and ne.arc_elimination.count == 12
    x = ne.solve()
    rel, _ = _relative_error(x, truth)
    estimated = ne.arc_elimination.parameters(x)[:, 0, 0]
    worst = np.abs(estimated - constants).max() / np.abs(obs).max()
    print('closed loop, potentials with arc constants: relative error {0:.2e} (host {1:.2e}, cond {2:.0f}); constants {3:.2e} of max|l|'.format(
        rel, data['host_rel_err'][2], data['loop_cond'][2], worst))
    assert rel <= 10 * float(data['host_rel_err'][2]) and worst <= 10 * float(data['host_rel_err'][2])


# ---- the machinery is the spherical harmonic route's ---------------------------------------------------------------------------------------
def test_coloured_noise_normals_are_those_of_the_whitened_dense_matrix():
    """ColouredNoise of order 2 over two arcs, three blocks of 256 points with their halos: the normals equal A~^T A~ with A~ the dense
    A_rbf whitened column by column (lstsq.decorrelate) and multiplied by engine.gemm, within 1e-13 of max|N|"""
    basis, field, a, _ = _loop()
    J, M = 48, 600
    arcs = np.array([0, 280])
    obs = field.gravitational_acceleration(a) + np.random.default_rng(2946).standard_normal((M, 3)) * 1e-3
    sequence = ga.lstsq.AutoregressiveModelSequence.from_covariance_function(wi.covariance_function('ar2'))
    model = ga.lstsq.ColouredNoise(sequence, arcs)
    ne = ga.lstsq.RadialBasisParameters(basis, model).from_accelerations(a, obs, block_points=256)
    A = ga.gravityfield.rbf_acceleration_design_matrix(basis, a)                        # [3 M, J], row 3 i + c
    whitened = ga.lstsq.decorrelate(np.hstack((A.reshape(M, 3 * J), obs)), sequence, arcs)
    Aw, lw = whitened[:, :3 * J].reshape(3 * M, J), whitened[:, 3 * J:].reshape(3 * M, 1)
    N_ref = _host(ga.engine.gemm(Aw, Aw, transa=True))
    n_ref = _host(ga.engine.gemm(Aw, lw, transa=True))
    got_N, got_n, got_l, count = ne.to_array()
    err_N, err_n = np.abs(got_N - N_ref).max() / np.abs(N_ref).max(), np.abs(got_n - n_ref).max() / np.abs(n_ref).max()
    print('coloured noise: normals {0:.2e} of max|N|, right-hand side {1:.2e} of max|n|'.format(err_N, err_n))
    assert count == 3 * M and got_N.shape == (J, J) and np.array_equal(got_N, got_N.T)
    assert err_N <= 1e-13 and err_n <= 1e-13 and abs(got_l - float(np.sum(lw * lw))) <= 1e-13 * got_l


def test_post_fit_residuals_are_l_minus_a_x():
    basis, field, a, _ = _loop()
    obs = field.gravitational_acceleration(a) + np.random.default_rng(2947).standard_normal((600, 3)) * 1e-3
    bound = ga.lstsq.RadialBasisParameters(basis)
    ne = bound.from_accelerations(a, obs)
    x = ne.solve()
    fit = bound.of_accelerations(x, a, obs, block_points=256)
    A = ga.gravityfield.rbf_acceleration_design_matrix(basis, a)
    expected = obs - (A @ _host(x)[:, 0]).reshape(600, 3)
    err = np.abs(fit.residuals - expected).max() / np.abs(obs).max()
    print('post-fit residuals: {0:.2e} of max|l|'.format(err))
    assert isinstance(fit.residuals, np.ndarray) and fit.residuals.shape == (600, 3) and err <= 1e-13
    assert np.array_equal(fit.whitened, fit.residuals) and np.array_equal(fit.arcs, [0])
    # residuals within delta = 1e-13 max|l| of each other: their square sums within 2 delta sum|e| (+ n delta^2, nothing at this size)
    assert abs(fit.arc_square_sums[0] - float(np.sum(expected * expected))) <= 2 * 1e-13 * np.abs(obs).max() * np.abs(expected).sum()
