"""
The gravitational gradient tensor with the node values of radial basis functions as parameters, on the GPU: the design matrix of
shg_rbf_gradient_design (gravityfield.rbf_gradient_design_matrix, engine.rbf_gradient_design), RadialBasisFunctions.gravitational_gradients
and from_gradients / of_gradients of lstsq.RadialBasisParameters: against the mp oracle's tensors of the reference's conversion to
spherical harmonics (tests/golden/g30_rbf_gradients.npz), bit for bit against the float64 NumPy restatement of the kernel
(rbf_gradient_inputs.restatement), against the spherical harmonic design matrix times to_potential_coefficients_matrix on the GPU at
d/o 60, for the kernel's contracts at its seams and through the normal equations, a closed loop on planted node values included.

The bounds against the fixture are 4 times the figures its generator recorded for the restatement, the closed loop 10 times the host's.
"""
import ctypes
import functools

import numpy as np
import pytest

import grates_amd as ga
import gradient_design_inputs as gdi
import rbf_gradient_inputs as rg
import rbf_inputs as ri
import whitening_inputs as wi

pytestmark = pytest.mark.gpu

GM, R = ri.GM, ri.R
U = 2.0 ** -53
SUBSETS = (('xx',), ('xx', 'yy', 'zz', 'xz'), ('xy', 'yz'))


def _host(t):
    return t if isinstance(t, np.ndarray) else ga.engine.to_host(t)


def _basis(lon, lat, k, min_degree, a=ri.A, f=ri.F):
    return ga.gravityfield.RadialBasisFunctions(ga.grid.IrregularGrid(lon, lat, a=a, f=f), ri.shape_factors(k), min_degree, k.size - 1, GM, R)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', sorted(ri.CASES))
def test_design_matrix_matches_the_oracle_and_the_restatement(golden, tag):
    """Earth-fixed and in the seeded frames, all six components and the subsets: within 4 times the recorded figure of the mp oracle's
    matrix (rotated by gradient_design_inputs.rotate_rows), and 0 from the restatement"""
    data = golden('g30_rbf_gradients')
    min_degree = ri.CASES[tag][0]
    lon, lat, k, xyz, frames, truth = (data[name + '_' + tag] for name in ('lon', 'lat', 'k', 'xyz', 'frames', 'A'))
    basis, nodes = _basis(lon, lat, k, min_degree), ri.node_table(lon, lat)
    scale, bound = float(data['scale_' + tag]), 4 * float(data['restatement_err_' + tag])
    failures = []
    for F in (None, frames):
        for components in (None,) + SUBSETS:
            A = ga.gravityfield.rbf_gradient_design_matrix(basis, xyz, F, components)
            K = 6 if components is None else len(components)
            assert isinstance(A, np.ndarray) and A.shape == (K * 29, lon.size) and np.all(np.isfinite(A))
            err = np.abs(A - gdi.rotate_rows(truth, F, components)).max() / scale
            restated = np.abs(A - rg.restatement(nodes, k, min_degree, xyz, F, components)).max() / scale
            print('{0} frames {1} components {2}: {3:.2e} of max|A| (bound {4:.2e}); {5:.2e} from the restatement'.format(
                tag, F is not None, components, err, bound, restated))
            if not (err <= bound and restated == 0.0):
                failures.append((F is not None, components))
    assert not failures


def test_degree_96_matches_the_oracle(golden):
    data = golden('g30_rbf_gradients')
    c = rg.N96
    basis = _basis(data['lon_n60'], data['lat_n60'], data['k_n96'], c['min_degree'])
    A = ga.gravityfield.rbf_gradient_design_matrix(basis, data['xyz_n60'][:c['points']])
    err, bound = np.abs(A - data['A_n96']).max() / float(data['scale_n96']), 4 * float(data['restatement_err_n96'])
    print('d/o 96, {0} points, 8 nodes: {1:.2e} of max|A| (bound {2:.2e})'.format(c['points'], err, bound))
    assert A.shape == (6 * c['points'], 8) and err <= bound


def test_degree_60_columns_are_the_spherical_harmonic_columns_times_the_transformation(golden):
    """A_rbf = A_sh(2 .. 60) F with F = to_potential_coefficients_matrix(), both sides from the GPU, in the seeded frames.  The bound is
    4 times the larger of the float64 growth of the closed sum at N = 60 (against long double) and the composition's own error, which
    the generator measured on the CPU against the restatement."""
    data = golden('g30_rbf_gradients')
    c = rg.N60
    basis = _basis(data['lon_n60'], data['lat_n60'], data['k_n60'], c['min_degree'])
    xyz, frames = data['xyz_n60'], data['frames_n60']
    F = basis.to_potential_coefficients_matrix()
    bound = 4 * max(float(data['growth'][rg.GROWTH_DEGREES.index(60)]), float(data['composition_err_n60']))
    for frm in (None, frames):
        A_sh = ga.gravityfield.gradient_design_matrix(xyz, c['min_degree'], c['max_degree'], GM, R, frames=frm, as_tensor=True)
        composed = _host(ga.engine.gemm(A_sh, ga.engine.to_device(F)))
        A = ga.gravityfield.rbf_gradient_design_matrix(basis, xyz, frm)
        err = np.abs(A - composed).max() / np.abs(A).max()
        print('d/o 60, frames {0}: {1:.2e} of max|A_rbf| (bound {2:.2e})'.format(frm is not None, err, bound))
        assert A.shape == composed.shape == (6 * c['points'], c['nodes']) and err <= bound
    restated = rg.restatement(ri.node_table(data['lon_n60'], data['lat_n60']), data['k_n60'], c['min_degree'], xyz, frames)
    assert np.array_equal(A, restated)


def test_forward_tensor_is_symmetric_and_matches_the_spherical_harmonic_route(golden):
    import torch
    data = golden('g30_rbf_gradients')
    c = ri.FORWARD
    basis = _basis(*ri.forward_nodes(), ri.degree_factors(c['min_degree'], c['max_degree']), c['min_degree'])
    basis.values = ri.forward_values()
    xyz = ri.forward_positions()
    mine = basis.gravitational_gradients(xyz)
    theirs = basis.to_potential_coefficients().gravitational_gradients(xyz)
    assert isinstance(mine, np.ndarray) and mine.shape == theirs.shape == (300, 3, 3)
    assert np.array_equal(mine, mine.transpose(0, 2, 1))
    on_device = basis.gravitational_gradients(ga.engine.to_device(xyz), as_tensor=True)
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and np.array_equal(_host(on_device), mine)
    err, bound = np.abs(mine - theirs).max() / np.abs(theirs).max(), 4 * float(data['forward_err'])
    print('gravitational_gradients: {0:.2e} of max|T| (bound {1:.2e})'.format(err, bound))
    assert err <= bound


# ---- seams and contracts ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seam_case():
    """band 2..8, tile + 5 nodes; 257 points: the 29 of the fixture (above a node, antipodal, 1 m beside, poles) and scattered ones"""
    tile = ga.engine.rbf_design_info()[0]
    lon, lat = ri.case_nodes('b2_8')
    extra = ri.scattered_nodes(tile + 5, 3031)
    lon, lat = np.concatenate((lon[:3], extra[0]))[:tile + 5], np.concatenate((lat[:3], extra[1]))[:tile + 5]
    xyz = np.vstack((rg.positions('b2_8'), ri.ai.scattered_positions(257 - 29, 3032)))
    return lon, lat, ri.degree_factors(2, 8), xyz, gdi.frames(257, 3033)


def _seam_basis(J):
    lon, lat, k = _seam_case()[:3]
    return _basis(lon[:J], lat[:J], k, 2)


def _rows(J, xyz, frames=None, components=None, weights=None):
    """At [J, K, M] on the host"""
    return _host(ga.engine.rbf_gradient_design(_seam_basis(J), xyz, frames, components, weights))


@pytest.mark.parametrize('framed', (False, True))
def test_entries_do_not_depend_on_the_batch(framed):
    """M in {1, 255, 256, 257} and J in {1, T - 1, T, T + 1, T + 5}: the entries of a point and a node are the same bits whatever the
    batch, the node count and the place of the point in the batch; two runs are bit-identical"""
    tile = ga.engine.rbf_design_info()[0]
    lon, lat, k, xyz, frames = _seam_case()

    def rows(J, index):
        return _rows(J, xyz[index], frames[index] if framed else None)
    everything = slice(0, 257)
    full = rows(tile + 5, everything)
    assert full.shape == (tile + 5, 6, 257) and np.all(np.isfinite(full)) and np.all(np.abs(full).max(axis=(1, 2)) > 0)
    for J in (1, tile - 1, tile, tile + 1, tile + 5):
        for M in (1, 255, 256, 257):
            got = rows(J, slice(0, M))
            assert np.array_equal(got, full[:J, :, :M]), (J, M)
            assert np.array_equal(got, rows(J, slice(0, M))), (J, M)                   # two runs
    for first, last in ((256, 257), (1, 257), (100, 200)):
        assert np.array_equal(rows(tile + 1, slice(first, last)), full[:tile + 1, :, first:last]), (first, last)
    order = np.random.default_rng(3034).permutation(257)
    assert np.array_equal(rows(tile + 5, order), full[:, :, order])


@pytest.mark.parametrize('framed', (False, True))
def test_leading_dimension_beyond_the_points(framed):
    """ldt = 300 for 257 points through the C entry point: the same bits, and the padding, filled with NaN before, is not touched"""
    import torch
    from grates_amd import _lib
    tile = ga.engine.rbf_design_info()[0]
    J, M, ldt, mask = tile + 1, 257, 300, 1 | 8 | 32 | 4
    lon, lat, k, xyz, frames = _seam_case()
    shape, nodes = ga.engine.rbf_node_table(_seam_basis(J))
    x, f = ga.engine.to_device(xyz), ga.engine.to_device(frames)
    out = torch.full((J, 4, ldt), float('nan'), dtype=torch.float64, device=x.device)
    _lib.call('shg_rbf_gradient_design', 8, 2, ctypes.c_void_p(shape.ctypes.data), ctypes.c_void_p(nodes.data_ptr()), J, ctypes.c_void_p(x.data_ptr()), M,
              ctypes.c_void_p(f.data_ptr()) if framed else None, mask, None, 0, GM, R, ctypes.c_void_p(out.data_ptr()), ldt,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    out = _host(out)
    assert np.array_equal(out[:, :, :M], _rows(J, xyz, frames if framed else None, ('xx', 'yy', 'zz', 'xz'))) and np.all(np.isnan(out[:, :, M:]))


@pytest.mark.parametrize('framed', (False, True))
def test_a_subset_of_components_is_the_matching_rows(framed):
    tile = ga.engine.rbf_design_info()[0]
    lon, lat, k, xyz, frames = _seam_case()
    F = frames if framed else None
    full = _rows(tile + 1, xyz, F)
    for components in SUBSETS + (('zz', 'xx'),):                                        # any order in, canonical order out
        picked = gdi.component_indices(components)
        assert np.array_equal(_rows(tile + 1, xyz, F, components), full[:, picked]), components


def test_identity_frames_are_the_frameless_call():
    """0 and 1 as factors round nothing: T f_b and f_a . (T f_b) are exact, up to the sign of a zero"""
    tile = ga.engine.rbf_design_info()[0]
    xyz = _seam_case()[3]
    eye = np.broadcast_to(np.eye(3), (257, 3, 3)).copy()
    for components in (None,) + SUBSETS:
        assert np.all(_rows(tile + 1, xyz, eye, components) == _rows(tile + 1, xyz, None, components)), components


@pytest.mark.parametrize('framed', (False, True))
def test_weights_scale_the_rows(framed):
    """a weighted matrix is bitwise the unweighted one times sqrt(w), per point and per selected component; a zero weight a zero row"""
    tile = ga.engine.rbf_design_info()[0]
    lon, lat, k, xyz, frames = _seam_case()
    F, J, M = frames if framed else None, tile + 1, 257
    rng = np.random.default_rng(3035)
    w = rng.uniform(0.1, 10.0, M)
    w[[0, 17, 255, 256]] = 0.0
    for components in (None, ('xx', 'yy', 'zz', 'xz')):
        plain = _rows(J, xyz, F, components)
        K = plain.shape[1]
        weighted = _rows(J, xyz, F, components, w)
        assert np.array_equal(weighted, plain * np.sqrt(w)[None, None, :]) and np.all(weighted[:, :, w == 0.0] == 0.0)
        assert np.all(np.abs(weighted[:, :, w > 0.0]).max(axis=(0, 1)) > 0)
        wk = rng.uniform(0.1, 10.0, (M, K))
        wk[5, 1] = wk[256] = 0.0
        weighted = _rows(J, xyz, F, components, wk)
        assert np.array_equal(weighted, plain * np.sqrt(wk).T[None, :, :]) and np.all(weighted[:, 1, 5] == 0.0) and np.all(weighted[:, :, 256] == 0.0)
        assert np.all(weighted[:, 0, 5] != 0.0)


def test_trace_is_zero_within_rounding():
    """xx + yy + zz, Earth-fixed and in seeded frames.  Every degree is trace-free on its own, so the trace is what rounding leaves.
    Earth-fixed, a diagonal entry is a sum of four terms (three additions) of products of rounded factors, each term within about
    3 ulp of its size, and the terms are no larger than about max|A| each after scaling (two more roundings): 3 entries x (4 terms x
    3 ulp + 3 additions + 2) = 51 roundings of size 2^-53 max|A| at most.  A frame adds 5 roundings per T f_b entry and 5 per f_a . u_b,
    on sums of three such entries: 3 x (3 x 17 + 10) = 183.  The sums S_rr, S_r + t S_t and S_tt themselves carry the rounding of the
    chain, 8 degrees x 3 roundings each, on three sums: 72 more.  Bounds: 128 and 256 ulp of max|A|."""
    tile = ga.engine.rbf_design_info()[0]
    lon, lat, k, xyz, frames = _seam_case()
    for F, bound in ((None, 128), (frames, 256)):
        rows = _rows(tile + 5, xyz, F, ('xx', 'yy', 'zz'))
        full = np.abs(_rows(tile + 5, xyz, F)).max()
        trace = np.abs((rows[:, 0] + rows[:, 1]) + rows[:, 2]).max()
        print('trace, frames {0}: {1:.1f} ulp of max|A| (bound {2})'.format(F is not None, trace / (full * U), bound))
        assert trace <= bound * U * full


# ---- normal equations --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loop(count):
    """(basis with the planted values, the field of its conversion, xyz, frames): the geometry of rbf_inputs.LOOP with `count` nodes"""
    c = ri.LOOP
    lon, lat = ri.fibonacci_nodes(count)
    basis = _basis(lon, lat, ri.degree_factors(c['min_degree'], c['max_degree']), c['min_degree'], R - c['depth'], 0.0)
    basis.values = ri.loop_values()[:count]
    return basis, basis.to_potential_coefficients(), ri.loop_positions()[0], rg.loop_frames()


def _observations(field, xyz, frames, components):
    return gdi.rotate_tensor(field.gravitational_gradients(xyz), frames, components)


def test_closed_loop_of_gradients(golden):
    """the observations come from the GPU's own spherical harmonic gravitational_gradients of to_potential_coefficients() of the
    planted values, rotated into the seeded frames; components (xx, yy, zz, xz)"""
    data = golden('g30_rbf_gradients')
    count = int(data['loop_nodes'])
    basis, field, xyz, frames = _loop(count)
    truth = ri.loop_values()[:count]
    obs = _observations(field, xyz, frames, rg.LOOP_COMPONENTS)
    ne = ga.lstsq.RadialBasisParameters(basis).from_gradients(xyz, obs, frames=frames, components=rg.LOOP_COMPONENTS)
    assert ne.observation_count == 4 * 600 and ne.right_hand_side.shape == (count, 1)
    x = _host(ne.solve())[:, 0]
    rel = np.linalg.norm(x - truth) / np.linalg.norm(truth)
    print('closed loop, gradients: relative error {0:.2e} (host {1:.2e}, cond(A) {2:.0f})'.format(rel, float(data['host_rel_err']), float(data['loop_cond'])))
    assert rel <= 10 * float(data['host_rel_err'])
    # full tensors [M, 3, 3] are accepted as observations: the same system
    full = np.einsum('iac,icd,ibd->iab', frames, field.gravitational_gradients(xyz), frames)
    again = ga.lstsq.RadialBasisParameters(basis).from_gradients(xyz, full, frames=frames, components=rg.LOOP_COMPONENTS)
    assert np.linalg.norm(_host(again.solve())[:, 0] - truth) <= 10 * float(data['host_rel_err']) * np.linalg.norm(truth)


def test_coloured_noise_normals_are_those_of_the_whitened_dense_matrix(golden):
    """ColouredNoise of order 2 over two arcs, three blocks of 256 points with their halos: the normals equal A~^T A~ with A~ the dense
    A_rbf whitened column by column (lstsq.decorrelate) and multiplied by engine.gemm, within 1e-13 of max|N|"""
    count = int(golden('g30_rbf_gradients')['loop_nodes'])
    basis, field, xyz, frames = _loop(count)
    J, M, K = count, 600, 4
    arcs = np.array([0, 280])
    obs = _observations(field, xyz, frames, rg.LOOP_COMPONENTS)
    obs = obs + np.random.default_rng(3041).standard_normal((M, K)) * 1e-3 * np.abs(obs).max()
    sequence = ga.lstsq.AutoregressiveModelSequence.from_covariance_function(wi.covariance_function('ar2'))
    model = ga.lstsq.ColouredNoise(sequence, arcs)
    ne = ga.lstsq.RadialBasisParameters(basis, model).from_gradients(xyz, obs, frames=frames, components=rg.LOOP_COMPONENTS, block_points=256)
    A = ga.gravityfield.rbf_gradient_design_matrix(basis, xyz, frames, rg.LOOP_COMPONENTS)          # [K M, J], row K i + c
    whitened = ga.lstsq.decorrelate(np.hstack((A.reshape(M, K * J), obs)), sequence, arcs)
    Aw, lw = whitened[:, :K * J].reshape(K * M, J), whitened[:, K * J:].reshape(K * M, 1)
    N_ref = _host(ga.engine.gemm(Aw, Aw, transa=True))
    n_ref = _host(ga.engine.gemm(Aw, lw, transa=True))
    got_N, got_n, got_l, n_obs = ne.to_array()
    err_N, err_n = np.abs(got_N - N_ref).max() / np.abs(N_ref).max(), np.abs(got_n - n_ref).max() / np.abs(n_ref).max()
    print('coloured noise: normals {0:.2e} of max|N|, right-hand side {1:.2e} of max|n|'.format(err_N, err_n))
    assert n_obs == K * M and got_N.shape == (J, J) and np.array_equal(got_N, got_N.T)
    assert err_N <= 1e-13 and err_n <= 1e-13 and abs(got_l - float(np.sum(lw * lw))) <= 1e-13 * got_l


def test_post_fit_residuals_are_l_minus_a_x(golden):
    count = int(golden('g30_rbf_gradients')['loop_nodes'])
    basis, field, xyz, frames = _loop(count)
    obs = _observations(field, xyz, frames, rg.LOOP_COMPONENTS)
    obs = obs + np.random.default_rng(3042).standard_normal(obs.shape) * 1e-3 * np.abs(obs).max()
    bound = ga.lstsq.RadialBasisParameters(basis)
    x = bound.from_gradients(xyz, obs, frames=frames, components=rg.LOOP_COMPONENTS).solve()
    fit = bound.of_gradients(x, xyz, obs, frames=frames, components=rg.LOOP_COMPONENTS, block_points=256)
    A = ga.gravityfield.rbf_gradient_design_matrix(basis, xyz, frames, rg.LOOP_COMPONENTS)
    expected = obs - (A @ _host(x)[:, 0]).reshape(600, 4)
    err = np.abs(fit.residuals - expected).max() / np.abs(obs).max()
    print('post-fit residuals: {0:.2e} of max|l|'.format(err))
    assert isinstance(fit.residuals, np.ndarray) and fit.residuals.shape == (600, 4) and err <= 1e-13
    assert np.array_equal(fit.whitened, fit.residuals) and np.array_equal(fit.arcs, [0])


def test_arc_biases_per_component_come_back(golden):
    """ArcParameters with a bias per component (arc_basis of degree 0, the shared form): planted biases of the size of the signal are
    estimated along; the node values and the biases (of max|l|) within 10 times the figures the host recorded for this system"""
    data = golden('g30_rbf_gradients')
    count = int(data['loop_nodes'])
    basis, field, xyz, frames = _loop(count)
    truth, arcs = ri.loop_values()[:count], ri.loop_arcs()
    clean = _observations(field, xyz, frames, rg.LOOP_COMPONENTS)
    biases = rg.loop_biases() * np.abs(clean).max()
    obs = clean + np.repeat(biases, ri.LOOP['arc_length'], axis=0)
    model = ga.lstsq.ArcParameters(ga.lstsq.arc_basis(arcs, 600, degree=0), arcs)
    ne = ga.lstsq.RadialBasisParameters(basis, model).from_gradients(xyz, obs, frames=frames, components=rg.LOOP_COMPONENTS)
    assert ne.observation_count == 4 * 600 - 4 * arcs.size and ne.arc_elimination.count == 4 * arcs.size
    x = ne.solve()
    rel = np.linalg.norm(_host(x)[:, 0] - truth) / np.linalg.norm(truth)
    estimated = ne.arc_elimination.parameters(x)[:, :, 0]
    worst = np.abs(estimated - biases).max() / np.abs(obs).max()
    print('arc biases: node values {0:.2e} (host {1:.2e}), biases {2:.2e} of max|l| (host {3:.2e}), cond(A) {4:.0f}'.format(
        rel, data['arc_rel_err'][0], worst, data['arc_rel_err'][1], float(data['arc_cond'])))
    assert estimated.shape == (arcs.size, 4) and rel <= 10 * float(data['arc_rel_err'][0]) and worst <= 10 * float(data['arc_rel_err'][1])


def test_gradients_and_accelerations_accumulate_on_one_basis(golden):
    """accumulate_normals of from_gradients and from_accelerations, the second scaled to the size of the first: the sum of two positive
    definite matrices is conditioned no worse than the worse of the two, so the bound is 10 times the larger of the two host figures"""
    data = golden('g30_rbf_gradients')
    host = max(float(data['host_rel_err']), float(golden('g29_radial_basis')['host_rel_err'][0]))
    count = int(data['loop_nodes'])
    basis, field, xyz, frames = _loop(count)
    truth = ri.loop_values()[:count]
    bound = ga.lstsq.RadialBasisParameters(basis)
    gradients = bound.from_gradients(xyz, _observations(field, xyz, frames, rg.LOOP_COMPONENTS), frames=frames, components=rg.LOOP_COMPONENTS)
    accelerations = bound.from_accelerations(xyz, field.gravitational_acceleration(xyz))
    scale = float(np.abs(_host(accelerations.matrix.device_block(0, 0))).max() / np.abs(_host(gradients.matrix.device_block(0, 0))).max())
    combined = ga.lstsq.accumulate_normals([gradients, accelerations], [1.0, scale])
    assert combined.observation_count == 4 * 600 + 3 * 600
    x = _host(combined.solve())[:, 0]
    rel = np.linalg.norm(x - truth) / np.linalg.norm(truth)
    print('gradients and accelerations: relative error {0:.2e} (host {1:.2e})'.format(rel, host))
    assert count == 48 and rel <= 10 * host                         # the host figure of the accelerations is that of 48 nodes
