"""
Golden vectors of the gradient-tensor design matrix with respect to the node values of radial basis functions
(g30_rbf_gradients.npz).  Run once with the reference package `grates` importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rbf_gradients.py [--processes P]

An independent truth: a column of A is the gradient tensor of the reference's RadialBasisFunctions.to_potential_coefficients() with
one node value set to 1 (reached as make_golden_radial_basis.py reaches the reference), evaluated by the mp oracle of
make_golden_gradients.py -- the potential with mpmath at 50 digits, central differences at mp precision -- which is imported as it
is and handed the coefficient tables, as make_golden_gradient_design.py hands it unit fields.  The oracle loses nothing near the axis
or near a node, so no point has a bound of its own.  Per case of rbf_inputs.CASES (band 0..8 and 2..8 with 24 nodes, 2..2 with 3):

    lon_<case>, lat_<case>, k_<case>     the nodes [rad, geodetic] and the degree factors k_n
    xyz_<case>, frames_<case>            rbf_inputs.pairs(case)[0], 29 points (with the points above a node, antipodal to it and 1 m
                                         beside it), and seeded proper rotations for them (the first is the identity)
    A_<case> [6 * 29, J]                 Earth-fixed, row 6 i + j for component j of xx, xy, xz, yy, yz, zz at point i
    scale_<case>                         max|A|
    restatement_err_<case>               rbf_gradient_inputs.restatement (the kernel's operation order in float64 NumPy) against A,
                                         of max|A|

and, all computed here on the CPU in NumPy:

    growth [4]            float64 against long double of the restatement at N = 8, 60, 96, 180 (rbf_gradient_inputs.growth), of max|A|
    lon_n60, lat_n60, k_n60, xyz_n60, frames_n60
                          the high-degree case rbf_gradient_inputs.N60 (band 2..60, flat shape factors, 8 nodes, 64 points)
    composition_err_n60   gradient_design_inputs.restatement (the spherical harmonic design matrix) times the reference's
                          to_potential_coefficients of the unit node values, against the restatement, of max|A|: the composition's
                          own error, Earth-fixed
    forward_err           restatement @ values against the mp oracle's tensor of to_potential_coefficients() for rbf_inputs.FORWARD
                          (band 2..12, 40 nodes) at its first FORWARD_POINTS points, of max|T|
    k_n96, A_n96 [6 * 16, 8], scale_n96, restatement_err_n96
                          the mp column at d/o 96 (rbf_gradient_inputs.N96: band 2..96, flat factors, N60's nodes and first 16 points)
    loop_cond, host_rel_err, loop_nodes
                          the closed loop: the geometry of rbf_inputs.LOOP (600 points) in seeded frames with the components
                          (xx, yy, zz, xz), planted node values, observations from the restatement of the spherical harmonic
                          route; cond(A) and |x^ - x| / |x| of the solution through host normals.  The node count is halved until
                          cond(A) <= 1e3 and the count that was used is stored
    arc_cond, arc_rel_err [2]
                          the same loop with a planted bias per arc and component (rbf_gradient_inputs.loop_biases, of the size of
                          the observations) estimated along: cond(A) with the biases projected out, |x^ - x| / |x| of the node values
                          and max|b^ - b| / max|l| of the biases
"""

import argparse
import multiprocessing
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

for _name, _attr in (('netCDF4', 'Dataset'), ('h5py', 'File')):
    if _name not in sys.modules:
        _mod = types.ModuleType(_name)
        setattr(_mod, _attr, None)
        sys.modules[_name] = _mod
sys.dont_write_bytecode = True
import grates  # noqa: E402

sys.path.insert(0, HERE)
import gradient_design_inputs as gdi  # noqa: E402
import make_golden_gradients as oracle  # noqa: E402
import rbf_gradient_inputs as rg  # noqa: E402
import rbf_inputs as ri  # noqa: E402
from mpmath import mp, mpf  # noqa: E402

FORWARD_POINTS = 40


def reference_basis(lon, lat, k, min_degree, a=ri.A, f=ri.F):
    grid = grates.grid.IrregularGrid(lon, lat, a=a, f=f)
    return grates.gravityfield.RadialBasisFunctions(grid, ri.shape_factors(k), min_degree, k.size - 1, ri.GM, ri.R)


def coefficients_of(basis, values):
    basis.values = np.ascontiguousarray(values, dtype=float)
    return np.array(basis.to_potential_coefficients().anm, dtype=float)


def _tables(anm):
    """what make_golden_gradients._setup builds for a case, for the coefficients anm [N + 1, N + 1]"""
    mp.dps = oracle.DPS
    N = anm.shape[0] - 1
    C = [[mpf(float(anm[n, m])) for n in range(N + 1)] for m in range(N + 1)]                    # C[m][n]
    S = [[mpf(float(anm[m - 1, n])) if m >= 1 else mpf(0) for n in range(N + 1)] for m in range(N + 1)]
    a = [[mpf(0)] * (N + 1) for _ in range(N + 1)]
    b = [[mpf(0)] * (N + 1) for _ in range(N + 1)]
    for m in range(N + 1):
        for n in range(m + 2, N + 1):
            a[m][n] = mp.sqrt(mpf((2 * n - 1) * (2 * n + 1)) / ((n - m) * (n + m)))
            b[m][n] = mp.sqrt(mpf((2 * n + 1) * (n - m - 1) * (n + m - 1)) / ((2 * n - 3) * (n - m) * (n + m)))
    return N, C, S, a, b


def column(args):
    """[6 M]: the oracle tensor of the field anm at every position"""
    key, anm, xyz = args
    assert oracle.gi.GM == ri.GM and oracle.gi.R == ri.R
    tag = ('rbf',) + key
    oracle._tables[tag] = _tables(anm)
    T = np.stack([oracle.tensor((tag, x)) for x in xyz])
    del oracle._tables[tag]
    return np.stack([T[:, c, d] for c, d in gdi.PAIRS], axis=1).ravel()


def solve(A, obs):
    return np.linalg.solve(A.T @ A, A.T @ obs)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--processes', type=int, default=min(os.cpu_count() or 1, 8))
    args = parser.parse_args()
    out = {}
    with multiprocessing.Pool(args.processes) as pool:
        for tag, (min_degree, max_degree, count, _) in ri.CASES.items():
            lon, lat = ri.case_nodes(tag)
            k = ri.degree_factors(min_degree, max_degree)
            xyz = rg.positions(tag)
            basis = reference_basis(lon, lat, k, min_degree)
            tasks = [((tag, j), coefficients_of(basis, values), xyz) for j, values in enumerate(np.eye(count))]
            A = np.stack(pool.map(column, tasks, chunksize=1), axis=1)
            assert A.shape == (6 * xyz.shape[0], count) and np.all(np.isfinite(A))
            scale = np.abs(A).max()
            err = np.abs(rg.restatement(ri.node_table(lon, lat), k, min_degree, xyz) - A).reshape(xyz.shape[0], -1).max(axis=1) / scale
            print('{0}: max|A| {1:.3e}, restatement {2:.2e} of it (worst point {3})'.format(tag, scale, err.max(), int(np.argmax(err))))
            F = rg.frames(xyz.shape[0])
            assert np.abs(np.einsum('iac,ibc->iab', F, F) - np.eye(3)).max() <= 1e-14 and np.array_equal(F[0], np.eye(3))
            out.update({'lon_' + tag: lon, 'lat_' + tag: lat, 'k_' + tag: k, 'xyz_' + tag: xyz, 'frames_' + tag: F, 'A_' + tag: A,
                        'scale_' + tag: scale, 'restatement_err_' + tag: err.max()})

        c = ri.FORWARD
        lon, lat = ri.forward_nodes()
        k = ri.degree_factors(c['min_degree'], c['max_degree'])
        xyz, values = ri.forward_positions()[:FORWARD_POINTS], ri.forward_values()
        anm = coefficients_of(reference_basis(lon, lat, k, c['min_degree']), values)
        T = np.concatenate(pool.map(column, [(('forward', i), anm, xyz[i:i + 1]) for i in range(xyz.shape[0])], chunksize=1))
        forward = rg.restatement(ri.node_table(lon, lat), k, c['min_degree'], xyz) @ values
        forward_err = np.abs(forward - T).max() / np.abs(T).max()
        print('forward at band {0}..{1}, {2} points: {3:.2e} of max|T|'.format(c['min_degree'], c['max_degree'], xyz.shape[0], forward_err))
        out.update(forward_err=forward_err, forward_points=FORWARD_POINTS)

        c = rg.N96
        lon, lat = rg.n60_nodes()
        k = ri.degree_factors(c['min_degree'], c['max_degree'], flat=True)
        xyz = rg.n60_positions()[:c['points']]
        basis = reference_basis(lon, lat, k, c['min_degree'])
        tasks = [(('n96', j, i), coefficients_of(basis, values), xyz[i:i + 1]) for j, values in enumerate(np.eye(lon.size)) for i in range(c['points'])]
        A = np.stack(pool.map(column, tasks, chunksize=1)).reshape(lon.size, c['points'] * 6).T
        err = np.abs(rg.restatement(ri.node_table(lon, lat), k, c['min_degree'], xyz) - A).max() / np.abs(A).max()
        print('n96: max|A| {0:.3e}, restatement {1:.2e} of it'.format(np.abs(A).max(), err))
        out.update(k_n96=k, A_n96=A, scale_n96=np.abs(A).max(), restatement_err_n96=err)

    growth = np.array([rg.growth(N) for N in rg.GROWTH_DEGREES])
    print('float64 against long double at N = {0}: {1}'.format(rg.GROWTH_DEGREES, growth))
    out['growth'] = growth

    c = rg.N60
    lon, lat = rg.n60_nodes()
    k = ri.degree_factors(c['min_degree'], c['max_degree'], flat=True)
    xyz = rg.n60_positions()
    basis = reference_basis(lon, lat, k, c['min_degree'])
    Fm = np.stack([gdi.ravel(coefficients_of(basis, values), c['min_degree'], c['max_degree']) for values in np.eye(c['nodes'])], axis=1)
    A = rg.restatement(ri.node_table(lon, lat), k, c['min_degree'], xyz)
    composed = gdi.restatement(xyz, c['min_degree'], c['max_degree']) @ Fm
    composition_err = np.abs(composed - A).max() / np.abs(A).max()
    print('n60: max|A| {0:.3e}; the composition against the restatement {1:.2e} of it'.format(np.abs(A).max(), composition_err))
    out.update(lon_n60=lon, lat_n60=lat, k_n60=k, xyz_n60=xyz, frames_n60=rg.n60_frames(), composition_err_n60=composition_err)

    c = ri.LOOP
    count = c['nodes']
    xyz, _ = ri.loop_positions()
    F = rg.loop_frames()
    k = ri.degree_factors(c['min_degree'], c['max_degree'])
    while True:
        lon, lat = ri.fibonacci_nodes(count)
        a_nodes, f_nodes = ri.R - c['depth'], 0.0
        A = rg.restatement(ri.node_table(lon, lat, a_nodes, f_nodes), k, c['min_degree'], xyz, F, rg.LOOP_COMPONENTS)
        loop_cond = np.linalg.cond(A)
        print('closed loop with {0} nodes: cond(A) {1:.1f}'.format(count, loop_cond))
        if loop_cond <= 1e3:
            break
        count //= 2
    x = ri.loop_values()[:count]
    anm = coefficients_of(reference_basis(lon, lat, k, c['min_degree'], a_nodes, f_nodes), x)
    obs = gdi.restatement(xyz, c['min_degree'], c['max_degree'], F, rg.LOOP_COMPONENTS) @ gdi.ravel(anm, c['min_degree'], c['max_degree'])
    host_rel_err = np.linalg.norm(solve(A, obs) - x) / np.linalg.norm(x)
    print('closed loop on the host: relative error {0:.2e}'.format(host_rel_err))
    assert host_rel_err <= 1e-8
    out.update(loop_cond=loop_cond, host_rel_err=host_rel_err, loop_nodes=count)

    B = rg.bias_indicator()
    biases = rg.loop_biases() * np.abs(obs).max()
    biased = obs + B @ biases.ravel()
    estimate = solve(np.hstack((A, B * np.abs(A).max())), biased)                       # the columns of B scaled to the size of A's
    arc_cond = np.linalg.cond(A - B @ np.linalg.lstsq(B, A, rcond=None)[0])
    arc_rel_err = np.array([np.linalg.norm(estimate[:count] - x) / np.linalg.norm(x),
                            np.abs(estimate[count:] * np.abs(A).max() - biases.ravel()).max() / np.abs(biased).max()])
    print('with a bias per arc and component: node values {0:.2e}, biases {1:.2e} of max|l|, cond(A) {2:.1f}'.format(*arc_rel_err, arc_cond))
    assert arc_cond <= 1e3 and np.all(arc_rel_err <= 1e-8)
    out.update(arc_cond=arc_cond, arc_rel_err=arc_rel_err)

    path = os.path.join(HERE, 'g30_rbf_gradients.npz')
    np.savez_compressed(path, **out)
    print('g30_rbf_gradients {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
