"""
Golden vectors of the design matrices with respect to the node values of radial basis functions (g29_radial_basis.npz).  Run once
with the reference package `grates` importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_radial_basis.py

Like make_golden_potential.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and reference
outputs.  The reference cannot evaluate a RadialBasisFunctions at points; its conversion reaches them: a column of a design matrix is
the functional of RadialBasisFunctions.to_potential_coefficients() with one node value set to 1 -- gravitational_acceleration for the
acceleration and, through e . (g(b) - g(a)) in float64 NumPy, the line of sight; the sphere-by-sphere to_grid(kernel='potential') of
make_golden_potential.py for the potential and the potential difference.  K is zero below min_degree (to_potential_coefficients sums
all degrees).  Per case of rbf_inputs.CASES (band 0..8 and 2..8 with 24 scattered nodes on GRS80, band 2..2 with 3):

    lon_<case>, lat_<case>, k_<case>        the nodes [rad, geodetic] and the degree factors k_n
    xyz_a_<case>, xyz_b_<case>, e_<case>    rbf_inputs.pairs and .directions: 29 points (pairs); the single-point kinds use xyz_a
    A_acc_<case> [87, J], A_los_<case>, A_pot_<case>, A_dif_<case> [29, J]
    acc_scale_<case>, pot_scale_<case>      max|A_acc| and max|A_pot| over both satellites: what the rounding errors are proportional to
    restatement_err_<case> [4]              rbf_inputs.restatement (the kernel's operation order in float64 NumPy) against the four
                                            matrices, acc and los of acc_scale, pot and dif of pot_scale, over all points but
                                            rbf_inputs.NEAR_AXIS
    axis_err_<case> [4]                     the same at that point alone, 1 mm off the axis: there the reference's colatitude
                                            (t = cos(atan2(rho, z)) is 1, s = sqrt(1 - t^2) is 0) drops the tangential part, 1e-10 of
                                            the row; the closed sums keep it.  The figure is the reference's error, not the restatement's

the d/o-96 case (8 nodes, flat shape factors in 2..96, 300 points at heights of -25 .. 500 km, acceleration only): lon_n96, lat_n96,
k_n96, xyz_n96, A_acc_n96, acc_scale_n96, restatement_err_n96; and the scalars, all computed here on the CPU in NumPy:

    forward_err [2]     restatement @ values against the reference's gravitational_acceleration and potential of
                        to_potential_coefficients() for rbf_inputs.FORWARD (band 2..12, 40 nodes, 300 points), of max|g| and max|V|
    host_rel_err [3]    the closed loops of rbf_inputs.LOOP (band 2..8, 48 Fibonacci nodes 10 km below R, 600 points on eight shells at
                        250 .. 500 km, planted node values; observations from the reference's spherical harmonic route): accelerations;
                        accelerations and line of sight summed; potentials with a planted constant per arc estimated along.  Solved
                        on the host through the normals of the restatement, |x^ - x| / |x| (2-norms)
    loop_cond [3]       cond(A) of these geometries, for the third with the arc constants projected out
"""

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
import rbf_inputs as ri  # noqa: E402


def reference_basis(lon, lat, k, min_degree, a=ri.A, f=ri.F):
    grid = grates.grid.IrregularGrid(lon, lat, a=a, f=f)
    return grates.gravityfield.RadialBasisFunctions(grid, ri.shape_factors(k), min_degree, k.size - 1, ri.GM, ri.R)


def coefficients_of(basis, values):
    basis.values = np.ascontiguousarray(values, dtype=float)
    return basis.to_potential_coefficients()


def unit_values(J):
    return np.eye(J)


def reference_potential(xyz):
    """gf -> V [M] of the reference at xyz, the points grouped by the sphere they lie on (make_golden_potential.py)"""
    radius = np.sqrt((xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]) + xyz[:, 2] * xyz[:, 2])
    lon = np.arctan2(xyz[:, 1], xyz[:, 0])
    lat = np.arctan2(xyz[:, 2], np.sqrt(xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]))
    grids = [(index, grates.grid.IrregularGrid(lon[index], lat[index], a=r, f=0)) for r, index in ((r, np.flatnonzero(radius == r)) for r in np.unique(radius))]

    def potential(gf):
        V = np.empty(xyz.shape[0])
        for index, grid in grids:
            V[index] = gf.to_grid(grid, kernel='potential').values
        return V
    return potential


def reference_matrices(basis, a, b, e):
    """(A_acc(a), A_acc(b), A_los, A_pot(a), A_pot(b), A_dif) column by column from unit node values"""
    J, M = basis.point_distribution.size, a.shape[0]
    pot_a, pot_b = reference_potential(a), reference_potential(b)
    acc_a, acc_b, los, Va, Vb = [], [], [], [], []
    for values in unit_values(J):
        gf = coefficients_of(basis, values)
        g = gf.gravitational_acceleration(np.vstack((a, b)))
        acc_a.append(g[:M].ravel())
        acc_b.append(g[M:].ravel())
        los.append(ri.project(e, g[M:], g[:M]))
        Va.append(pot_a(gf))
        Vb.append(pot_b(gf))
    acc_a, acc_b, los, Va, Vb = (np.stack(columns, axis=1) for columns in (acc_a, acc_b, los, Va, Vb))
    same = np.all(a == b, axis=1)
    Vb[same] = Va[same]                               # one position, two synthesis calls of the reference: its sums differ in the last bits
    return acc_a, acc_b, los, Va, Vb, Vb - Va


def solve(A, obs):
    return np.linalg.solve(A.T @ A, A.T @ obs)


def main():
    out = {}
    for tag, (min_degree, max_degree, _, _) in ri.CASES.items():
        lon, lat = ri.case_nodes(tag)
        k = ri.degree_factors(min_degree, max_degree)
        a, b = ri.pairs(tag)
        e = ri.directions(tag)
        acc_a, acc_b, los, Va, Vb, dif = reference_matrices(reference_basis(lon, lat, k, min_degree), a, b, e)
        acc_scale, pot_scale = max(np.abs(acc_a).max(), np.abs(acc_b).max()), max(np.abs(Va).max(), np.abs(Vb).max())
        assert np.all(np.isfinite(acc_a)) and np.all(dif[ri.separations() == 0.0] == 0.0) and np.all(los[ri.separations() == 0.0] == 0.0)
        nodes = ri.node_table(lon, lat)
        rows = np.stack([ri.point_errors(ri.restatement(kind, nodes, k, min_degree, a, b, e), ref) / scale
                         for kind, ref, scale in (('acc', acc_a, acc_scale), ('los', los, acc_scale), ('pot', Va, pot_scale), ('dif', dif, pot_scale))])
        err, axis_err = np.delete(rows, ri.NEAR_AXIS, axis=1).max(axis=1), rows[:, ri.NEAR_AXIS]
        print('{0}: max|A_acc| {1:.3e}, max|A_pot| {2:.3e}; restatement acc {3:.2e}, los {4:.2e} of max|A_acc|, pot {5:.2e}, dif {6:.2e} of max|A_pot|; '
              'at the point 1 mm off the axis {7}'.format(tag, acc_scale, pot_scale, *err, axis_err))
        out.update({'lon_' + tag: lon, 'lat_' + tag: lat, 'k_' + tag: k, 'xyz_a_' + tag: a, 'xyz_b_' + tag: b, 'e_' + tag: e, 'A_acc_' + tag: acc_a,
                    'A_los_' + tag: los, 'A_pot_' + tag: Va, 'A_dif_' + tag: dif, 'acc_scale_' + tag: acc_scale, 'pot_scale_' + tag: pot_scale,
                    'restatement_err_' + tag: err, 'axis_err_' + tag: axis_err})

    c = ri.N96
    lon, lat = ri.n96_nodes()
    k = ri.degree_factors(c['min_degree'], c['max_degree'], flat=True)
    xyz = ri.n96_positions()
    basis = reference_basis(lon, lat, k, c['min_degree'])
    A96 = np.stack([coefficients_of(basis, values).gravitational_acceleration(xyz).ravel() for values in unit_values(c['nodes'])], axis=1)
    scale96 = np.abs(A96).max()
    err96 = np.abs(ri.restatement('acc', ri.node_table(lon, lat), k, c['min_degree'], xyz) - A96).max() / scale96
    print('n96: max|A_acc| {0:.3e}; restatement {1:.2e} of it'.format(scale96, err96))
    out.update(lon_n96=lon, lat_n96=lat, k_n96=k, xyz_n96=xyz, A_acc_n96=A96, acc_scale_n96=scale96, restatement_err_n96=err96)

    c = ri.FORWARD
    lon, lat = ri.forward_nodes()
    k = ri.degree_factors(c['min_degree'], c['max_degree'])
    xyz, values = ri.forward_positions(), ri.forward_values()
    gf = coefficients_of(reference_basis(lon, lat, k, c['min_degree']), values)
    g, V = gf.gravitational_acceleration(xyz), reference_potential(xyz)(gf)
    nodes = ri.node_table(lon, lat)
    forward_err = np.array([np.abs((ri.restatement('acc', nodes, k, c['min_degree'], xyz) @ values).reshape(-1, 3) - g).max() / np.abs(g).max(),
                            np.abs(ri.restatement('pot', nodes, k, c['min_degree'], xyz) @ values - V).max() / np.abs(V).max()])
    print('forward at band {0}..{1}: acceleration {2:.2e} of max|g|, potential {3:.2e} of max|V|'.format(c['min_degree'], c['max_degree'], *forward_err))

    c = ri.LOOP
    lon, lat, a_nodes, f_nodes = ri.loop_nodes()
    k = ri.degree_factors(c['min_degree'], c['max_degree'])
    x = ri.loop_values()
    gf = coefficients_of(reference_basis(lon, lat, k, c['min_degree'], a_nodes, f_nodes), x)
    nodes = ri.node_table(lon, lat, a_nodes, f_nodes)
    a, b = ri.loop_pairs()
    g = gf.gravitational_acceleration(np.vstack((a, b)))
    M = a.shape[0]
    d = b - a
    e = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, np.newaxis]
    A_acc = ri.restatement('acc', nodes, k, c['min_degree'], a)
    A_los = ri.restatement('los', nodes, k, c['min_degree'], a, b, e)
    A_pot = ri.restatement('pot', nodes, k, c['min_degree'], a)
    B = ri.arc_indicator()
    both = np.vstack((A_acc, A_los))
    full = np.hstack((A_pot, B))
    projected = A_pot - B @ np.linalg.lstsq(B, A_pot, rcond=None)[0]
    estimates = (solve(A_acc, g[:M].ravel()), solve(both, np.concatenate((g[:M].ravel(), ri.project(e, g[M:], g[:M])))),
                 solve(full, reference_potential(a)(gf) + B @ ri.loop_constants())[:x.size])
    host_rel_err = np.array([np.linalg.norm(estimate - x) / np.linalg.norm(x) for estimate in estimates])
    loop_cond = np.array([np.linalg.cond(A_acc), np.linalg.cond(both), np.linalg.cond(projected)])
    print('closed loops on the host (acc, acc + los, pot with arc constants): relative errors {0}, cond(A) {1}'.format(host_rel_err, loop_cond))
    assert np.all(loop_cond <= 1e4) and np.all(host_rel_err <= 1e-8)

    out.update(forward_err=forward_err, host_rel_err=host_rel_err, loop_cond=loop_cond)
    path = os.path.join(HERE, 'g29_radial_basis.npz')
    np.savez_compressed(path, **out)
    print('g29_radial_basis {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
