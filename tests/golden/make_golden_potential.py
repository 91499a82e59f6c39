"""
Golden vectors of the gravitational potential at points, of its design matrix and of the design matrix of the potential difference of
satellite pairs (g28_potential.npz).  Run once with the reference package `grates` importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_potential.py

Like make_golden_line_of_sight.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and
reference outputs.  The reference has no point functional of the potential; its grid synthesis reaches it:
PotentialCoefficients.to_grid(IrregularGrid(lon, lat, a=r, f=0), kernel='potential').values is V on the sphere of radius r, so the
points are taken sphere by sphere (a few shells for the scattered points, a sphere of its own for every special position), with
lon = atan2(y, x) and lat = atan2(z, sqrt(x^2 + y^2)).  The design matrices come column by column from unit coefficient fields, the
pair matrices as the difference of the two satellites' columns:

    xyz, xyz_a, xyz_b             potential_inputs.positions() and .pairs() (xyz_a is xyz)
    A_pot8, A_pot2                d/o 8 and d/o 2, min_degree 0, at xyz
    A_pot8_min2, A_pot2_min2      the same from unit fields of degrees >= 2 only (the column slices of the former)
    A_dif8 ... A_dif2_min2        the four of V(b) - V(a): separations of 220 km, 1 km, 1 m and 0
    pot_scale8, pot_scale2        max|A_pot| over both satellites: what the rounding errors of a row are proportional to
    xyz60, V60, V60_scale         V of a d/o-60 anomaly field at potential_inputs.v60_positions(), and max|V60|

and the scalars, all computed here on the CPU in NumPy:

    restatement_err   potential_inputs.restatement / difference_restatement (the kernel's formulas in float64 NumPy) against the eight
                      matrices, of pot_scale; forward_err: potential_inputs.forward against V60, of V60_scale
    ax_err            A @ x against the reference's V at potential_inputs.ax_positions() (A from 3721 unit fields), of max|V|
    host_rel_err      [3]: the closed loops of potential_inputs.LOOP (V, V(b) - V(a), V with a planted constant per arc, estimated
                      along with the field) solved on the host through the normals, |x^ - x| / |x| (2-norms); loop_cond [3] is cond(A)
                      of these geometries, for the third with the arc constants projected out
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
import design_inputs as di  # noqa: E402
import potential_inputs as pi  # noqa: E402


def reference_potential(xyz, radius):
    """anm -> V [M] of the reference at xyz, the points grouped by the sphere (`radius`) they lie on"""
    lon = np.arctan2(xyz[:, 1], xyz[:, 0])
    lat = np.arctan2(xyz[:, 2], np.sqrt(xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]))
    groups = [(r, np.flatnonzero(radius == r)) for r in np.unique(radius)]
    grids = [(index, grates.grid.IrregularGrid(lon[index], lat[index], a=r, f=0)) for r, index in groups]

    def potential(anm):
        gf = grates.gravityfield.PotentialCoefficients(pi.GM, pi.R)
        gf.anm = anm
        V = np.empty(xyz.shape[0])
        for index, grid in grids:
            V[index] = gf.to_grid(grid, kernel='potential').values
        return V
    return potential


def unit_field_matrix(potential, min_degree, max_degree):
    """A [M, P] column by column from the reference's V of unit coefficient fields"""
    return np.stack([potential(di.unit_field(n, m, sine, max_degree)) for n, m, sine in di.degreewise(min_degree, max_degree)], axis=1)


def solve(A, obs):
    return np.linalg.solve(A.T @ A, A.T @ obs)


def main():
    xyz, radius = pi.positions()
    a, b = pi.pairs()
    assert np.array_equal(a, xyz)
    at_a, at_b = reference_potential(a, radius), reference_potential(b, pi.radius_of(b))
    out = {'xyz': xyz, 'xyz_a': a, 'xyz_b': b}
    restatement_err = 0.0
    far = pi.separations() > 100e3
    for N in pi.DEGREES:
        A_a, A_b = unit_field_matrix(at_a, 0, N), unit_field_matrix(at_b, 0, N)
        A_a2, A_b2 = unit_field_matrix(at_a, 2, N), unit_field_matrix(at_b, 2, N)
        assert np.array_equal(A_a2, A_a[:, 4:]) and np.array_equal(A_b2, A_b[:, 4:]), N
        scale = max(np.abs(A_a).max(), np.abs(A_b).max())
        D, D2 = A_b - A_a, A_b2 - A_a2
        assert np.all(np.isfinite(A_a)) and np.all(np.isfinite(D)) and np.all(D[pi.separations() == 0.0] == 0.0)
        out.update({'A_pot{0}'.format(N): A_a, 'A_pot{0}_min2'.format(N): A_a2, 'A_dif{0}'.format(N): D, 'A_dif{0}_min2'.format(N): D2,
                    'pot_scale{0}'.format(N): scale})
        err_pot = np.abs(pi.restatement(a, 0, N) - A_a).max(axis=1)
        err_dif = np.abs(pi.difference_restatement(a, b, 0, N) - D).max(axis=1)
        restatement_err = max(restatement_err, err_pot.max() / scale, err_dif.max() / scale)
        print('d/o {0}: max|A_pot| {1:.3e}, max|A_dif| at 220 km {2:.3e}; restatement {3:.2e} (point {4}) and {5:.2e} (pair {6}) of max|A_pot|, '
              '{7:.2e} of max|A_dif| at 220 km'.format(N, scale, np.abs(D[far]).max(), err_pot.max() / scale, err_pot.argmax(), err_dif.max() / scale,
                                                       err_dif.argmax(), err_dif[far].max() / np.abs(D[far]).max()))

    N = pi.V60[0]
    xyz60, radius60 = pi.v60_positions()
    anm = pi.v60_field()
    V60 = reference_potential(xyz60, radius60)(anm)
    V60_scale = np.abs(V60).max()
    forward_err = np.abs(pi.forward(xyz60, anm) - V60).max() / V60_scale
    print('forward restatement at d/o {0}, {1} points: {2:.2e} of max|V| = {3:.3e}'.format(N, xyz60.shape[0], forward_err, V60_scale))
    out.update(xyz60=xyz60, V60=V60, V60_scale=V60_scale)

    xyz_ax, radius_ax = pi.ax_positions()
    at_ax = reference_potential(xyz_ax, radius_ax)
    V_ax = at_ax(anm)
    ax_err = np.abs(unit_field_matrix(at_ax, 0, N) @ di.ravel(anm, 0, N) - V_ax).max() / np.abs(V_ax).max()
    print('A @ x at d/o {0}, {1} points: {2:.2e} of max|V|'.format(N, xyz_ax.shape[0], ax_err))

    loop = pi.LOOP
    N, min_degree = loop['N'], loop['min_degree']
    anm = pi.loop_field()
    x = di.ravel(anm, min_degree, N)
    la, lb, radius_a, radius_b = pi.loop_pairs()
    at_a, at_b = reference_potential(la, radius_a), reference_potential(lb, radius_b)
    A_a, A_b = unit_field_matrix(at_a, min_degree, N), unit_field_matrix(at_b, min_degree, N)
    V_a, V_b = at_a(anm), at_b(anm)
    B = pi.arc_indicator()
    full = np.hstack((A_a, B))
    projected = A_a - B @ np.linalg.lstsq(B, A_a, rcond=None)[0]
    estimates = (solve(A_a, V_a), solve(A_b - A_a, V_b - V_a), solve(full, V_a + B @ pi.loop_constants())[:x.size])
    host_rel_err = np.array([np.linalg.norm(e - x) / np.linalg.norm(x) for e in estimates])
    loop_cond = np.array([np.linalg.cond(A_a), np.linalg.cond(A_b - A_a), np.linalg.cond(projected)])
    print('closed loops on the host (V, V(b) - V(a), V with arc constants): relative errors {0}, cond(A) {1}'.format(host_rel_err, loop_cond))
    assert np.all(loop_cond <= 1e4) and np.all(host_rel_err <= 1e-8)

    out.update(restatement_err=restatement_err, forward_err=forward_err, ax_err=ax_err, host_rel_err=host_rel_err, loop_cond=loop_cond)
    path = os.path.join(HERE, 'g28_potential.npz')
    np.savez_compressed(path, **out)
    print('g28_potential {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
