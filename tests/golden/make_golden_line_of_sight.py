"""
Golden vectors of the design matrix of the line-of-sight gravity difference of satellite pairs (g26_line_of_sight.npz).  Run once
with the reference package `grates` importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_line_of_sight.py

Like make_golden_acceleration_design.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and
reference outputs.  The reference has neither the observation nor its design matrix; both come from its
PotentialCoefficients.gravitational_acceleration, the design matrix column by column from unit coefficient fields at the two
satellites, then e . (g(b) - g(a)) in float64 NumPy (los_inputs.project):

    xyz_a, xyz_b, directions      los_inputs.pairs() and the seeded explicit lines of sight
    A_los8, A_los2                d/o 8 and d/o 2, min_degree 0, e = (b - a) / |b - a|
    A_los8_min2, A_los2_min2      the same from unit fields of degrees >= 2 only (the column slices of the former)
    A_los8_dir ... A_los2_dir_min2  the four with e = directions
    acc_scale8, acc_scale2        max|A_acc| over both satellites: what the rounding errors of a row are proportional to
    l60, g60_scale                e . (g(b) - g(a)) of a d/o-60 anomaly field at los_inputs.l60_pairs(), and max|g| over both satellites

and the scalars, all computed here on the CPU in NumPy:

    restatement_err   los_inputs.restatement (the kernels' formulas in float64 NumPy) against the eight matrices, of acc_scale;
                      restatement_err_by_separation: the same for the pairs of 220 km, 1 km and 1 m
    ax_err            A @ x against l60 (A from 3721 calls of the reference at the 826 stacked points), of g60_scale
    host_rel_err      the closed loop of los_inputs.LOOP solved on the host through the normals, |x^ - x| / |x| (2-norms);
                      loop_cond is cond(A) of that geometry
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
import los_inputs as li  # noqa: E402


def reference_acceleration(xyz):
    def acceleration(anm):
        gf = grates.gravityfield.PotentialCoefficients(li.GM, li.R)
        gf.anm = anm
        return gf.gravitational_acceleration(xyz)
    return acceleration


def endpoint_matrices(a, b, min_degree, max_degree):
    """the acceleration design matrices [3 M, P] of the two satellites, from one reference call per unit field on the stacked points"""
    M = a.shape[0]
    stacked = np.vstack((a, b))
    A = di.unit_field_matrix(reference_acceleration(stacked), stacked, min_degree, max_degree)
    return A[:3 * M], A[3 * M:]


def reference_difference(a, b, e, anm):
    g = reference_acceleration(np.vstack((a, b)))(anm)
    M = a.shape[0]
    return li.project(e, g[M:], g[:M]), np.abs(g).max()


def main():
    a, b = li.pairs()
    explicit = li.directions()
    sep = li.separations()
    out = {'xyz_a': a, 'xyz_b': b, 'directions': explicit}
    restatement_err, by_separation = 0.0, np.zeros(3)
    groups = (sep > 100e3, (sep > 10.0) & (sep < 100e3), sep < 10.0)
    for N in li.DEGREES:
        A_a, A_b = endpoint_matrices(a, b, 0, N)
        A_a2, A_b2 = endpoint_matrices(a, b, 2, N)
        scale = max(np.abs(A_a).max(), np.abs(A_b).max())
        out['acc_scale{0}'.format(N)] = scale
        for tag, e in (('', li.line_of_sight(a, b)), ('_dir', explicit)):
            A = li.from_acceleration_matrices(A_a, A_b, e)
            A_min2 = li.from_acceleration_matrices(A_a2, A_b2, e)
            assert np.all(np.isfinite(A)) and np.array_equal(A_min2, A[:, 4:]), N
            out['A_los{0}{1}'.format(N, tag)], out['A_los{0}{1}_min2'.format(N, tag)] = A, A_min2
            err = np.abs(li.restatement(a, b, 0, N, None if not tag else e) - A).max(axis=1)
            restatement_err = max(restatement_err, err.max() / scale)
            by_separation = np.maximum(by_separation, [err[g].max() / scale for g in groups])
            big = np.abs(A[groups[0]]).max()
            print('d/o {0}{1}: A {2}, max|A_acc| {3:.3e}, max|A_los| at 220 km {4:.3e}, restatement {5:.2e} of max|A_acc| ({6} at 220 km, 1 km, 1 m; '
                  '{7} of max|A_los| at 220 km)'.format(N, tag, A.shape, scale, big, err.max() / scale,
                                                       ', '.join('{0:.1e}'.format(err[g].max() / scale) for g in groups),
                                                       ', '.join('{0:.1e}'.format(err[g].max() / big) for g in groups)))

    tag, N, _, _ = li.L60
    a, b = li.l60_pairs()
    anm = li.l60_field()
    e = li.line_of_sight(a, b)
    l60, g60_scale = reference_difference(a, b, e, anm)
    A_a, A_b = endpoint_matrices(a, b, 0, N)
    ax_err = np.abs(li.from_acceleration_matrices(A_a, A_b, e) @ di.ravel(anm, 0, N) - l60).max() / g60_scale
    print('A @ x at d/o {0}, {1} pairs: {2:.2e} of max|g|'.format(N, a.shape[0], ax_err))
    out.update(l60=l60, g60_scale=g60_scale)

    loop = li.LOOP
    (a, b), anm = li.loop_pairs(), li.loop_field()
    e = li.line_of_sight(a, b)
    A_a, A_b = endpoint_matrices(a, b, loop['min_degree'], loop['N'])
    A = li.from_acceleration_matrices(A_a, A_b, e)
    obs, _ = reference_difference(a, b, e, anm)
    x = di.ravel(anm, loop['min_degree'], loop['N'])
    solution = np.linalg.solve(A.T @ A, A.T @ obs)
    host_rel_err = np.linalg.norm(solution - x) / np.linalg.norm(x)
    loop_cond = np.linalg.cond(A)
    print('closed loop on the host: relative error {0:.2e}, cond(A) {1:.1f}'.format(host_rel_err, loop_cond))
    assert loop_cond <= 1e4 and host_rel_err <= 1e-8

    out.update(restatement_err=restatement_err, restatement_err_by_separation=by_separation, ax_err=ax_err, host_rel_err=host_rel_err,
               loop_cond=loop_cond)
    path = os.path.join(HERE, 'g26_line_of_sight.npz')
    np.savez_compressed(path, **out)
    print('g26_line_of_sight {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
