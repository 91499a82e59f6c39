"""
Golden vectors of the design matrix of the gravitational acceleration (g24_acceleration_design.npz).  Run once with the reference
package `grates` importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_acceleration_design.py

Like make_golden_acceleration.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and
reference outputs.  The reference has no design matrix; A comes column by column from its
PotentialCoefficients.gravitational_acceleration of unit coefficient fields:

    xyz, A8, A2       d/o 8 and d/o 2 at design_inputs.positions(), min_degree 0
    A8_min2, A2_min2  the same from unit fields of degrees >= 2 only (the column slices of the former)

and three scalars, all computed here on the CPU in NumPy:

    restatement_err   design_inputs.restatement (the kernel's formulas in float64 NumPy) against A8 and A2, of max|A|
    ax_err            A @ x against the reference's acceleration of a d/o-60 anomaly field at the positions of the g22 case
                      'static60' (A from 3721 calls of the reference), of max|g|
    host_rel_err      the closed loop of design_inputs.LOOP solved on the host through the normals, |x^ - x| / |x| (2-norms);
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
import acceleration_inputs as ai  # noqa: E402
import design_inputs as di  # noqa: E402


def reference_acceleration(xyz):
    def acceleration(anm):
        gf = grates.gravityfield.PotentialCoefficients(di.GM, di.R)
        gf.anm = anm
        return gf.gravitational_acceleration(xyz)
    return acceleration


def main():
    out = {'xyz': di.positions()}
    restatement_err = 0.0
    for N in di.DEGREES:
        A = di.unit_field_matrix(reference_acceleration(out['xyz']), out['xyz'], 0, N)
        A_min2 = di.unit_field_matrix(reference_acceleration(out['xyz']), out['xyz'], 2, N)
        assert np.all(np.isfinite(A)) and np.array_equal(A_min2, A[:, 4:]), N
        out['A{0}'.format(N)], out['A{0}_min2'.format(N)] = A, A_min2
        err = np.abs(di.restatement(out['xyz'], 0, N) - A).max() / np.abs(A).max()
        restatement_err = max(restatement_err, err)
        print('d/o {0}: A {1}, max|A| {2:.3e}, restatement {3:.2e} of max|A|'.format(N, A.shape, np.abs(A).max(), err))

    tag, N, seed = di.AX
    xyz = ai.positions(tag)
    anm = ai.coefficients(N, 'anomaly', seed)
    acceleration = reference_acceleration(xyz)
    g = acceleration(anm)
    A = di.unit_field_matrix(acceleration, xyz, 0, N)
    ax_err = np.abs(A @ di.ravel(anm, 0, N) - g.ravel()).max() / np.abs(g).max()
    print('A @ x at d/o {0}, {1} points: {2:.2e} of max|g|'.format(N, xyz.shape[0], ax_err))

    loop = di.LOOP
    xyz, anm = di.loop_positions(), di.loop_field()
    acceleration = reference_acceleration(xyz)
    A = di.unit_field_matrix(acceleration, xyz, loop['min_degree'], loop['N'])
    obs = acceleration(anm).ravel()
    x = di.ravel(anm, loop['min_degree'], loop['N'])
    solution = np.linalg.solve(A.T @ A, A.T @ obs)
    host_rel_err = np.linalg.norm(solution - x) / np.linalg.norm(x)
    loop_cond = np.linalg.cond(A)
    print('closed loop on the host: relative error {0:.2e}, cond(A) {1:.1f}'.format(host_rel_err, loop_cond))
    assert loop_cond <= 1e4 and host_rel_err <= 1e-8

    out.update(restatement_err=restatement_err, ax_err=ax_err, host_rel_err=host_rel_err, loop_cond=loop_cond)
    path = os.path.join(HERE, 'g24_acceleration_design.npz')
    np.savez_compressed(path, **out)
    print('g24_acceleration_design {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
