"""
Golden vectors of the gravitational acceleration at points (g22_acceleration.npz).  Run once with the reference package `grates`
importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_acceleration.py

Like make_golden_basin.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and reference
outputs.  Per case (acceleration_inputs.CASES): the positions xyz [M, 3] and the reference's
PotentialCoefficients.gravitational_acceleration(xyz) of the seeded coefficients.
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


def main():
    out = {}
    for tag, (N, kind, seed, _) in ai.CASES.items():
        gf = grates.gravityfield.PotentialCoefficients(ai.GM, ai.R)
        gf.anm = ai.coefficients(N, kind, seed)
        xyz = ai.positions(tag)
        g = gf.gravitational_acceleration(xyz)
        assert np.all(np.isfinite(g)), tag
        out['xyz_' + tag] = xyz
        out['g_' + tag] = g
        print('{0:12s} d/o {1:3d} points {2:4d} max|g| {3:.3e}'.format(tag, N, xyz.shape[0], np.abs(g).max()))
    path = os.path.join(HERE, 'g22_acceleration.npz')
    np.savez_compressed(path, **out)
    print('g22_acceleration {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
