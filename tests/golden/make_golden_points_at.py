"""
Golden vectors of the gravitational acceleration of time-variable fields at points, each point at its own epoch
(g32_points_at.npz).  Run once with the reference package `grates` importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_points_at.py

Like make_golden_acceleration.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and reference
outputs.  Per case (points_at_inputs.CASES):
    xyz     [M, 3]   the positions
    mjd     [M]      the epochs as modified Julian dates (whole days + seconds / 86400), iso [M] the same as ISO strings
    g       [M, 3]   the reference's TimeVariableGravityField(constituents).evaluate_at(t_i).gravitational_acceleration(x_i[None]), row by row
    first   [M]      the field of the series before the epoch (np.searchsorted(t, epoch) - 1, 0 at the first node)
    weights [M, W]   the weights of the reference's expressions: tau of the trend, (cos, sin)(2 pi tau) of each cycle, then (1 - w, w)
                     of the series
    scale            max_i sum_j |w_ij| |g_j(x_i)| over the fields j of all constituents, |.| the largest component: the bound of the
                     tests is relative to it, and the generator asserts max|g| >= scale / 4 (no cancellation hides behind it)
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
import points_at_inputs as pi  # noqa: E402


def reference_weights(tag, epochs):
    """(first [M], weights [M, W]) with the reference's expressions (grates/gravityfield.py:940-941, 1089, 1135-1137)"""
    nodes = np.array(pi.series_epochs())
    first, rows = [], []
    for epoch in epochs:
        row = []
        if pi.CASES[tag][2]:
            row.append((epoch - pi.REFERENCE_EPOCH).total_seconds() / (86400 * 365.25))
            for period in pi.PERIODS:
                dt = (epoch - pi.REFERENCE_EPOCH).total_seconds() / (86400 * period)
                row += [np.cos(2 * np.pi * dt), np.sin(2 * np.pi * dt)]
        idx = int(np.searchsorted(nodes, epoch))
        if idx == 0:                                                 # the first node: the reference blends field -1 with 0 and field 0 with 1
            first.append(0)
            row += [1.0, 0.0]
        else:
            weight = (epoch - nodes[idx - 1]).total_seconds() / (nodes[idx] - nodes[idx - 1]).total_seconds()
            first.append(idx - 1)
            row += [1 - weight, weight]
        rows.append(row)
    return np.array(first), np.array(rows)


def main():
    out = {}
    for tag, (N, _, with_model) in pi.CASES.items():
        xyz, epochs = pi.positions(tag), pi.epochs(tag)
        assert xyz.shape[0] == len(epochs)
        tv = grates.gravityfield.TimeVariableGravityField(pi.constituents(tag, grates))
        g = np.vstack([tv.evaluate_at(t).gravitational_acceleration(x[np.newaxis, :]) for t, x in zip(epochs, xyz)])
        assert g.shape == xyz.shape and np.all(np.isfinite(g)), tag
        first, weights = reference_weights(tag, epochs)
        fields = ([pi.field(a, None, grates) for a in pi.model_coefficients(tag)] if with_model else [])
        model = len(fields)
        fields += [pi.field(a, None, grates) for a in pi.series_coefficients(tag)]
        size = np.stack([np.abs(f.gravitational_acceleration(xyz)).max(axis=1) for f in fields], axis=1)      # [M, fields]
        rows = np.arange(xyz.shape[0])
        bound = (np.abs(weights[:, :model]) * size[:, :model]).sum(axis=1) + \
            np.abs(weights[:, model]) * size[rows, model + first] + np.abs(weights[:, model + 1]) * size[rows, model + first + 1]
        scale = float(bound.max())
        assert np.abs(g).max() >= scale / 4, (tag, np.abs(g).max(), scale)
        out['xyz_' + tag] = xyz
        out['mjd_' + tag] = np.array([pi.mjd(t) for t in epochs])
        out['iso_' + tag] = np.array([t.isoformat() for t in epochs])
        out['g_' + tag] = g
        out['first_' + tag] = first
        out['weights_' + tag] = weights
        out['scale_' + tag] = np.array(scale)
        print('{0:10s} d/o {1:3d} points {2:3d} max|g| {3:.3e} scale {4:.3e}'.format(tag, N, xyz.shape[0], np.abs(g).max(), scale))
    path = os.path.join(HERE, 'g32_points_at.npz')
    np.savez_compressed(path, **out)
    print('g32_points_at {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
