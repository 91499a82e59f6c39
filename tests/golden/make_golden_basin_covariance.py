"""
Golden vectors of the basin functionals and basin covariances (g21_basin_covariance.npz).  Run once where the reference is available:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_basin_covariance.py

Like make_golden_basin.py it imports the reference package with empty stand-ins for netCDF4 / h5py and stores only inputs and reference
outputs.  Per case (basin_covariance_inputs.CASES): the reference's masks of the four basins (np.packbits), its functionals
F = (area * mask) @ synthesis_matrix(...) / sum(area * mask) and F Sigma F^T; for the 'ewh' cases also both with the reference's
Gaussian filter matrix W (F W and F W Sigma W^T F^T).
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
sys.path.insert(0, '/root/reference')
import grates  # noqa: E402

sys.path.insert(0, HERE)
import basin_covariance_inputs as ci  # noqa: E402


def main():
    out = {}
    grids = dict(ci.grids(grates.grid))
    basins = ci.basins(grates.grid)
    for gtag, grid in grids.items():
        masks = np.array([grid.create_mask(b) for b in basins])
        assert masks[-1].sum() == 0 and all(m.sum() > 0 for m in masks[:-1]), gtag
        out['masks_' + gtag] = np.packbits(masks, axis=1)
        out['count_' + gtag] = np.array([masks.shape[1], masks.shape[0]])
        print('{0:10s} points {1:6d} inside {2}'.format(gtag, masks.shape[1], masks.sum(axis=1)))
    for gtag, kernel, nmin in ci.CASES:
        grid = grids[gtag]
        masks = np.unpackbits(out['masks_' + gtag], axis=1, count=int(out['count_' + gtag][0])).astype(bool)
        area = grid.area if grid.area is not None else np.ones(grid.point_count)
        A = grid.synthesis_matrix(nmin, ci.MAX_DEGREE, kernel)
        with np.errstate(invalid='ignore', divide='ignore'):
            F = (area * masks) @ A / np.sum(area * masks, axis=1)[:, None]
        S = ci.sigma(*ci.covariance(nmin))
        t = ci.tag(gtag, kernel, nmin)
        out['F_' + t] = F
        out['C_' + t] = F @ S @ F.T
        if (gtag, kernel, nmin) in ci.FILTERED:
            W = grates.filter.Gaussian(ci.FILTER_RADIUS).matrix(nmin, ci.MAX_DEGREE)
            out['FW_' + t] = F @ W
            out['CW_' + t] = (F @ W) @ S @ (F @ W).T
    path = os.path.join(HERE, 'g21_basin_covariance.npz')
    np.savez_compressed(path, **out)
    print('g21_basin_covariance {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
