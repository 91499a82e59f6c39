"""
Golden vectors of the surface synthesis of radial basis functions and of its formal errors (g31_rbf_surface.npz).  Run once with the
reference package `grates` importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rbf_surface.py

Like make_golden_radial_basis.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and reference
outputs.  The reference reaches a grid from node values through its conversion: a column of S is
RadialBasisFunctions.to_potential_coefficients().to_grid(IrregularGrid(lon, lat, a, f), kernel) with one node value set to 1 (K is zero
below min_degree: to_potential_coefficients sums all degrees), and the standard deviations are
IrregularGrid.covariance_propagation(F C F^T, ...) with F = to_potential_coefficients_matrix() and the seeded C = B B^T / J of
rbf_surface_inputs.covariance.  Per case of rbf_surface_inputs.CASES (band 0..8 and 2..8 with 24 scattered nodes on GRS80, band 2..2
with 3; 40 scattered grid points, one exactly above each of the first three nodes and one antipodal to each) and per kernel of
rbf_surface_inputs.KERNELS (ewh, potential, geoid, anomaly):

    lon_<case>, lat_<case>, k_<case>          the nodes [rad, geodetic] and the degree factors k_n (those of g29_radial_basis.npz)
    glon_<case>, glat_<case>                  the grid points [46]
    kn_<case>_<kernel> [46, N + 1]            the reference's surface factors (1 / k_n)(R / r)^(n+1) GM / R of the grid points
    S_<case>_<kernel> [46, J]                 the reference's surface synthesis, column by column
    sigma_<case>_<kernel> [46]                the reference's standard deviations
    S_err_<case> [4], sigma_err_<case> [4]    rbf_surface_inputs.surface and .sigmas (the kernels' operation order in float64 NumPy) against
                                              them, per kernel: max|S - S_ref| / max|S_ref| and max|sigma - sigma_ref| / max sigma_ref

and the d/o-96 case (8 nodes, flat shape factors in 2..96, 60 points, ewh): lon_n96, lat_n96, k_n96, glon_n96, glat_n96, kn_n96,
S_n96, sigma_n96, S_err_n96, sigma_err_n96.  Every sigma of the fixture is above 1e-4 of the largest of its case (asserted here), so the
relative measure means something at every point.
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
import rbf_surface_inputs as si  # noqa: E402


def reference_case(lon, lat, k, min_degree, glon, glat, kernel, C):
    """(kn [M, N + 1], S [M, J], sigma [M]) of the reference"""
    N, J = k.size - 1, lon.size
    basis = grates.gravityfield.RadialBasisFunctions(grates.grid.IrregularGrid(lon, lat, a=si.A, f=si.F), ri.shape_factors(k), min_degree, N, si.GM, si.R)
    grid = grates.grid.IrregularGrid(glon, glat, a=si.A, f=si.F)
    columns = []
    for values in np.eye(J):
        basis.values = np.ascontiguousarray(values)
        columns.append(basis.to_potential_coefficients().to_grid(grid, kernel).values.copy())
    S = np.stack(columns, axis=1)
    Fm = basis.to_potential_coefficients_matrix()
    sigma = grid.copy().covariance_propagation(Fm @ C @ Fm.T, min_degree, N, kernel, si.GM, si.R)
    colat = grates.utilities.colatitude(glat, si.A, si.F)
    radius = grates.utilities.geocentric_radius(glat, si.A, si.F)
    kn = grates.kernel.get_kernel(kernel).inverse_coefficients(0, N, radius, colat) * np.power((si.R / radius)[:, np.newaxis], np.arange(N + 1, dtype=int) + 1) \
        * si.GM / si.R
    return kn, S, sigma


def restated(lon, lat, k, min_degree, glon, glat, kn, C):
    S = si.surface(ri.node_table(lon, lat), k, min_degree, si.unit_vectors(glon, glat), kn)
    return S, si.sigmas(S, C)


def main():
    out = {}
    for tag, (min_degree, max_degree, count, _) in si.CASES.items():
        lon, lat = ri.case_nodes(tag)
        k = ri.degree_factors(min_degree, max_degree)
        glon, glat = si.grid_points(tag)
        C = si.covariance(count, si.COVARIANCE_SEED[tag])
        out.update({'lon_' + tag: lon, 'lat_' + tag: lat, 'k_' + tag: k, 'glon_' + tag: glon, 'glat_' + tag: glat})
        S_err, sigma_err = [], []
        for kernel in si.KERNELS:
            kn, S, sigma = reference_case(lon, lat, k, min_degree, glon, glat, kernel, C)
            assert np.all(np.isfinite(S)) and np.all(np.isfinite(sigma)) and np.all(np.isfinite(kn[:, min_degree:]))
            assert sigma.min() > 1e-4 * sigma.max(), (tag, kernel, sigma.min() / sigma.max())
            mine, mine_sigma = restated(lon, lat, k, min_degree, glon, glat, kn, C)
            S_err.append(np.abs(mine - S).max() / np.abs(S).max())
            sigma_err.append(np.abs(mine_sigma - sigma).max() / sigma.max())
            special = np.abs(mine - S)[si.SCATTERED:].max() / np.abs(S).max()
            print('{0} {1}: max|S| {2:.3e}, restatement {3:.2e} of it ({4:.2e} at the points above and antipodal to a node); sigma {5:.3e} .. {6:.3e}, '
                  'restatement {7:.2e} of the largest'.format(tag, kernel, np.abs(S).max(), S_err[-1], special, sigma.min(), sigma.max(), sigma_err[-1]))
            out.update({'kn_{0}_{1}'.format(tag, kernel): kn, 'S_{0}_{1}'.format(tag, kernel): S, 'sigma_{0}_{1}'.format(tag, kernel): sigma})
        out.update({'S_err_' + tag: np.array(S_err), 'sigma_err_' + tag: np.array(sigma_err)})

    c = si.N96
    lon, lat = ri.n96_nodes()
    k = ri.degree_factors(c['min_degree'], c['max_degree'], flat=True)
    glon, glat = si.n96_points()
    C = si.covariance(lon.size, si.COVARIANCE_SEED['n96'])
    kn, S, sigma = reference_case(lon, lat, k, c['min_degree'], glon, glat, c['kernel'], C)
    assert np.all(np.isfinite(S)) and sigma.min() > 1e-4 * sigma.max()
    mine, mine_sigma = restated(lon, lat, k, c['min_degree'], glon, glat, kn, C)
    S_err, sigma_err = np.abs(mine - S).max() / np.abs(S).max(), np.abs(mine_sigma - sigma).max() / sigma.max()
    print('n96 {0}: max|S| {1:.3e}, restatement {2:.2e} of it; sigma {3:.3e} .. {4:.3e}, restatement {5:.2e} of the largest'.format(
        c['kernel'], np.abs(S).max(), S_err, sigma.min(), sigma.max(), sigma_err))
    out.update(lon_n96=lon, lat_n96=lat, k_n96=k, glon_n96=glon, glat_n96=glat, kn_n96=kn, S_n96=S, sigma_n96=sigma, S_err_n96=S_err, sigma_err_n96=sigma_err)

    path = os.path.join(HERE, 'g31_rbf_surface.npz')
    np.savez_compressed(path, **out)
    print('g31_rbf_surface {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
