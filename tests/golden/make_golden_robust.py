"""
Golden vectors of the robust (Huber) least squares adjustment (g32_robust.npz).  Run once with the reference package `grates`
importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_robust.py

Like make_golden_whitening.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and reference
outputs: l [200], A [200, 6] of leverage_inputs.robust_problem(True) and x_hat, C, outlier_flag of the reference's
robust_least_squares(l, A, max_iter=1).  A has orthonormal columns and the one iteration runs at unit weights: the one setting in which
the reference's formulas (the inverse of A_bar^T A, the redundancy 1 - sum(A_bar^2, axis=1)) are those of the textbook estimator.
The script checks that the reference flags exactly the five planted observations.
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
import leverage_inputs as lev  # noqa: E402


def main():
    l, A, truth, planted = lev.robust_problem(True)
    x_hat, C, outlier_flag = grates.lstsq.robust_least_squares(l.copy(), A.copy(), max_iter=1)
    assert np.array_equal(np.flatnonzero(outlier_flag), planted), np.flatnonzero(outlier_flag)
    np.savez_compressed(os.path.join(HERE, 'g32_robust.npz'), l=l, A=A, truth=truth, planted=planted, x_hat=x_hat, C=C, outlier_flag=outlier_flag)
    print('g32_robust.npz: flags', np.flatnonzero(outlier_flag), 'sigma0^2', C[0, 0] / np.linalg.inv(A.T @ A)[0, 0])


if __name__ == '__main__':
    main()
