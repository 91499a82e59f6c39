"""
Fixture g34_trsvd_reference.json: the errors of the REFERENCE's own lstsq.trsvd (grates/lstsq.py:1277-1314, NumPy on the CPU) on the two
matrices of tests/test_gpu_eigen.py, k = 12, default iterations, for 20 seeds of numpy.random each.  Run once where the reference is
mounted, like make_golden.py:  python tests/golden/make_g34_trsvd.py.  Only numbers are written.
  values:   max_i |s_i - sigma_i| / sigma_1 against numpy.linalg.svd
  residual: |A - U diag(s) Vt[:k]|_2 / sigma_13
tests/test_gpu_eigen.py allows 4 x the worst of each: the random draws dominate both errors, and the draws differ.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
for _name, _attr in (('netCDF4', 'Dataset'), ('h5py', 'File')):         # file readers the reference imports and trsvd does not use
    if _name not in sys.modules:
        _mod = types.ModuleType(_name)
        setattr(_mod, _attr, None)
        sys.modules[_name] = _mod
sys.dont_write_bytecode = True
sys.path.insert(0, '/root/reference')

import eigen_reference as er  # noqa: E402
import grates.lstsq  # noqa: E402

K, SEEDS, DECAY, MATRIX_SEED = 12, 20, 0.7, 3400


def main():
    out = {'k': K, 'decay': DECAY, 'matrix_seed': MATRIX_SEED, 'seeds': SEEDS, 'cases': {}}
    for m, n in ((300, 200), (200, 300)):
        A = er.spectrum_matrix(m, n, DECAY, MATRIX_SEED + m)
        sigma = np.linalg.svd(A, compute_uv=False)
        values, residual = [], []
        for seed in range(SEEDS):
            np.random.seed(seed)
            U, s, Vt = grates.lstsq.trsvd(A, K)
            values.append(float(np.abs(s - sigma[:K]).max() / sigma[0]))
            residual.append(float(np.linalg.norm(A - (U * s) @ Vt[:K], 2) / sigma[K]))
        out['cases']['{0}x{1}'.format(m, n)] = {'values': values, 'residual': residual, 'worst_values': max(values), 'worst_residual': max(residual)}
    with open(os.path.join(HERE, 'g34_trsvd_reference.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v['worst_values'], v['worst_residual']) for k, v in out['cases'].items()}))


if __name__ == '__main__':
    main()
