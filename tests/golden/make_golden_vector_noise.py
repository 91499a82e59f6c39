"""
Golden vectors of the vector noise models (g35_vector_noise.npz).  Run once with the reference package `grates` importable (for
example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vector_noise.py

Like make_golden_whitening.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and reference
outputs.  The reference has the stochastic model, AutoregressiveModelSequence of dimension K, and no filter; for the VAR(2) process
of dimension 3 of tests/vector_noise_reference.py:

    covariance            [3, 3, 3]: the lags Sigma_0 .. Sigma_2 handed to AutoregressiveModelSequence.from_covariance_function
    coefficients          [3, 2, 3, 3]: entry [s, k - 1] holds B_k of the reference's model of order s, zero beyond
    Q                     [3, 3, 3]: the white-noise covariance of the model of order s
    normals{L}            normal_equations(L).to_array()[0] (upper triangle) for L = 3 and L = 12: Sigma^-1 of L epochs, [3 L, 3 L]
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

sys.path.insert(0, os.path.dirname(HERE))
import vector_noise_reference as vr  # noqa: E402

K, ORDER, LENGTHS = 3, 2, (3, 12)


def main():
    B1, B2, Q = vr.process(K)
    function = vr.covariance_function([B1, B2], Q, ORDER)
    sequence = grates.lstsq.AutoregressiveModelSequence.from_covariance_function(function)
    assert sequence.maximum_order == ORDER and sequence.dimension == K
    models = sequence._AutoregressiveModelSequence__armodels               # the reference has no accessor for them
    out = {'covariance': np.array(function), 'coefficients': np.zeros((ORDER + 1, ORDER, K, K)), 'Q': np.zeros((ORDER + 1, K, K))}
    for s, model in enumerate(models):
        assert model.order == s and model.dimension == K
        for k, coefficient in enumerate(model.coefficients):
            out['coefficients'][s, k] = coefficient
        out['Q'][s] = model.white_noise_covariance
    for L in LENGTHS:
        normals = sequence.normal_equations(L).to_array()[0]
        assert normals.shape == (K * L, K * L)
        out['normals{0}'.format(L)] = normals
    print('B_1 of the model of order 2 against the process: {0:.2e}; Q: {1:.2e}'.format(
        np.abs(out['coefficients'][2, 0] - B1).max(), np.abs(out['Q'][2] - Q).max()))
    path = os.path.join(HERE, 'g35_vector_noise.npz')
    np.savez_compressed(path, **out)
    print('g35_vector_noise {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
