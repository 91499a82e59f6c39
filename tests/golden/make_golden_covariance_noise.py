"""
Golden vectors of noise given by a covariance function (g33_covariance_noise.npz).  Run once with the reference package `grates`
importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_covariance_noise.py

Like make_golden_whitening.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and reference
outputs: for the covariance function of covariance_noise_inputs.covariance at q = 40,

    covariance                    the lags 0 .. 40 handed to AutoregressiveModelSequence.from_covariance_function
    coefficients                  [41, 40]: row s holds phi_1 .. phi_s of the reference's model of order s, zero beyond
    variances                     [41]: the white-noise variance of the model of order s
    normals{L}                    normal_equations(L).to_array()[0] (upper triangle) for L = 41 and L = 60
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
import covariance_noise_inputs as ci  # noqa: E402


def main():
    q = ci.ORDER
    function = ci.covariance_function(q + 1)
    out = {'covariance': np.array([lag[0, 0] for lag in function])}
    sequence = grates.lstsq.AutoregressiveModelSequence.from_covariance_function(function)
    assert sequence.maximum_order == q and sequence.dimension == 1
    models = sequence._AutoregressiveModelSequence__armodels                   # the reference has no accessor for them
    assert len(models) == q + 1
    coefficients, variances = np.zeros((q + 1, q)), np.zeros(q + 1)
    for s, model in enumerate(models):
        assert model.order == s and model.dimension == 1
        coefficients[s, :s] = [np.asarray(c).reshape(()) for c in model.coefficients]
        variances[s] = np.asarray(model.white_noise_covariance).reshape(())
    out['coefficients'], out['variances'] = coefficients, variances
    for L in ci.LENGTHS:
        normals = sequence.normal_equations(L).to_array()[0]
        assert normals.shape == (L, L)
        out['normals{0}'.format(L)] = normals
    path = os.path.join(HERE, 'g33_covariance_noise.npz')
    np.savez_compressed(path, **out)
    print('g33_covariance_noise {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
