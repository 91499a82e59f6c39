"""
Golden vectors of the decorrelation of coloured observation noise (g27_whitening.npz).  Run once with the reference package `grates`
importable (for example on PYTHONPATH):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_whitening.py

Like make_golden_line_of_sight.py it imports the reference with empty stand-ins for netCDF4 / h5py and stores only inputs and reference
outputs.  The reference has the stochastic model, AutoregressiveModelSequence, and no filter; per process `name` of
whitening_inputs.PROCESSES (scalar AR processes of order p = 2 and p = 5, covariance function of lags 0 .. p as [1, 1] arrays):

    {name}_covariance             the lags 0 .. p handed to AutoregressiveModelSequence.from_covariance_function
    {name}_coefficients           [p + 1, p]: row s holds phi_1 .. phi_s of the reference's model of order s, zero beyond
    {name}_Q                      [p + 1]: the white-noise variance of the model of order s
    {name}_normals{L}             normal_equations(L).to_array()[0] (upper triangle) for L = p + 1 and L = 12: Sigma^-1 of L epochs
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
import whitening_inputs as wi  # noqa: E402


def main():
    out = {}
    for name in sorted(wi.PROCESSES):
        p = wi.order(name)
        function = wi.covariance_function(name)
        out[name + '_covariance'] = np.array([lag[0, 0] for lag in function])
        sequence = grates.lstsq.AutoregressiveModelSequence.from_covariance_function(function)
        assert sequence.maximum_order == p and sequence.dimension == 1
        models = sequence._AutoregressiveModelSequence__armodels               # the reference has no accessor for them
        assert len(models) == p + 1
        coefficients, Q = np.zeros((p + 1, p)), np.zeros(p + 1)
        for s, model in enumerate(models):
            assert model.order == s and model.dimension == 1
            coefficients[s, :s] = [np.asarray(c).reshape(()) for c in model.coefficients]
            Q[s] = np.asarray(model.white_noise_covariance).reshape(())
        out[name + '_coefficients'], out[name + '_Q'] = coefficients, Q
        for L in (p + 1, wi.LENGTHS):
            normals = sequence.normal_equations(L).to_array()[0]
            assert normals.shape == (L, L)
            out['{0}_normals{1}'.format(name, L)] = normals
        print('{0}: p {1}, phi {2}, Q {3}; the process: phi {4}, sigma^2 {5}'.format(name, p, coefficients[p], Q, wi.coefficients(name),
                                                                                   wi.PROCESSES[name][1]))
    path = os.path.join(HERE, 'g27_whitening.npz')
    np.savez_compressed(path, **out)
    print('g27_whitening {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
