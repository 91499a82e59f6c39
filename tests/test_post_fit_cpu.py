"""
CPU checks of the post-fit pass: the argument checks of shg_segment_lag_products before any HIP call, its host rules under a sanitizer
(tools/lags_host_check.cpp, a stand-alone program), the Python checks of lstsq.PostFit before anything reaches the device, and the host
references of tests/golden/postfit_inputs.py against each other.
"""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import arc_inputs as arc
import design_inputs as di
import grates_amd as ga
import los_inputs as li
import postfit_inputs as pf
import whitening_inputs as wi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C entry point ---------------------------------------------------------------------------------------------------------------
def test_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    call = lib.shg_segment_lag_products
    X, seg, S = (ctypes.c_void_p(address) for address in (0x10000000, 0x30000000, 0x40000000))   # never dereferenced

    def error():
        return lib.shg_last_error().decode()
    #    rows M X ldx lags nseg seg S stream
    for rows, M, ldx in ((-1, 10, 10), (6, -1, 10), (6, 10, -1)):
        assert call(rows, M, X, ldx, 5, 2, seg, S, None) == -1
        assert 'shg_segment_lag_products: negative size' in error()
    for lags in (-1, 129, 1 << 20):
        assert call(6, 10, X, 10, lags, 2, seg, S, None) == -1
        assert 'lags {0} outside 0 .. 128'.format(lags) in error()
    assert call(6, 10, X, 10, 5, -1, seg, S, None) == -1
    assert 'nseg -1 is negative' in error()
    assert call(6, 10, X, 9, 5, 2, seg, S, None) == -1
    assert 'ldx 9 below M 10' in error()
    for pointers in ((None, seg, S), (X, None, S), (X, seg, None)):
        assert call(6, 10, pointers[0], 10, 5, 2, pointers[1], pointers[2], None) == -1
        assert 'shg_segment_lag_products: NULL pointer' in error()
    assert call((1 << 20) + 1, 1 << 20, X, 1 << 20, 5, 2, seg, S, None) == -1                              # 2^40 + 2^20 values of X
    assert 'values of X are too large' in error()
    assert call(1 << 20, 4, X, 4, 15, (1 << 16) + 1, seg, S, None) == -1                                    # ... of S alone
    assert 'values of S are too large' in error()
    # nothing to do: no pointer is looked at and no HIP call is made
    assert call(0, 10, None, 10, 5, 2, None, None, None) == 0
    assert call(6, 10, None, 10, 5, 0, None, None, None) == 0
    assert call(6, 10, X, 10, 129, 0, seg, S, None) == -1                                                  # the checks come before the early return
    with pytest.raises(_lib.ShgError, match='lags 129 outside 0 .. 128'):
        _lib.call('shg_segment_lag_products', 6, 10, X, 10, 129, 2, seg, S, None)


def test_host_rules_run_clean_under_a_sanitizer(tmp_path):
    """the argument rules and the launch geometry as a stand-alone CPU program with its own main, built with
    -fsanitize=address,undefined: nothing of it is loaded into Python"""
    compiler = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert compiler, 'a host C++ compiler is needed'
    program = str(tmp_path / 'lags_host_check')
    subprocess.run([compiler, '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'lags_host_check.cpp'),
                    '-o', program], check=True)
    done = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and done.stdout.strip() == 'ok', done.stdout


# ---- PostFit: every check before the device ----------------------------------------------------------------------------------------------
def _constructors():
    """components: the of_* call on five valid points at degrees 0 .. 4 (P = 25)"""
    xyz = di.positions()[:5]
    a, b = (x[:5] for x in li.pairs())
    post = ga.lstsq.PostFit
    return {3: lambda x, **kw: post.of_accelerations(x, xyz, np.ones((5, 3)), 0, 4, **kw),
            4: lambda x, **kw: post.of_gradients(x, xyz, np.ones((5, 4)), 0, 4, components=('xx', 'yy', 'zz', 'xz'), **kw),
            1: lambda x, **kw: post.of_line_of_sight(x, a, b, np.ones(5), 0, 4, **kw)}


def test_post_fit_checks_before_the_device(golden):
    """every ValueError below is raised without a GPU: the checks precede require_gpu"""
    five = wi.sequence(golden('g27_whitening'), 'ar5', ga.lstsq)
    for components, build in _constructors().items():
        for solution in (np.zeros(24), np.zeros((25, 2)), np.zeros((1, 25)), np.zeros(())):
            with pytest.raises(ValueError, match=r'solution must have shape \(25,\) or \(25, 1\)'):
                build(solution)
        for vectors in (np.zeros((24, 3)), np.zeros(25), np.zeros((25, 0)), np.zeros((25, 2, 2))):
            with pytest.raises(ValueError, match=r'vectors must have shape \(25, S\)'):
                build(np.zeros(25), vectors=vectors)
        for model in ([0, 2], np.array([0, 3]), 'arcs', five):                                  # arcs (or a bare noise model) without a model
            with pytest.raises(ValueError, match='model must be None, a ColouredNoise or an ArcParameters'):
                build(np.zeros(25), model=model)
        # the checks of the matching from_* run unchanged
        with pytest.raises(ValueError, match='arcs must'):
            build(np.zeros(25), model=ga.lstsq.ColouredNoise(five, [0, 5]))
        with pytest.raises(ValueError, match='arcs must'):
            build(np.zeros(25), model=ga.lstsq.ArcParameters(np.ones((5, 2)), [1, 2]))
        with pytest.raises(ValueError, match=r'the arc basis must have shape \(5, u\)'):
            build(np.zeros(25), model=ga.lstsq.ArcParameters(np.ones((6, 2))))
        with pytest.raises(ValueError, match='block_points must be positive'):
            build(np.zeros(25), block_points=0)
        with pytest.raises(ValueError, match='weights'):
            build(np.zeros(25), weights=-np.ones(5))
    with pytest.raises(ValueError, match='7 positions but 5 accelerations'):
        ga.lstsq.PostFit.of_accelerations(np.zeros(25), np.ones((7, 3)), np.ones((5, 3)), 0, 4)


def _bare_fit(arcs, count, K=2):
    """a PostFit with the state covariance_function and arc_redundancies check before they touch the device"""
    fit = ga.lstsq.PostFit(None, None, None, None)
    fit.arcs = np.asarray(arcs)
    fit.arc_observation_counts = K * np.diff(np.append(fit.arcs, count))

    class Rows:
        shape = (K, count)
    fit._PostFit__rows, fit._PostFit__traces = Rows, None
    return fit


def test_covariance_function_and_redundancy_arguments():
    fit = _bare_fit([0, 1, 4, 300], 700)
    for lag in (-1, 129, 2.5):
        with pytest.raises(ValueError, match='maximum_lag must be an integer in 0 .. 128'):
            fit.covariance_function(lag)
    short = _bare_fit([0, 3, 7], 10)
    with pytest.raises(ValueError, match='no arc is longer than 4 points: no pair at lag 4'):
        short.covariance_function(5, biased=False)
    with pytest.raises(ValueError, match='need the Monte-Carlo vectors'):
        fit.arc_redundancies()
    with pytest.raises(ValueError, match='need the Monte-Carlo vectors'):
        fit.arc_variance_factors(2.0)


def test_signatures():
    post = ga.lstsq.PostFit
    for name, first in (('accelerations', ['xyz', 'g']), ('gradients', ['xyz', 'gradients']), ('line_of_sight', ['xyz_a', 'xyz_b', 'differences'])):
        plain = [(prm.name, prm.default) for prm in inspect.signature(getattr(ga.lstsq.NormalEquations, 'from_' + name)).parameters.values()]
        plain = [item for item in plain if item[0] not in ('noise_model', 'arcs')]
        mine = [(prm.name, prm.default) for prm in inspect.signature(getattr(post, 'of_' + name)).parameters.values()]
        assert mine == [('solution', inspect.Parameter.empty)] + plain + [('model', None), ('vectors', None)]
        assert [item[0] for item in mine[1:1 + len(first)]] == first
    assert list(inspect.signature(post.covariance_function).parameters) == ['self', 'maximum_lag', 'per_component', 'biased']
    assert [prm.default for prm in inspect.signature(post.covariance_function).parameters.values()][2:] == [False, True]
    for name in ('arc_redundancies', 'arc_variance_factors'):
        assert [(prm.name, prm.default) for prm in inspect.signature(getattr(post, name)).parameters.values()][1:] == [('variance_factor', 1.0)]
    assert list(inspect.signature(ga.engine.segment_lag_products).parameters) == ['X', 'seg', 'lags', 'out']


def test_signatures_of_all_twelve_entry_points():
    """the parameter lists of from_* (NormalEquations, ColouredNoise, ArcParameters) and of_* (PostFit) and of the three constructors,
    written out: names, order and defaults"""
    empty, GM, R = inspect.Parameter.empty, 3.9860044150e+14, 6.3781363000e+06
    tail = [('weights', None), ('block_points', None)]
    kinds = {'accelerations': [('xyz', empty), ('g', empty), ('min_degree', empty), ('max_degree', empty), ('GM', GM), ('R', R)] + tail,
             'gradients': [('xyz', empty), ('gradients', empty), ('min_degree', empty), ('max_degree', empty), ('GM', GM), ('R', R), ('frames', None),
                           ('components', None)] + tail,
             'line_of_sight': [('xyz_a', empty), ('xyz_b', empty), ('differences', empty), ('min_degree', empty), ('max_degree', empty), ('GM', GM), ('R', R),
                               ('directions', None)] + tail}

    def listed(function):
        return [(prm.name, prm.default) for prm in inspect.signature(function).parameters.values()]
    lstsq = ga.lstsq
    checked = 0
    for kind, plain in kinds.items():
        extra = [('noise_model', None), ('arcs', None)] if kind == 'accelerations' else []
        assert listed(getattr(lstsq.NormalEquations, 'from_' + kind)) == plain + extra
        assert listed(getattr(lstsq.ColouredNoise, 'from_' + kind)) == [('self', empty)] + plain
        assert listed(getattr(lstsq.ArcParameters, 'from_' + kind)) == [('self', empty)] + plain
        assert listed(getattr(lstsq.PostFit, 'of_' + kind)) == [('solution', empty)] + plain + [('model', None), ('vectors', None)]
        checked += 4
    assert checked == 12
    assert listed(lstsq.PostFit.__init__) == [('self', empty), ('solution', empty), ('vectors', empty), ('model', empty), ('template', empty)]
    assert listed(lstsq.ColouredNoise.__init__) == [('self', empty), ('noise_model', empty), ('arcs', None)]
    assert listed(lstsq.ArcParameters.__init__) == [('self', empty), ('basis', empty), ('arcs', None), ('noise_model', None), ('keep', True)]


# ---- the host references against each other ------------------------------------------------------------------------------------------------
def test_exact_lag_products_against_a_plain_loop():
    rng = np.random.default_rng(2901)
    X = rng.standard_normal((2, 40)) * np.exp(rng.uniform(-20, 20, (2, 40)))
    for seg in ([0, 1, 4, 30, 40], [3, 3, 17, 39]):
        S, magnitude, pairs = pf.exact_lag_products(X, seg, 6)
        assert np.array_equal(S, pf.plain_lag_products(X, seg, 6))
        lengths = np.maximum(np.diff(seg), 0)
        assert np.array_equal(pairs, np.maximum(lengths[:, None] - np.arange(7), 0))
        assert np.all(S[:, pairs == 0] == 0.0) and np.all(magnitude >= np.abs(S)) and np.all(S[:, :, 0] == magnitude[:, :, 0])
    S, _, _ = pf.exact_lag_products(X, [0, 40], 3)
    assert np.allclose(S[0, 0], [np.dot(X[0, :40 - k], X[0, k:]) for k in range(4)], rtol=1e-12, atol=0)


def test_divisors():
    arcs, M = [0, 1, 4, 300], 700                                                               # lengths 1, 3, 296, 400
    unbiased = pf.divisors(arcs, M, 400, False)
    assert unbiased[0] == 700 and unbiased[1] == 0 + 2 + 295 + 399 and unbiased[2] == 1 + 294 + 398 and unbiased[3] == 293 + 397
    assert unbiased[296] == 104 and unbiased[399] == 1 and unbiased[400] == 0
    assert np.array_equal(unbiased, [sum(max(n - k, 0) for n in (1, 3, 296, 400)) for k in range(401)])
    assert np.array_equal(pf.divisors(arcs, M, 5, True), np.full(6, 700))
    assert np.array_equal(pf.divisors(None if False else [0], M, 2, False), [700, 699, 698])


def test_redundancy_of_an_arc_against_the_hat_matrix():
    """r_a = K len_a - sum_{i in a} H_ii: the hat matrix of the explicit system [A~ B~] (SVD, and numpy.linalg.lstsq) against the way
    the pass forms it, n_a - trace of the projected rows through the inverse of the reduced normals; P = 20, short arcs included"""
    M, K, P, arcs = 60, 3, 20, [0, 1, 4, 30]
    rng = np.random.default_rng(2902)
    root = np.sqrt(rng.uniform(0.25, 4.0, (M, K)))
    A = (rng.standard_normal((K, M, P)) * root.T[:, :, None]).reshape(K * M, P)
    basis = ga.lstsq.arc_basis(arcs, M, degree=1, periods=(23,))
    bounds = arc.bounds_of(arcs, M)
    units = arc.explicit_columns(arc.transformed_basis(basis, root, K), bounds, True)
    F = np.hstack([A] + units)
    diagonal, second = pf.hat_diagonal(F), pf.hat_diagonal_lstsq(F)
    disagreement = np.abs(diagonal - second).max()
    ranks = pf.projectors(units)[1].reshape(4, K)
    assert np.array_equal(ranks, np.repeat([[1], [3], [4], [4]], K, axis=1))
    assert np.array_equal(ranks.ravel(), arc.schur(A, np.zeros(K * M), units)[4])
    expected = pf.hat_redundancies(diagonal, bounds, K, M)
    got = pf.pass_redundancies(A, units, ranks, bounds, K, M)
    print('hat matrix: SVD against lstsq {0:.2e}; redundancies {1} against {2}'.format(disagreement, got, expected))
    assert disagreement <= 1e-12 and np.all(diagonal > -1e-12) and np.all(diagonal < 1 + 1e-12)
    assert np.abs(got - expected).max() <= 1e-10
    assert abs(expected.sum() - (K * M - P - ranks.sum())) <= 1e-10                              # the redundancy of the whole system
    assert abs(expected[0]) <= 1e-10                                                            # one point, one parameter per axis: nothing left
    # the projection removes exactly what the parameters of parameters() explain
    l = rng.standard_normal(K * M)
    y = pf.parameters(l, units)
    assert np.abs(pf.project(l, units) - (l - np.hstack(units) @ y.ravel())).max() <= 1e-11


def test_covariance_reference_is_consistent():
    rng = np.random.default_rng(2903)
    e = rng.standard_normal((700, 4))
    c, bound, pooled, pooled_bound = pf.covariance_function(e, [0, 150, 300], 5, True)
    assert c.shape == bound.shape == (4, 6) and pooled.shape == pooled_bound.shape == (6,)
    assert np.allclose(pooled, c.mean(axis=0), rtol=1e-14, atol=0) and np.all(bound > 0)
    assert np.allclose(c[:, 0], (e * e).mean(axis=0), rtol=1e-14, atol=0)
    unbiased = pf.covariance_function(e, [0, 150, 300], 5, False)[0]
    assert np.allclose(unbiased * pf.divisors([0, 150, 300], 700, 5, False), c * 700, rtol=1e-14, atol=0)
