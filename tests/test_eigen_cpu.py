"""
CPU checks of the dense eigen and singular value decompositions: the NumPy model of shg_jacobi_svd and engine.syev
(tests/eigen_reference.py: the kernel's tournament order, threshold, rotation formula and shift) against LAPACK, the round-robin
schedule itself, shg_jacobi_svd's argument checks (before any HIP call), the signatures of the lstsq names against the reference's
(tests/golden/g19_api.json) and the ValueErrors of teigh, trsvd and UnscentedTransformSymmetric, which fire before anything reaches
the device.
"""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest

import grates_amd as ga
import eigen_reference as er

SIZES = [1, 2, 3, 33, 64]


@pytest.mark.parametrize('c', [1, 2, 3, 4, 7, 64, 65, 128])
def test_tournament_meets_every_pair_once(c):
    m = (c + 1) & ~1
    seen = []
    for s in range(m - 1):
        pairs = er.stage_pairs(c, s)
        flat = [i for pq in pairs for i in pq]
        assert len(flat) == len(set(flat)) and len(pairs) == c // 2      # disjoint, floor(c / 2) pairs
        assert all(0 <= p < q < c for p, q in pairs)
        seen += pairs
    assert sorted(seen) == [(p, q) for p in range(c) for q in range(p + 1, c)]


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', er.KINDS[:3])
def test_syev_model_against_lapack(kind, n):
    A = er.matrix(kind, n, 100 + n)
    w, v, sweeps, shift = er.syev_model(A)
    assert 1 <= sweeps <= 30
    b = er.bound(sweeps, n)
    dw, residual, orthogonality = er.eigen_figures(er.mirror_upper(A), w, v, shift)
    assert dw <= b and residual <= b and orthogonality <= b, (dw, residual, orthogonality, b)
    assert (np.diff(w) >= 0).all()


@pytest.mark.parametrize('n', SIZES)
def test_syev_model_reads_the_upper_triangle_only(n):
    A = er.matrix('general', n, 200 + n)
    w, v, _, _ = er.syev_model(A)
    w2, v2, _, _ = er.syev_model(np.triu(A) + np.tril(np.full((n, n), np.nan), -1))
    assert np.array_equal(w, w2) and np.array_equal(v, v2)
    assert er.eigen_figures(er.mirror_upper(A), w, v, er.gershgorin_shift(er.mirror_upper(A)))[0] <= er.bound(30, n)


@pytest.mark.parametrize('r,c', [(n, n) for n in SIZES] + [(40, 5), (7, 7)])
def test_jacobi_model_against_lapack(r, c):
    G = er.matrix('general', c, 300 + r + c, rows=r)
    Go, V, sigma, sweeps = er.jacobi_model(G)
    assert 1 <= sweeps <= 30
    b = er.bound(sweeps, c)
    figures = er.svd_figures(G, Go, V, sigma)
    assert max(figures) <= b, (figures, b)


def test_without_the_shift_a_plus_minus_pair_mixes():
    """why engine.syev shifts: one-sided Jacobi on A itself diagonalises A^2, where lambda and -lambda are one double eigenvalue"""
    A = er.matrix('pairs', 8, 5)
    _, V, _, _ = er.jacobi_model(A)
    w = np.sort(np.einsum('ij,ij->j', V, A @ V))
    assert np.abs(w - np.linalg.eigvalsh(A)).max() > 1e-3
    assert er.eigen_figures(A, *er.syev_model(A)[:2], er.gershgorin_shift(A))[0] <= er.bound(30, 8)


def test_model_edges():
    G = np.zeros((5, 3))
    G[:, 1] = [3.0, 0.0, 4.0, 0.0, 0.0]
    Go, V, sigma, sweeps = er.jacobi_model(G)
    assert sweeps == 1 and np.array_equal(Go, G) and np.array_equal(V, np.eye(3)) and np.array_equal(sigma, [0.0, 5.0, 0.0])
    G[2, 2] = np.nan
    assert er.jacobi_model(G)[3] == 1                              # non-finite input: no rotation, one sweep
    assert er.jacobi_model(np.ones((1, 1)))[3] == 1
    assert er.gershgorin_shift(np.array([[2.0, -1.0], [-1.0, 2.0]])) == 0.0
    assert er.gershgorin_shift(np.array([[0.0, 3.0], [3.0, -1.0]])) == 4.0


def test_entry_point_rejects_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(0x1000)                                 # never dereferenced: validation fails first

    def call(G=dummy, ldg=8, strideG=64, V=dummy, ldv=8, strideV=64, sigma=dummy, r=8, c=8, batch=1, max_sweeps=30, sweeps=dummy):
        return lib.shg_jacobi_svd(G, ldg, strideG, V, ldv, strideV, sigma, r, c, batch, max_sweeps, sweeps, None)
    for bad in (dict(r=0), dict(c=0), dict(r=129, ldg=129), dict(c=129, ldg=129, ldv=129), dict(r=-1)):
        assert call(**bad) == -1
        assert 'outside 1 .. 128' in lib.shg_last_error().decode()
    for bad, text in ((dict(batch=0), 'batch 0 below 1'), (dict(max_sweeps=0), 'max_sweeps 0 below 1'), (dict(ldg=7), 'ldg 7 or ldv 8 below'),
                      (dict(ldv=7), 'ldg 8 or ldv 7 below'), (dict(batch=2, strideG=63), 'below the extent of one matrix'),
                      (dict(batch=2, strideV=63), 'below the extent of one matrix')):
        assert call(**bad) == -1
        assert text in lib.shg_last_error().decode()
    for missing in ('G', 'V', 'sigma', 'sweeps'):
        assert call(**{missing: None}) == -1
        assert 'NULL pointer' in lib.shg_last_error().decode()


# ---- the public names ----------------------------------------------------------------------------------------------------------------
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g19_api.json')) as _f:
    API = json.load(_f)['modules']['lstsq']


def _params(obj):
    """[name, kind, has a default] of every parameter, as tests/golden/make_golden.py records them"""
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in inspect.signature(obj).parameters.values()]


def _compatible(ref, own):
    """the rule of tests/test_api_signatures.py: the reference's leading parameters by name, kind and default; appended ones have defaults"""
    assert len(own) >= len(ref), (ref, own)
    for r, o in zip(ref, own):
        assert r[0] == o[0] and r[1] == o[1], (r, o)
        assert (r[2] is None) == (o[2] is None), (r, o)
        assert r[2] is None or r[2] == o[2] or r[2].startswith('<instance of'), (r, o)
    for extra in own[len(ref):]:
        assert extra[2] is not None or extra[1] in ('VAR_POSITIONAL', 'VAR_KEYWORD'), extra


@pytest.mark.parametrize('name', ['teigh', 'trsvd', 'robust_least_squares'])
def test_function_has_the_reference_signature(name):
    assert API[name]['kind'] == 'function'
    _compatible(API[name]['signature'], _params(getattr(ga.lstsq, name)))


def test_unscented_transform_has_the_reference_members():
    cls = ga.lstsq.UnscentedTransformSymmetric
    members = API['UnscentedTransformSymmetric']['members']
    assert sorted(members) == ['__init__', 'average', 'set_size', 'sigma_point_covariance', 'sigma_points', 'weights']
    for name, ref in members.items():
        if isinstance(ref, str):
            assert isinstance(inspect.getattr_static(cls, name), property)
        else:
            _compatible(ref, _params(getattr(cls, name)))
    ut = cls(7, 0.3)
    assert ut.set_size == 15 and ut.dim == 7 and ut.w0 == 0.3
    w, wc = ut.weights()
    assert w is wc and w.shape == (15,) and w[0] == 0.3 and np.array_equal(w[1:], np.full(14, 0.5 * (1 - 0.3) / 7))
    assert abs(w.sum() - 1.0) <= 4 * er.U


def test_appended_parameters():
    sig = inspect.signature(ga.lstsq.teigh)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [('tolerance', 1e-12), ('max_iter', 100), ('generator', None)]
    sig = inspect.signature(ga.lstsq.trsvd)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[3:]] == [('generator', None)]
    for name in ('jacobi_svd', 'syev'):
        assert inspect.signature(getattr(ga.engine, name)).parameters['max_sweeps'].default == 30
    assert list(inspect.signature(ga.engine.orthonormalise).parameters) == ['B']


def _no_device(monkeypatch):
    def refuse():
        raise AssertionError('the device was reached before the arguments were checked')
    monkeypatch.setattr(ga.engine, 'require_gpu', refuse)


def test_teigh_value_errors_fire_on_the_host(monkeypatch):
    _no_device(monkeypatch)
    for M, k in ((np.zeros((4, 5)), 2), (np.zeros(4), 1), (np.zeros((4, 4)), 0), (np.zeros((4, 4)), 5), (np.zeros((4, 4)), 1.5),
                 (np.zeros((129, 129)), 113), (np.zeros((300, 300)), 128)):
        with pytest.raises(ValueError, match='teigh'):
            ga.lstsq.teigh(M, k)
    with pytest.raises(ValueError, match='max_iter'):
        ga.lstsq.teigh(np.zeros((4, 4)), 2, max_iter=0)
    with pytest.raises(AssertionError):                     # 112 pairs of a 129 x 129 matrix and 128 of a 128 x 128 one are in range
        ga.lstsq.teigh(np.zeros((129, 129)), 112)
    with pytest.raises(AssertionError):
        ga.lstsq.teigh(np.zeros((128, 128)), 128)


def test_trsvd_value_errors_fire_on_the_host(monkeypatch):
    _no_device(monkeypatch)
    for A, k in ((np.zeros(7), 1), (np.zeros((300, 200)), 129), (np.zeros((300, 200)), 0), (np.zeros((20, 10)), 11), (np.zeros((10, 20)), 11)):
        with pytest.raises(ValueError, match='trsvd'):
            ga.lstsq.trsvd(A, k)
    with pytest.raises(ValueError, match='iteration_count'):
        ga.lstsq.trsvd(np.zeros((20, 10)), 3, iteration_count=-1)
    with pytest.raises(AssertionError):
        ga.lstsq.trsvd(np.zeros((300, 200)), 128)


def test_sigma_points_value_errors_fire_on_the_host(monkeypatch):
    _no_device(monkeypatch)
    ut = ga.lstsq.UnscentedTransformSymmetric(3, 0.5)
    for x0, w, v in ((np.zeros(5), np.zeros(3), np.zeros((4, 3))), (np.zeros(4), np.zeros(2), np.zeros((4, 3))), (np.zeros(4), np.zeros(2), np.zeros((4, 2)))):
        with pytest.raises(ValueError, match='sigma_points'):
            ut.sigma_points(x0, w, v)
