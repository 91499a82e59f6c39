"""
The long double reference of tests/factorisation_reference.py against LAPACK, its inputs, and the solver's formulation emulated on the
host (no GPU): what the bounds of tests/test_gpu_factorisation_seams.py are made of.

The emulation does in float64, with LAPACK for the 128 x 128 leaves, what csrc/blas.hip does: 128-column panels, U12 = X11^T A12 with the
explicit inverse X11 of the diagonal factor block, A22 -= U12^T U12, the inverse grown by block columns X_0..k-1,k = -X_0..k-1,0..k-1
(U_0..k-1,k X_kk), and x = X (X^T b) in place of the two triangular solves.  It has to stay within 2 times LAPACK in all three figures
on every input of the conditioning test: the factor 2 is a condition on the inputs (if the formulation itself lost accuracy on one of
them, a bound of "10 times LAPACK" on the kernels would be asking for the wrong thing).
"""

import numpy as np
import pytest
import scipy.linalg as la

import factorisation_reference as fr


def lapack_inverse_of_factor(Uf):
    X, info = la.lapack.dtrtri(np.asfortranarray(Uf), lower=0)
    assert info == 0
    return X


def emulate(A, b, panel=128):
    """(U, X, x) of the solver's formulation in float64"""
    n = A.shape[0]
    W = np.triu(A).copy()
    X = np.zeros((n, n))
    starts = list(range(0, n, panel))
    for k0 in starts:
        k1 = min(k0 + panel, n)
        W[k0:k1, k0:k1] = la.cholesky(W[k0:k1, k0:k1], lower=False)
        X[k0:k1, k0:k1] = lapack_inverse_of_factor(W[k0:k1, k0:k1])
        if k1 < n:
            W[k0:k1, k1:] = X[k0:k1, k0:k1].T @ W[k0:k1, k1:]
            W[k1:, k1:] -= np.triu(W[k0:k1, k1:].T @ W[k0:k1, k1:])
    for k0 in starts[1:]:
        k1 = min(k0 + panel, n)
        X[:k0, k0:k1] = -X[:k0, :k0] @ (W[:k0, k0:k1] @ X[k0:k1, k0:k1])
    return W, X, X @ (X.T @ b)


def own_inverse_error(X, Uf):
    """inverse_error of X as the inverse of the factor it was computed from"""
    return fr.inverse_error(X, Uf, fr.triangular_inverse(Uf))


def right_hand_sides(n, seed):
    return np.random.default_rng(seed + 1).standard_normal((n, 3))


@pytest.mark.parametrize('n', [1, 2, 33, 129, 300])
def test_reference_agrees_with_lapack(n):
    A, Uf, X = fr.reference(n, 1e2, n)
    ref = la.cholesky(A, lower=False)
    assert np.max(np.abs(Uf - ref)) <= 1e-13 * np.max(np.abs(ref))
    Xl = lapack_inverse_of_factor(ref)
    assert np.max(np.abs(X - Xl)) <= 1e-13 * np.max(np.abs(Xl))
    assert np.array_equal(np.tril(X, -1), np.zeros_like(X)) and np.array_equal(np.tril(Uf, -1), np.zeros_like(Uf))
    b = right_hand_sides(n, n)
    xl = la.cho_solve((ref, False), b)
    assert np.max(np.abs(fr.solve(Uf, b) - xl)) <= 1e-13 * np.max(np.abs(xl))
    assert np.max(np.abs(fr.solve(Uf, b[:, 0]) - xl[:, 0])) <= 1e-13 * np.max(np.abs(xl))
    Zl = la.cho_solve((ref, False), np.eye(n))
    assert np.max(np.abs(fr.inverse_from_factor(Uf) - Zl)) <= 1e-13 * np.max(np.abs(Zl))
    # the figures of a long double result against itself and against float64 LAPACK
    assert fr.scaled_residual(Uf, A) < 1e-18 and fr.inverse_error(X, Uf, X) == 0.0 and fr.forward_error(xl, xl) == 0.0
    assert fr.scaled_residual(ref, A) < 10 * max(n, 4) * fr.U


def test_reference_reads_the_upper_triangle_only():
    A, Uf, _ = fr.reference(33, 1e2, 33)
    junk = A.copy()
    junk[np.tril_indices(33, -1)] = np.nan
    got, p = fr.cholesky_upper(junk)
    assert p == 0 and np.array_equal(got, Uf)


def lapack_pivot(A):
    with pytest.raises(np.linalg.LinAlgError) as err:
        la.cholesky(A, lower=False)
    message = str(err.value)
    assert '-th leading minor' in message
    return int(message.split('-th leading minor')[0].split()[-1])


@pytest.mark.parametrize('n,pivots', [(fr.PIVOT_N, fr.PIVOTS), (fr.WALKER_N, fr.WALKER_PIVOTS), (fr.WALKER_CUT[2] - fr.WALKER_CUT[1], fr.WALKER_SCHUR_PIVOTS)])
def test_first_bad_minor_is_where_it_says(n, pivots):
    """every (n, p) of the GPU tests: the reference and LAPACK report p"""
    for p in pivots:
        A = fr.first_bad_minor(n, p, p)
        assert fr.cholesky_upper(A)[1] == p, (n, p)
        assert lapack_pivot(A) == p, (n, p)
    good = fr.first_bad_minor(n, 0, 0)
    assert fr.cholesky_upper(good)[1] == 0
    la.cholesky(good, lower=False)


def test_semidefinite_and_nan_inputs():
    A = fr.semidefinite_rank1(fr.RANK1_N)
    assert fr.cholesky_upper(A)[1] == 2 and lapack_pivot(A) == 2
    good, _, _ = fr.reference(fr.PIVOT_N, 1e2, fr.PIVOT_N)
    for i, j in fr.NAN_SITES:
        assert fr.cholesky_upper(fr.with_nan(good, i, j))[1] == j + 1, (i, j)


@pytest.mark.parametrize('n', fr.GRADED_N)
def test_graded_scales_exactly(n):
    A = fr.spd_spectrum(n, 1e4, n)
    Ag, e = fr.graded(A, n)
    assert e.min() >= -40 and e.max() <= 40 and e.min() < -20 and e.max() > 20
    for i in range(n):
        for j in range(n):
            assert Ag[i, j] == A[i, j] * 2.0 ** int(e[i] + e[j])             # bit for bit (2^(e_i + e_j) is exact, and so is the product)
    assert np.array_equal(Ag, Ag.T) and np.isfinite(Ag).all()
    # the figures do not see the scaling: the reference factor of D A D is U D, its inverse D^-1 X
    _, Uf, X = fr.reference(n, 1e4, n)
    Ug, p = fr.cholesky_upper(Ag)
    assert p == 0 and np.array_equal(Ug, np.ldexp(Uf, e[None, :]))
    assert np.array_equal(fr.triangular_inverse(Ug), np.ldexp(X, -e[:, None]))


@pytest.mark.parametrize('n,kappa,seed,bounds', fr.CONDITIONING)
def test_formulation_within_twice_lapack(n, kappa, seed, bounds):
    A, Uf, X = fr.reference(n, kappa, seed)
    b = right_hand_sides(n, seed)
    x_ref = fr.solve(Uf, b)
    Ul = la.cholesky(A, lower=False)
    lapack = (fr.forward_error(la.cho_solve((Ul, False), b), x_ref), fr.scaled_residual(Ul, A), own_inverse_error(lapack_inverse_of_factor(Ul), Ul))
    Ue, Xe, xe = emulate(A, b)
    ours = (fr.forward_error(xe, x_ref), fr.scaled_residual(Ue, A), own_inverse_error(Xe, Ue))
    ratios = tuple(o / l for o, l in zip(ours, lapack))
    print('n = {0} kappa = {1:.0e}: LAPACK forward {2:.3e} residual {3:.3e} inverse {4:.3e}; emulation / LAPACK {5:.2f} {6:.2f} {7:.2f}'.format(
        n, kappa, *lapack, *ratios))
    assert max(ratios) <= 2.0, ratios
