"""
The dense Cholesky factorisation behind every normal-equation solve -- the leaf kernel and the three sweeps of csrc/blas.hip
(potrf_upper, potrf_inverse_rec, potrf_inverse_lookahead) and the block walker of csrc/blockchol.hip -- at its seams: the pivot index
on every path, every size next to a border of the leaf's 32-row groups and of the 128-column panels, ill-conditioned and graded
matrices, and memory that must not be read or written.  References, figures and inputs: tests/factorisation_reference.py (long double,
nothing of the library); what LAPACK and the formulation itself deliver on the same inputs: tests/test_factorisation_reference_cpu.py.

Doors (`factor`):
  right      engine.potrf (potrf_upper: blocked right-looking sweep), X from engine.trtri of that factor
  recursive  one-block table through engine.block_potrf with the look-ahead off (potrf_inverse_rec), inverse in a buffer of its own
  lookahead  the same with the look-ahead on (potrf_inverse_lookahead for n > 256)
  in_place   look-ahead on, the inverse takes the place of the block: X only, the same bits as 'lookahead'
  pair       engine.block_potrf_pair with two one-block tables holding two different matrices (one flag per item)

Bounds.  L is LAPACK's figure on the same input, computed here with SciPy; u = 2^-53.  scaled_residual(U) and inverse_error(X) (of X
against the long double inverse of the factor it was computed from) are at most 10 max(L, n u): "within 10 times the host" is the
project's convention, and the floor n u, below the classical gamma(n + 1), only keeps L = 0 at n = 1 from emptying the bound.
"""

import functools

import numpy as np
import pytest
import scipy.linalg as la
import torch

import factorisation_reference as fr
import grates_amd as ga
from grates_amd import lstsq as ls

pytestmark = pytest.mark.gpu
eng = ga.engine

FACTOR_SWEEPS = ('right', 'recursive', 'lookahead', 'pair')      # doors that return a factor
ALL_SWEEPS = FACTOR_SWEEPS + ('in_place',)
MODE_OF = {'recursive': 'off', 'lookahead': 'on', 'in_place': 'on', 'pair': 'on'}


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order='C', copy=True)).cuda()          # (a copy: the inputs are shared and read-only)


def pivot_in(message):
    """k of "k-th leading minor of the array is not positive definite" """
    assert '-th leading minor' in message, message
    return int(message.split('-th leading minor')[0].split()[-1])


def block_sweep(mats, mode, in_place=False):
    """One-block tables of the matrices `mats` (one: engine.block_potrf, two: engine.block_potrf_pair) under look-ahead `mode`;
    returns [(U, X, flag), ...] as host arrays (in place: U is None).  The inverse buffers start as NaN: every entry is written."""
    n = mats[0].shape[0]
    blocks = [dev(A) for A in mats]
    inverses = blocks if in_place else [torch.full((n, n), float('nan'), dtype=torch.float64, device='cuda') for _ in mats]
    tables = [eng.BlockTable(np.array([0, n]), {(0, 0): b}) for b in blocks]
    pointers = [np.array([x.data_ptr()], dtype=np.uint64) for x in inverses]
    eng.block_set_lookahead(mode)
    try:
        if len(mats) == 1:
            flags = (eng.block_potrf(tables[0], pointers[0]),)
        else:
            flags = eng.block_potrf_pair(tables[0], pointers[0], tables[1], pointers[1])
    finally:
        eng.block_set_lookahead(True)
    return [(None if in_place else b.cpu().numpy(), x.cpu().numpy(), int(f)) for b, x, f in zip(blocks, inverses, flags)]


def companion(A):
    """a different matrix of the same kind for the second slot of a pair: A with rows and columns reversed"""
    return A[::-1, ::-1].copy()


def factor(A, sweep):
    """(U, X, pivot) through one door; X is None where the factorisation failed ('right'), U is None for 'in_place'"""
    if sweep == 'right':
        T = dev(A)
        eng.potrf(T, check=False)
        pivot = 0
        try:
            eng.potrf(dev(A))                                   # the flag, as Python reports it
        except np.linalg.LinAlgError as err:
            pivot = pivot_in(str(err))
        return T.cpu().numpy(), (eng.trtri(T).cpu().numpy() if pivot == 0 else None), pivot
    if sweep == 'pair':
        return block_sweep([A, companion(A)], MODE_OF[sweep])[0]
    return block_sweep([A], MODE_OF[sweep], in_place=sweep == 'in_place')[0]


def lapack_trtri(Uf):
    X, info = la.lapack.dtrtri(np.asfortranarray(Uf), lower=0)
    assert info == 0
    return X


def own_inverse_error(X, Uf):
    return fr.inverse_error(X, Uf, fr.triangular_inverse(Uf))


@functools.lru_cache(maxsize=None)
def lapack_figures(key):
    """(scaled residual of scipy.linalg.cholesky, inverse error of dtrtri on that factor) for the input `key` (see `matrix`)"""
    A = matrix(key)
    Ul = la.cholesky(A, lower=False)
    return fr.scaled_residual(Ul, A), own_inverse_error(lapack_trtri(Ul), Ul)


@functools.lru_cache(maxsize=None)
def matrix(key):
    kind, n = key
    A = fr.spd_spectrum(n, 1e4, n)
    if kind == 'graded':
        A = fr.graded(A, n)[0]
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def result(key, sweep):
    """(U, X, pivot) of one door on one input, once ('pair': the input in the first slot of the pair, 'pair1': in the second)"""
    A = matrix(key)
    if sweep == 'pair1':
        return block_sweep([companion(A), A], 'on')[1]
    return factor(A, sweep)


def check_factor_and_inverse(key, sweep):
    """the bounds of the size test for one door on one input"""
    A, n = matrix(key), key[1]
    Uf, X, pivot = result(key, sweep)
    assert pivot == 0
    if sweep == 'in_place':
        assert np.array_equal(X, result(key, 'lookahead')[1])                # the same bits as with a buffer of its own
        return
    assert np.isfinite(Uf).all() and np.isfinite(X).all()
    assert np.array_equal(np.tril(Uf, -1), np.zeros_like(Uf)) and np.array_equal(np.tril(X, -1), np.zeros_like(X))
    L_res, L_inv = lapack_figures(key)
    res, inv = fr.scaled_residual(Uf, A), own_inverse_error(X, Uf)
    print('{0} {1}: scaled residual {2:.3e} (LAPACK {3:.3e}), inverse error {4:.3e} (LAPACK {5:.3e}), n u = {6:.3e}'.format(
        key, sweep, res, L_res, inv, L_inv, n * fr.U))
    assert res <= 10 * max(L_res, n * fr.U), (sweep, n, res, L_res)
    assert inv <= 10 * max(L_inv, n * fr.U), (sweep, n, inv, L_inv)


# ---- a. sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', fr.SIZES)
@pytest.mark.parametrize('sweep', ALL_SWEEPS + ('pair1',))
def test_sizes(sweep, n):
    check_factor_and_inverse(('plain', n), sweep)


@pytest.mark.parametrize('n', fr.SIZES)
def test_sweeps_agree(n):
    """The factors of all doors agree to 20 n u sqrt(a_jj), entry by entry (|u_ij| <= sqrt(a_jj)).  Their inverses agree as far as that
    allows: factors that differ by dU have inverses that differ by X dU X to first order, at most 20 n u (|X| E |X|)_ij with
    E_kj = sqrt(a_jj) on and above the diagonal, and each door's X lies within 10 max(L, n u) (|X| |U| |X|)_ij of the inverse of its own
    factor (test_sizes), twice that between two doors.  (The two bound matrices are sums of non-negative terms, evaluated in float64
    from the factor and the inverse of the first door.)"""
    key = ('plain', n)
    A = matrix(key)
    doors = FACTOR_SWEEPS + ('pair1',)
    factors = np.stack([result(key, s)[0] for s in doors])
    spread = factors.max(axis=0) - factors.min(axis=0)
    worst = float(np.max(spread / np.sqrt(np.diag(A))[None, :]))
    print('n = {0}: largest spread between the factors of the doors {1:.3e} sqrt(a_jj), bound {2:.3e}'.format(n, worst, 20 * n * fr.U))
    assert worst <= 20 * n * fr.U
    inverses = np.stack([result(key, s)[1] for s in doors + ('in_place',)])
    spread = np.triu(inverses.max(axis=0) - inverses.min(axis=0))
    U0, X0 = np.abs(factors[0]), np.abs(inverses[0])
    E = np.triu(np.ones((n, n))) * np.sqrt(np.diag(A))[None, :]
    bound = 20 * n * fr.U * (X0 @ E @ X0) + 2 * 10 * max(lapack_figures(key)[1], n * fr.U) * (X0 @ U0 @ X0)
    iu = np.triu_indices(n)
    worst = float(np.max(spread[iu] / bound[iu]))
    print('n = {0}: largest spread between the inverses of the doors {1:.3e} of its bound'.format(n, worst))
    assert worst <= 1.0


# ---- b. pivot index -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', fr.PIVOTS)
@pytest.mark.parametrize('sweep', ALL_SWEEPS)
def test_pivot_index(sweep, p):
    assert factor(fr.first_bad_minor(fr.PIVOT_N, p, p), sweep)[2] == p


@pytest.mark.parametrize('p', fr.PIVOTS)
@pytest.mark.parametrize('mode', ['on', 'off'])
def test_pivot_index_of_a_pair(mode, p):
    """one flag per item: (good, bad at p), (bad at p, good), (bad at p, bad at q)"""
    q = fr.PIVOTS[(fr.PIVOTS.index(p) + 4) % len(fr.PIVOTS)]
    good, bad_p, bad_q = (fr.first_bad_minor(fr.PIVOT_N, k, k) for k in (0, p, q))
    for pair, expected in (((good, bad_p), (0, p)), ((bad_p, good), (p, 0)), ((bad_p, bad_q), (p, q))):
        flags = tuple(item[2] for item in block_sweep(list(pair), mode))
        assert flags == expected, (mode, flags, expected)


@pytest.mark.parametrize('sweep', ALL_SWEEPS)
def test_pivot_index_semidefinite(sweep):
    A = fr.semidefinite_rank1(fr.RANK1_N)
    assert factor(A, sweep)[2] == 2
    if sweep == 'pair':
        good = fr.first_bad_minor(fr.RANK1_N, 0, 0)
        for mode in ('on', 'off'):
            assert tuple(item[2] for item in block_sweep([good, A], mode)) == (0, 2)


@pytest.mark.parametrize('site', fr.NAN_SITES)
@pytest.mark.parametrize('sweep', ALL_SWEEPS)
def test_pivot_index_of_a_nan(sweep, site):
    """one NaN at (i, j) of the upper triangle reaches pivot j first (the reference says so: test_semidefinite_and_nan_inputs)"""
    good = fr.reference(fr.PIVOT_N, 1e2, fr.PIVOT_N)[0]
    assert factor(fr.with_nan(good, *site), sweep)[2] == site[1] + 1


def walker_matrix(A):
    """BlockMatrix of the upper triangle of A cut as (300, 130)"""
    cut = np.array(fr.WALKER_CUT)
    return ls.BlockMatrix.from_array(np.triu(A), cut, cut)


def under(mode, call):
    """call() under look-ahead `mode`, the default restored afterwards"""
    eng.block_set_lookahead(mode)
    try:
        return call()
    finally:
        eng.block_set_lookahead(True)


@pytest.mark.parametrize('p', fr.WALKER_PIVOTS)
@pytest.mark.parametrize('mode', ['off', 'plain', 'carry'])
def test_block_walker_pivot_index(mode, p):
    """BlockMatrix.cholesky() over block rows (300, 130): the message carries the index counted over the whole matrix"""
    bm = walker_matrix(fr.first_bad_minor(fr.WALKER_N, p, p))
    with pytest.raises(np.linalg.LinAlgError) as err:
        under(mode, bm.cholesky)
    assert pivot_in(str(err.value)) == p


@pytest.mark.parametrize('q', fr.WALKER_SCHUR_PIVOTS)
@pytest.mark.parametrize('mode', ['off', 'plain', 'carry'])
def test_block_walker_pivot_index_of_a_later_call(mode, q):
    """the first block row factors; the failure is planted in the Schur complement of the second one and found by a call that starts
    there: the index still counts from the start of the matrix, bounds[1] + q"""
    bm = walker_matrix(fr.first_bad_minor(fr.WALKER_N, 0, 0))
    under(mode, lambda: bm._cholesky_rows(0, 1))
    rows = fr.WALKER_CUT[2] - fr.WALKER_CUT[1]
    bm.device_block(1, 1).copy_(dev(fr.first_bad_minor(rows, q, q)))
    with pytest.raises(np.linalg.LinAlgError) as err:
        under(mode, lambda: bm._cholesky_rows(1, 2))
    assert pivot_in(str(err.value)) == fr.WALKER_CUT[1] + q


# ---- c. conditioning ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conditioning_reference(n, kappa, seed):
    A, Uf, X = fr.reference(n, kappa, seed)
    b = np.random.default_rng(seed + 1).standard_normal((n, 3))
    x_ref, Z_ref = fr.solve(Uf, b), X @ X.T
    Ul = la.cholesky(A, lower=False)
    Zl, info = la.lapack.dpotri(Ul, lower=0)
    assert info == 0
    lapack = (fr.forward_error(la.cho_solve((Ul, False), b), x_ref), fr.max_norm_error(Zl, Z_ref), fr.scaled_residual(Ul, A))
    return A, b, x_ref, Z_ref, lapack


CONDITIONING_RUNS = [case + (mode,) for case in fr.CONDITIONING for mode in (('on', 'off') if len(case[3]) == 2 else ('carry', 'plain', 'off'))]


@pytest.mark.parametrize('n,kappa,seed,bounds,mode', CONDITIONING_RUNS)
def test_conditioning(n, kappa, seed, bounds, mode):
    """BlockMatrix.cholesky(), two solve_triangular calls with three right-hand sides and sparse_inverse() (full pattern: the whole
    inverse) on Q diag(lambda) Q^T with condition number kappa, against long double: each figure within 10 times LAPACK's"""
    A, b, x_ref, Z_ref, (L_fwd, L_inv, L_res) = conditioning_reference(n, kappa, seed)
    cut = np.array(bounds)
    bm = ls.BlockMatrix.from_array(np.triu(A), cut, cut)
    under(mode, bm.cholesky)
    res = fr.scaled_residual(bm.to_array(), A)
    x = bm.solve_triangular(bm.solve_triangular(b, transpose=True))
    fwd = fr.forward_error(x, x_ref)
    bm.sparse_inverse()
    inv = fr.max_norm_error(bm.to_array(), Z_ref)
    print('conditioning n = {0} kappa = {1:.0e} cut {2} mode {3}: forward error {4:.3e} = {5:.2f} LAPACK, inverse {6:.3e} = {7:.2f} LAPACK, '
          'scaled residual {8:.3e} = {9:.2f} LAPACK'.format(n, kappa, tuple(int(d) for d in np.diff(cut)), mode, fwd, fwd / L_fwd, inv, inv / L_inv, res, res / L_res))
    assert fwd <= 10 * L_fwd
    assert inv <= 10 * L_inv
    assert res <= 10 * max(L_res, n * fr.U)


# ---- d. grading ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', fr.GRADED_N)
@pytest.mark.parametrize('sweep', ALL_SWEEPS + ('pair1',))
def test_graded(sweep, n):
    """D A D with D = diag(2^e_i), |e_i| <= 40: scaling by powers of two commutes with every operation of these kernels (fma and MFMA
    accumulation, the square root of a value scaled by 4^e, the reciprocal estimate from the mantissa and its Newton steps, the sums
    over K slices) as long as nothing under- or overflows, and the routes depend on the shapes alone: U(D A D) = U(A) D and
    X(D A D) = D^-1 X(A), bit for bit.  And the graded matrix meets the bounds of the size test, which see every entry at its own scale."""
    e = fr.graded(fr.spd_spectrum(n, 1e4, n), n)[1]
    Uf, X, pivot = result(('plain', n), sweep)
    Ug, Xg, pivot_g = result(('graded', n), sweep)
    assert pivot == 0 and pivot_g == 0
    if Uf is not None:
        assert np.array_equal(Ug, np.ldexp(Uf, e[None, :]))
    assert np.array_equal(Xg, np.ldexp(X, -e[:, None]))
    check_factor_and_inverse(('graded', n), sweep)


# ---- e. untouched memory ---------------------------------------------------------------------------------------------------------------
def nan_below(A):
    B = A.copy()
    B[np.tril_indices(A.shape[0], -1)] = np.nan
    return B


@pytest.mark.parametrize('sweep', ALL_SWEEPS)
def test_lower_triangle_is_not_read(sweep):
    """NaN in the whole strictly lower triangle (0 * NaN does not vanish): the same bits as on the clean matrix"""
    A = fr.reference(fr.PIVOT_N, 1e2, fr.PIVOT_N)[0]
    clean, dirty = factor(A, sweep), factor(nan_below(A), sweep)
    assert clean[2] == 0 and dirty[2] == 0
    if sweep == 'pair':
        second = block_sweep([nan_below(companion(A)), nan_below(A)], 'on')[1]
        assert np.array_equal(second[0], clean[0]) and np.array_equal(second[1], clean[1])
    if clean[0] is not None:
        assert np.isfinite(dirty[0]).all() and np.array_equal(dirty[0], clean[0])
    assert np.isfinite(dirty[1]).all() and np.array_equal(dirty[1], clean[1])


def test_trtri_does_not_read_the_lower_triangle():
    A = fr.reference(fr.PIVOT_N, 1e2, fr.PIVOT_N)[0]
    Uf = eng.potrf(dev(A)).cpu().numpy()
    clean = eng.trtri(dev(Uf)).cpu().numpy()
    dirty = eng.trtri(dev(nan_below(Uf))).cpu().numpy()
    assert np.isfinite(dirty).all() and np.array_equal(dirty, clean)


def test_views_inside_nan():
    """the matrix as a 300 x 300 view at (23, 17) of a NaN-filled 340 x 352 tensor: potrf (in place) and trtri give the bits of the
    contiguous case, and nothing outside the view is written"""
    n, r0, c0 = fr.PIVOT_N, 23, 17
    A = fr.reference(n, 1e2, n)[0]
    U_ref = eng.potrf(dev(A))
    X_ref = eng.trtri(U_ref)
    big = torch.full((340, 352), float('nan'), dtype=torch.float64, device='cuda')
    view = big[r0:r0 + n, c0:c0 + n]
    view.copy_(dev(nan_below(A)))
    outside = torch.ones((340, 352), dtype=torch.bool, device='cuda')
    outside[r0:r0 + n, c0:c0 + n] = False
    eng.potrf(view)
    assert bool(torch.isfinite(view).all()) and torch.equal(view, U_ref)
    assert bool(torch.isnan(big[outside]).all())
    view.copy_(dev(nan_below(U_ref.cpu().numpy())))
    X = eng.trtri(view)
    assert bool(torch.isfinite(X).all()) and torch.equal(X, X_ref)
    assert bool(torch.isnan(big[outside]).all())
