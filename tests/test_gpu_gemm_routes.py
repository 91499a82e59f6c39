"""
Every route of the dense fp64 product dispatcher on the device, case by case from tests/gemm_route_cases.py, through
shg_gemm_ex (and through shg_gemm where the case is a plain product).  A case first asserts its route on the actual device
pointers (engine.gemm_route), then:

  exact          A, B, C0 hold small integers, alpha and beta come from {0, +-1, +-2, +-0.5} (C0 even for +-0.5).  The host first
                 checks |alpha| (|A| @ |B|) + |beta| |C0| < 2^53 everywhere; then every summation order, fused or not, split or
                 not, gives the same bits as the float64 host product: assert_array_equal, no tolerance.
  componentwise  real data with a wide range (rows of op(A) scaled by 2^(-40 i / M), columns of op(B) by 2^(+40 j / N)):
                 |got - ref| <= 2 gamma_n E elementwise, E = |alpha| |op A| |op B| + |beta| |C0|, gamma_n = n u / (1 - n u), u = 2^-53,
                 n = K + 20 (K products and sums, up to 16 split-K partials, alpha and beta).  Device result and host reference
                 both obey gamma_n E against the exact value, hence the factor 2.  The bound is derived, not measured.
  poison         beta = 0 on an output full of NaN equals, bit for bit, the result on a zeroed output (which is also the second
                 call of the repeatability check); padding columns (ldc > N) and the rows behind the last one keep their bits,
                 NaN and finite; the padding of the operands holds NaN throughout.
  structure      the zero side of a triangular operand holds NaN; the result equals the one for explicit zeros bit for bit.  With
                 upper_only the upper triangle is checked and every 128 x 128 block wholly below the diagonal keeps its poison.
  batch          integer data: every item equals the single-item call on its slice, bit for bit.
  in place       integer data: the supported forms (C is B, C is A) equal the out-of-place result bit for bit; real data: the bound.
"""
import zlib

import numpy as np
import pytest
import torch

import gemm_route_cases as rc
import grates_amd as ga

pytestmark = pytest.mark.gpu
eng = ga.engine

U = 2.0 ** -53
PAIRS = [(-1.0, 1.0), (2.0, -2.0), (0.5, 0.5), (-0.5, -1.0), (-2.0, 2.0), (1.0, -0.5), (0.0, -2.0), (1.0, 1.0)]
ALPHAS = [1.0, -1.0, 2.0, -0.5, 0.5, -2.0]


class Operands:
    """Host storage of a case -- A [items][rows][lda], B likewise, C [batch][M][ldc] plus two spare rows -- and its device copy."""

    def __init__(self, c, kind, seed):
        self.c, self.L = c, rc.layout(c)
        L, M, N, K, batch = self.L, c['M'], c['N'], c['K'], c['batch']
        rng = np.random.default_rng(seed)
        self.itemsA = 1 if 'A' in c['repeat'] else batch
        self.itemsB = 1 if 'B' in c['repeat'] else batch

        def values(items, rows, cols, row_scale=None, col_scale=None):
            if kind == 'int':
                return rng.integers(-3, 4, size=(items, rows, cols)).astype(np.float64)
            v = rng.standard_normal((items, rows, cols))
            if row_scale is not None:
                v *= row_scale[None, :, None]
            if col_scale is not None:
                v *= col_scale[None, None, :]
            return v

        down = 2.0 ** (-40.0 * np.arange(M) / max(M, 1))          # rows of op(A)
        up = 2.0 ** (40.0 * np.arange(N) / max(N, 1))             # columns of op(B)
        self.A = np.full((self.itemsA, L['rowsA'], L['lda']), np.nan)
        self.A[:, :, :L['colsA']] = values(self.itemsA, L['rowsA'], L['colsA'], *((None, down) if c['ta'] else (down, None)))
        self.B = np.full((self.itemsB, L['rowsB'], L['ldb']), np.nan)
        self.B[:, :, :L['colsB']] = values(self.itemsB, L['rowsB'], L['colsB'], *((up, None) if c['tb'] else (None, up)))
        self.C0 = values(batch, M, N, down, up)
        if kind == 'int':
            self.C0 *= 2.0                                          # even: +-0.5 C0 stays an integer

    # ---- what the product means -------------------------------------------------------------------------------------------------
    def op(self, which, zero_side=0.0):
        """op(A) or op(B) [items][rows][cols] with the zero side of a triangular operand set to `zero_side`"""
        c, L = self.c, self.L
        X = self.A[:, :, :L['colsA']] if which == 'A' else self.B[:, :, :L['colsB']]
        X = X.transpose(0, 2, 1) if c['ta' if which == 'A' else 'tb'] else X
        upper, lower = (rc.A_UPPER, rc.A_LOWER) if which == 'A' else (rc.B_UPPER, rc.B_LOWER)
        if c['flags'] & (upper | lower):
            n = X.shape[1]
            keep = np.triu(np.ones((n, n), bool)) if c['flags'] & upper else np.tril(np.ones((n, n), bool))
            X = np.where(keep[None], X, zero_side)
        return X

    def poison_zero_sides(self):
        """NaN on the zero side of the triangular operands, in the stored arrays"""
        c, L = self.c, self.L
        for which, X, cols, t in (('A', self.A, L['colsA'], c['ta']), ('B', self.B, L['colsB'], c['tb'])):
            P = self.op(which, np.nan)
            X[:, :, :cols] = P.transpose(0, 2, 1) if t else P

    def reference(self, alpha, beta, C0):
        """(ref, E) [batch][M][N]: the float64 host product and the magnitude sum of the componentwise bound"""
        A, B = self.op('A'), self.op('B')
        if self.c['K'] == 0:
            prod, mag = np.zeros_like(C0), np.zeros_like(C0)
        else:
            prod, mag = np.matmul(A, B), np.matmul(np.abs(A), np.abs(B))
        prod, mag = np.broadcast_to(prod, C0.shape), np.broadcast_to(mag, C0.shape)
        # (beta = 0 means "C is not read", as in BLAS: no 0 * C0 term)
        ref = alpha * prod + (beta * C0 if beta != 0.0 else 0.0)
        return ref, abs(alpha) * mag + abs(beta) * np.abs(C0)

    # ---- running it ---------------------------------------------------------------------------------------------------------------
    def upload(self):
        c, L = self.c, self.L
        slack = c['b_offset']

        def strided(host, items, rows, cols, ld, stride, offset=0):
            flat = torch.full((host.size + items * offset + 8,), float('nan'), dtype=torch.float64, device='cuda')
            item = rows * ld + offset
            view = torch.as_strided(flat, (items, rows, cols), (item, ld, 1), offset)
            view.copy_(torch.from_numpy(np.ascontiguousarray(host[:, :, :cols])).cuda())
            return (view if items > 1 else view[0]), torch.as_strided(flat, (items, rows, ld), (item, ld, 1), offset)

        self.dA, self.storageA = strided(self.A, self.itemsA, L['rowsA'], L['colsA'], L['lda'], L['strideA'])
        self.dB, self.storageB = strided(self.B, self.itemsB, L['rowsB'], L['colsB'], L['ldb'], L['strideB'], slack)

    def run(self, alpha, beta, prefill, door='ex', inplace=None, item=None):
        """One product on the device; returns the whole output storage [batch][M + 2][ldc] and what it held before the call.
        prefill: the M x N part of the output before the call (ignored in place); item: that item alone, as a product of its own."""
        c, L = self.c, self.L
        inplace = c['inplace'] if inplace is None else inplace
        M, N, batch = c['M'], c['N'], c['batch']
        if c['inplace']:
            self.upload()                                          # an operand is overwritten: a fresh copy per call
        A, B = self.dA, self.dB
        if inplace:
            out = A if inplace == 'A' else B
            storage, before = None, None
        else:
            ldc = L['ldc']
            before = np.empty((batch, M + 2, ldc))
            before[:] = np.where((np.arange(ldc)[None, :] + np.arange(M + 2)[:, None]) % 2 == 0, np.nan, 7.5)[None]      # padding: NaN and finite
            before[:, :M, :N] = prefill
            storage = torch.from_numpy(before).cuda()
            out = storage[:, :M, :N] if batch > 1 else storage[0, :M, :N]
        if item is not None:
            A = A[item] if A.dim() == 3 else A
            B = B[item] if B.dim() == 3 else B
            out = out[item]
        if item is None and inplace == c['inplace']:
            args = eng.gemm_ex_args(A, B, out, c['ta'], c['tb'])
            got = eng.gemm_route(*args, flags=c['flags'])
            assert got == c['expect'], 'case {0} takes route {1} on the device pointers, the table expects {2}'.format(c['name'], got, c['expect'])
        if door == 'gemm':
            eng.gemm(A, B, transa=c['ta'], transb=c['tb'], alpha=alpha, beta=beta, out=out)
        else:
            eng.gemm_ex(A, B, out, c['ta'], c['tb'], alpha, beta, c['flags'])
        torch.cuda.synchronize()
        if inplace:
            return (self.storageA if inplace == 'A' else self.storageB).cpu().numpy(), None         # with the padding columns
        return storage.cpu().numpy(), before


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def wanted(c):
    """mask [M][N] of the entries a call promises: all of them, or the upper triangle"""
    M, N = c['M'], c['N']
    return np.triu(np.ones((M, N), bool)) if c['flags'] & rc.UPPER_ONLY else np.ones((M, N), bool)


def check_untouched(c, got, before):
    """padding columns, the rows behind the last one and, with upper_only, the 128-blocks below the diagonal keep their bits"""
    M, N = c['M'], c['N']
    keep = np.ones(got.shape[1:], bool)
    keep[:M, :N] = False
    if c['flags'] & rc.UPPER_ONLY:
        blocks = np.arange(M)[:, None] // 128 > np.arange(N)[None, :] // 128
        assert blocks.any() or M <= 128
        keep[:M, :N] = blocks
    assert np.array_equal(bits(got)[:, keep], bits(before)[:, keep]), 'case {0}: bits outside the output changed'.format(c['name'])


@pytest.mark.parametrize('name', list(rc.CASES))
def test_route_case(name):
    c = rc.CASES[name]
    M, N, K, batch = c['M'], c['N'], c['K'], c['batch']
    seed = zlib.crc32(name.encode())
    alpha0 = ALPHAS[seed % len(ALPHAS)]
    alpha1, beta1 = PAIRS[(seed // 7) % len(PAIRS)]
    mask = wanted(c)

    # ---- exact: integers ---------------------------------------------------------------------------------------------------------
    ops = Operands(c, 'int', seed)
    ops.poison_zero_sides()
    ops.upload()
    C0 = ops.op('B') if c['inplace'] == 'B' else ops.op('A') if c['inplace'] == 'A' else ops.C0
    C0 = np.broadcast_to(C0, (batch, M, N))
    for alpha, beta in ((alpha0, 0.0), (alpha1, beta1)):
        ref, E = ops.reference(alpha, beta, C0)
        assert E.size == 0 or E.max() < 2.0 ** 53 / 1024, 'the integer data of case {0} could round'.format(name)
        prefill = np.full((batch, M, N), np.nan) if beta == 0.0 else C0
        got, before = ops.run(alpha, beta, prefill)
        np.testing.assert_array_equal(got[:, :M, :N][:, mask], ref[:, mask], err_msg='case {0}, alpha {1}, beta {2}'.format(name, alpha, beta))
        if before is not None:
            check_untouched(c, got, before)
        if c['inplace']:                                                                # against the out-of-place product, bit for bit
            apart, _ = ops.run(alpha, beta, C0, inplace='')
            assert np.array_equal(bits(got[:, :M, :N]), bits(apart[:, :M, :N])), 'case {0}: in place differs from out of place'.format(name)
            pad = np.ones(got.shape[1:], bool)
            pad[:M, :N] = False
            assert np.isnan(got[:, pad]).all(), 'case {0}: the padding of the overwritten operand changed'.format(name)
        if batch > 1 and not c['inplace']:                                              # every item as a product of its own
            for i in range(batch):
                alone, _ = ops.run(alpha, beta, prefill, item=i)
                assert np.array_equal(bits(alone[i, :M, :N][mask]), bits(got[i, :M, :N][mask])), 'case {0}: item {1} alone differs'.format(name, i)
        if c['door'] == 'both':
            again, before = ops.run(alpha, beta, prefill, door='gemm')
            np.testing.assert_array_equal(again[:, :M, :N], ref, err_msg='case {0} through shg_gemm'.format(name))
            check_untouched(c, again, before)
    del ops

    # ---- real data with a wide range: componentwise bound, poison, structure, repeatability ----------------------------------------
    ops = Operands(c, 'real', seed + 1)
    ops.poison_zero_sides()
    ops.upload()
    C0 = ops.op('B') if c['inplace'] == 'B' else ops.op('A') if c['inplace'] == 'A' else ops.C0
    C0 = np.broadcast_to(C0, (batch, M, N))
    n = K + 20
    gamma = n * U / (1.0 - n * U)
    results = {}
    for alpha, beta in ((alpha0, 0.0), (alpha1, beta1)):
        ref, E = ops.reference(alpha, beta, C0)
        prefill = np.full((batch, M, N), np.nan) if beta == 0.0 else C0
        got, before = ops.run(alpha, beta, prefill)
        results[beta] = got
        err = np.abs(got[:, :M, :N] - ref)
        bad = ~(err <= 2.0 * gamma * E) & mask[None]
        if bad.any():
            worst = np.nanmax(np.where(bad, err / np.where(E > 0, E, 1.0), 0.0))
            print('case {0}: {1} entries beyond 2 gamma E, worst |got - ref| / E = {2:.3e} (2 gamma = {3:.3e})'.format(name, int(bad.sum()), worst, 2 * gamma))
        assert not bad.any(), 'case {0}, alpha {1}, beta {2}: componentwise bound missed'.format(name, alpha, beta)
        if before is not None:
            check_untouched(c, got, before)
    # the same call again: on a zeroed output (poison + repeatability), and with explicit zeros on the zero sides (structure)
    first = results[0.0][:, :M, :N][:, mask]
    if not c['inplace']:
        again, _ = ops.run(alpha0, 0.0, np.zeros((batch, M, N)))
    else:
        again, _ = ops.run(alpha0, 0.0, None)
    assert np.array_equal(bits(again[:, :M, :N][:, mask]), bits(first)), 'case {0}: a second call gives other bits'.format(name)
    if c['flags'] & 15:
        L = ops.L
        for which, X, cols, t in (('A', ops.A, L['colsA'], c['ta']), ('B', ops.B, L['colsB'], c['tb'])):
            P = ops.op(which, 0.0)
            X[:, :, :cols] = P.transpose(0, 2, 1) if t else P
        ops.upload()
        zeros, _ = ops.run(alpha0, 0.0, np.full((batch, M, N), np.nan))
        assert np.array_equal(bits(zeros[:, :M, :N][:, mask]), bits(first)), 'case {0}: NaN on the zero side changes the result'.format(name)


# ---- the other doors to a dense product: the exact and the poison check at the shapes their own tests use ------------------------
def _ints(rng, *shape):
    return rng.integers(-3, 4, size=shape).astype(np.float64)


def _poisoned(rows, cols, ld):
    """[rows + 1][ld] of NaN and finite values in turn: the output of a call before it runs"""
    host = np.where((np.arange(ld)[None, :] + np.arange(rows + 1)[:, None]) % 2 == 0, np.nan, -3.25)
    return host, torch.from_numpy(host).cuda()


def _check(got, before, rows, cols, ref, what):
    np.testing.assert_array_equal(got[:rows, :cols], ref, err_msg=what)
    keep = np.ones(got.shape, bool)
    keep[:rows, :cols] = False
    assert np.array_equal(bits(got)[keep], bits(before)[keep]), what + ': bits outside the output changed'


@pytest.mark.parametrize('M,N,K', [(1, 1, 1), (16, 16, 4), (128, 128, 16), (130, 70, 33), (257, 129, 100), (64, 300, 7), (500, 3, 511), (2570, 2700, 515)])
def test_dgemm_exact_and_poison(M, N, K):
    from grates_amd import _lib
    rng = np.random.default_rng(M + N + K)
    A, B = _ints(rng, M, K), _ints(rng, K, N)
    assert (np.abs(A) @ np.abs(B)).max() < 2.0 ** 43
    before, out = _poisoned(M, N, N + 3)
    dA, dB = eng.to_device(A), eng.to_device(B)
    _lib.call('shg_dgemm', M, N, K, eng._ptr(dA), K, eng._ptr(dB), N, eng._ptr(out), N + 3, eng._stream())
    _check(out.cpu().numpy(), before, M, N, A @ B, 'shg_dgemm {0} x {1} x {2}'.format(M, N, K))


@pytest.mark.parametrize('P,T', [(437, 1), (437, 5), (437, 37), (437, 240), (2300, 240)])
def test_dense_filter_exact_and_poison(P, T):
    """P = 437: degrees 2 .. 20, the filter matrices of test_gpu_filters.py; 2300 x 240 takes the tall kernel"""
    from grates_amd import _lib
    rng = np.random.default_rng(P + T)
    W, X = _ints(rng, P, P), _ints(rng, P, T)
    assert (np.abs(W) @ np.abs(X)).max() < 2.0 ** 43
    before, out = _poisoned(P, T, T)                               # Y [P][T] is contiguous: the row behind the last one is the padding
    dW, dX = eng.to_device(W), eng.to_device(X)
    _lib.call('shg_dense_filter', eng._ptr(dW), P, eng._ptr(dX), T, eng._ptr(out), eng._stream())
    _check(out.cpu().numpy(), before, P, T, W @ X, 'shg_dense_filter {0} x {1}'.format(P, T))


@pytest.mark.parametrize('n,k', [(1, 1), (5, 9), (130, 67), (257, 300)])
def test_congruence_exact_and_poison(n, k):
    from grates_amd import _lib
    rng = np.random.default_rng(3 + n + k)
    W, S = _ints(rng, n, k), _ints(rng, k, k)
    S = S + S.T
    ref = W @ S @ W.T
    assert (np.abs(W) @ np.abs(S) @ np.abs(W.T)).max() < 2.0 ** 43
    before, out = _poisoned(n, n, n + 2)
    dW, dS = eng.to_device(W), eng.to_device(S)
    work = torch.full((n, k), float('nan'), dtype=torch.float64, device='cuda')
    _lib.call('shg_congruence', n, k, eng._ptr(dW), k, eng._ptr(dS), k, eng._ptr(out), n + 2, eng._ptr(work), eng._stream())
    _check(out.cpu().numpy(), before, n, n, ref, 'shg_congruence {0} x {1}'.format(n, k))


@pytest.mark.parametrize('B,n', [(1, 100), (5, 441), (17, 1000), (40, 2601), (64, 9409)])
def test_basin_covariance_exact_and_poison(B, n):
    """The strictly lower triangle of S holds NaN: include/shg.h promises that it is never loaded.  (n = 9409: degree 96, 64 masks.)"""
    from grates_amd import _lib
    rng = np.random.default_rng(B + n)
    F, S = _ints(rng, B, n), np.triu(_ints(rng, n, n))
    full = S + np.triu(S, 1).T
    ref = F @ full @ F.T
    assert (np.abs(F) @ np.abs(full) @ np.abs(F.T)).max() < 2.0 ** 43
    S[np.tril(np.ones((n, n), bool), -1)] = np.nan
    before, out = _poisoned(B, B, B)
    dF, dS = eng.to_device(F), eng.to_device(S)
    _lib.call('shg_basin_covariance', B, n, eng._ptr(dF), n, eng._ptr(dS), n, eng._ptr(out), eng._stream())
    _check(out.cpu().numpy(), before, B, B, ref, 'shg_basin_covariance {0} x {1}'.format(B, n))
