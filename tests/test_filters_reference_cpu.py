"""
The references of tests/filters_reference.py and the dispatch query engine.orderwise_filter_info, without a GPU.

    orderwise_reference   against orc.orderwise_filter epoch by epoch (NumPy's float64 products are one more correct evaluation: within E)
                          and against the reference's own outputs (g10_filter) at that file's 1e-13
    order_major_rows      a bijection, and the map engine.order_major_first_row gives
    poisoned_blocks       the leading corners are the plain blocks, everything else is the poison, the oracle never reads it
    orderwise_filter_info the seams of the dispatch of shg_orderwise_filter (csrc/filters.hip: orderwise_group, orderwise_via_series)
    solve_residual        of the host solutions on the inputs of the GPU solver tests: under the bound d gamma(3 d + 1)

Measured here (printed before each assertion, pytest -s): orc.orderwise_filter against the reference at most 0.31 E; np.linalg.solve on the
spd_solve inputs 0.16 (n = 1) ... 2e-6 (n = 165) of the bound, on the DDK blocks at most 0.17 of it (the smallest blocks).  np.linalg.solve
against scipy's cho_solve on the DDK blocks (max |difference| / max |block|, per block): 0 ... 8.5e-16 at degrees 0 ... 120 -- conditioning
does not lift the floor of the device comparison at 1e-12.
"""

import os
import re

import numpy as np
import pytest

import grates_amd as ga
import filters_reference as fr
import inputs
from conftest import ROOT, relerr
from oracle import shg_oracle as orc


@pytest.mark.parametrize('N', [0, 1, 2, 17, 33])
@pytest.mark.parametrize('poisoned', [False, True])
def test_orderwise_reference_against_oracle(N, poisoned):
    Nb, B = 33, 5
    blocks = fr.poisoned_blocks(42, Nb, N) if poisoned else fr.random_blocks(42, Nb)
    batch = fr.coefficient_batch(100, N, B)
    ref, E = fr.orderwise_reference(blocks, batch)
    assert ref.shape == E.shape == batch.shape and ref.dtype == E.dtype == np.longdouble
    worst = max(fr.worst_ratio(orc.orderwise_filter(batch[e], blocks), ref[e], E[e]) for e in range(B))
    print('d/o {0} of {1}{2}: oracle against the reference {3:.3f} E'.format(N, Nb, ' poisoned' if poisoned else '', worst))
    assert worst <= 1.0
    assert np.array_equal(ref[:, 0:2, 0:2], batch[:, 0:2, 0:2]) and not E[:, 0:2, 0:2].any()
    if N >= 2:
        rest = np.ones((N + 1, N + 1), dtype=bool)
        rest[0:2, 0:2] = False
        assert np.all(E[:, rest] > 0) and float(np.max(E)) < 1e-24          # the bound is there, and far below one misplaced term (1e-12)


def test_orderwise_reference_against_golden(golden):
    g = golden('g10_filter')
    for nmax, ngf in ((20, 20), (120, 96)):
        ref, _ = fr.orderwise_reference(inputs.orderwise_random_blocks(42, nmax), inputs.coefficients(43, ngf)[np.newaxis])
        err = relerr(ref[0], g['orderwise_{0}_{1}'.format(nmax, ngf)])
        print('orderwise_{0}_{1}: reference against golden {2:.2e}'.format(nmax, ngf, err))
        assert err < 1e-13


def test_worst_ratio_sees_one_wrong_entry():
    blocks, batch = fr.random_blocks(42, 33), fr.coefficient_batch(100, 17, 3)
    ref, E = fr.orderwise_reference(blocks, batch)
    good = ref.astype(np.float64)
    assert fr.worst_ratio(good, ref, E) <= 1.0
    bad = good.copy()
    bad[2, 9, 4] *= 1 + 1e-12
    assert fr.worst_ratio(bad, ref, E) > 1.0
    bad = good.copy()
    bad[1, 1, 0] = np.nextafter(bad[1, 1, 0], 1.0)                          # degrees 0 and 1: exact or nothing
    assert fr.worst_ratio(bad, ref, E) == float('inf')


@pytest.mark.parametrize('N', range(41))
def test_order_major_rows(N):
    rows = fr.order_major_rows(N)
    assert rows.shape == (N + 1, N + 1) and np.array_equal(np.sort(rows.ravel()), np.arange((N + 1) ** 2))
    for s in range(2 * N + 1):
        m = (s + 1) >> 1
        first = ga.engine.order_major_first_row(N, s)
        for n in range(m, N + 1):
            r, c = (n, m) if (s == 0 or s & 1) else (m - 1, n)
            assert rows[r, c] == first + n - m, (N, s, n)


def test_poisoned_blocks():
    plain = inputs.orderwise_random_blocks(42, 12)
    bad = fr.poisoned_blocks(42, 12, 7)
    assert len(bad) == len(plain) == 25
    for s, (p, b) in enumerate(zip(plain, bad)):
        n = max(7 + 1 - ((s + 1) >> 1), 0)
        mask = np.zeros(p.shape, dtype=bool)
        mask[:n, :n] = True
        assert b.shape == p.shape and np.array_equal(b[mask], p[mask]) and np.all(b[~mask] == 1e30)
    assert any(np.all(b == 1e30) for b in bad)                               # the blocks of the orders beyond the field
    x = inputs.coefficients(5, 7)
    assert np.array_equal(orc.orderwise_filter(x, bad), orc.orderwise_filter(x, plain))
    assert all(np.array_equal(a, b) for a, b in zip(fr.poisoned_blocks(42, 12, 12), plain))


def order_major_max_lds():
    text = open(os.path.join(ROOT, 'grates_amd', 'csrc', 'filters.hip')).read()
    m = re.search(r'constexpr size_t kOrderMajorMaxLds = (\d+) \* (\d+);', text)
    assert m and 'return (size_t)16 * (N + 2) * sizeof(double);' in text     # order_major_lds_bytes: one row of 16 epochs
    return int(m.group(1)) * int(m.group(2))


def test_orderwise_filter_info_seams():
    info = ga.engine.orderwise_filter_info
    assert sorted(info(20, 5)) == ['epochs_per_workgroup', 'group', 'lds_bytes', 'via_series']
    for N, G in ((0, 8), (143, 8), (144, 4), (295, 4), (296, 2), (599, 2), (600, 0), (5000, 0)):
        got = info(N, 3)
        assert got['group'] == G and got['epochs_per_workgroup'] == 16 and got['via_series'] is False, (N, got)
        assert (got['lds_bytes'] == 0) == (G == 0) and got['lds_bytes'] <= 160 * 1024, (N, got)
        if G:
            # G planes of round_up(N + 1, 8) rows of 17 doubles, padded by less than 16 doubles each
            plane = got['lds_bytes'] // (8 * G)
            rows = -(-(N + 1) // 8) * 8 * 17
            assert got['lds_bytes'] % (8 * G) == 0 and rows <= plane < rows + 16 and plane % 16 == (1 + 16 // G) % 16, (N, got)
    # the next larger group does not fit where the smaller one takes over
    assert info(143, 1)['lds_bytes'] <= 160 * 1024 < 8 * (info(144, 1)['lds_bytes'] // 4)
    assert info(295, 1)['lds_bytes'] <= 160 * 1024 < 4 * (info(296, 1)['lds_bytes'] // 2)
    for N in (0, 40, 143, 144, 296, 520):
        assert info(N, 63)['via_series'] is False and info(N, 64)['via_series'] is True and info(N, 1000)['via_series'] is True, N
        assert info(N, 63)['group'] == info(N, 64)['group']                  # G does not depend on the epochs
    last = order_major_max_lds() // 128 - 2                                  # the last degree whose row stage (16 epochs x (N + 2) doubles) fits
    assert info(last, 64)['via_series'] is True and info(last + 1, 64)['via_series'] is False
    assert info(last + 1, 10 ** 6)['via_series'] is False
    assert info(3, 0) == {'via_series': False, 'group': 8, 'lds_bytes': info(3, 1)['lds_bytes'], 'epochs_per_workgroup': 16}
    with pytest.raises(ga._lib.ShgError):
        info(-1, 3)
    with pytest.raises(ga._lib.ShgError):
        info(3, -1)


def test_refusal_message_names_the_last_degree():
    """The texts that state the last degree of the block kernel agree with the query."""
    info = ga.engine.orderwise_filter_info
    last = max(N for N in range(500, 700) if info(N, 1)['group'])
    assert info(last + 1, 1)['group'] == 0
    text = open(os.path.join(ROOT, 'grates_amd', 'csrc', 'filters.hip')).read()
    assert '(max degree {0})'.format(last) in text and '2: <= {0})'.format(last) in text
    doc = open(os.path.join(ROOT, 'tests', 'test_gpu_filters.py')).read()
    assert 'up to {0} (beyond that the kernel refuses)'.format(last) in ' '.join(doc.split())


@pytest.mark.parametrize('n,k', fr.SPD_CASES)
def test_solve_residual_of_host_solution_spd(n, k):
    A, B = fr.spd_case(n, k)
    assert np.array_equal(A, A.T) and np.linalg.eigvalsh(A)[0] >= 1.0 - 1e-12
    X = np.linalg.solve(A, B)
    bound = fr.solve_bound(n)
    for c0 in range(0, k, 256):
        res = fr.solve_residual(A, X[:, c0:c0 + 256], B[:, c0:c0 + 256])
        print('n = {0}, columns {1} ..: residual {2:.2e}, bound {3:.2e}'.format(n, c0, res, bound))
        assert res <= bound
    wrong = X.copy()
    assert float(np.max(fr.solve_residual_columns(A, X, B))) <= bound
    wrong = X.copy()
    wrong[n // 2, k - 1] *= 1 + 1e-6                                         # one entry of the last column off in the sixth digit
    assert fr.solve_residual(A, wrong[:, 256 * ((k - 1) // 256):], B[:, 256 * ((k - 1) // 256):]) > bound
    assert fr.solve_residual_columns(A, wrong, B)[k - 1] > bound and np.all(fr.solve_residual_columns(A, wrong, B)[:k - 1] <= bound)


@pytest.mark.parametrize('Nb', fr.DDK_DEGREES)
def test_solve_residual_of_host_solution_ddk(Nb):
    import scipy.linalg
    normals, w = fr.ddk_case(Nb)
    assert w[0] == 1 and np.array_equal(w[1:], orc.DDK_SCALE[5] * np.arange(1, Nb + 1, dtype=float) ** 4)
    blocks = orc.ddk_blocks(normals, 5)
    worst, spread = 0.0, 0.0
    for s, (Nk, W) in enumerate(zip(normals, blocks)):
        m = (s + 1) >> 1
        A = Nk + np.diag(w[m:])
        res, bound = fr.solve_residual(A, W, Nk), fr.solve_bound(Nb + 1 - m)
        assert res <= bound, (Nb, s, res, bound)
        worst = max(worst, res / bound)
        spread = max(spread, relerr(scipy.linalg.cho_solve(scipy.linalg.cho_factor(A), Nk), W))
    print('DDK5 blocks of d/o {0}: worst residual / bound {1:.2e}; solve against cho_solve {2:.2e}'.format(Nb, worst, spread))
    assert spread <= 1e-13                                                   # two host solutions agree: 1e-12 is a fair floor for the device
