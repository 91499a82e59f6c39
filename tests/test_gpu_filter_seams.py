"""
Every kernel of csrc/filters.hip at the seams of its dispatch and of its index maps, against the plain references of
tests/filters_reference.py (pinned without a GPU by tests/test_filters_reference_cpu.py).

    orderwise_filter_kernel<8 | 4 | 2>   the kernel on the reference layout (fewer than 64 epochs): every degree 0 .. 40 -- every n0 mod 16, the
                                         T == 1 branch of the unit map, orders beyond N in the last group, N % 8 == 0, group counts that are and
                                         are not multiples of 8 --, the degrees 143 | 144 and 295 | 296 where G changes, dense blocks throughout
    orderwise_filter_om_kernel           every epoch of 1, 2 and 3 slices at degrees 0 .. 40, 63 .. 66 (a second pass of row tiles) and
                                         127 .. 130 (a third pass, 4 and 5 chunks), padding epochs full of 1e300
    both                                 fields of a lower degree than the blocks, with 1e30 in every block entry they must not let through
                                         (the kernels multiply those by staged zeros); the two routes of shg_orderwise_filter agree to the bit
    order_major_kernel<pack | unpack>    the whole row map, zero padding, at epoch counts around the tiles of 16 and 32
    spd_solve_kernel, ddk_blocks_kernel  one, two and three column tiles; block degrees 0 .. 120 (the benchmark's)
    degree_scale_om_kernel               every position of the first scaled degree, a second turn of the grid-stride loop

The order-wise assertion is componentwise, at every coefficient of every epoch: |got - ref| <= E = gamma(n + 2) (|W| |x|), the worst-case
bound of an n-term fp64 dot product in any order of summation (filters_reference.py: derived, not measured), and equality at degrees 0
and 1.  The solvers are held to the Cholesky backward-error bound d gamma(3 d + 1) on the scaled residual, per column tile, per column and
per block.  The route and the G each case is written for are asserted through engine.orderwise_filter_info before the call.  Every figure
is printed before it is asserted (pytest -s).

Measured on the MI355X (worst |got - ref| / E over every coefficient of every epoch of a group of cases; the file takes 13 s, the longest
case 2 s, most of it the long-double reference on the host):
    block kernel, d/o 0 .. 40 x {1, 16, 17, 63} epochs   poisoned blocks of d/o 40: 0.456 at (14, 63); blocks of the degree: 0.445 at (18, 63)
    block kernel at the G seams, 17 epochs               143 (G = 8) 0.310, 144 (4) 0.335, 295 (4) 0.356, 296 (2) 0.359;
                                                         poisoned: 143 of 150 (8) 0.359, 150 of 300 (4) 0.361, 296 of 300 (2) 0.258
    order-major kernel x {1, 33, 65} epochs              d/o 0 .. 40: 0.428 | poisoned 0.461; 63 .. 66: 0.398 | 0.412; 127 .. 130: 0.449 | 0.410
    the two routes, 63 of 64 epochs                      0 coefficients differ at 33 of 40, 144 of 144 and 143 of 150 poisoned: the claim of the source holds
    spd_solve                                            scaled residual per tile 4.6e-17 .. 9.8e-17, worst single column 9.8e-17 (bounds 4.4e-16 .. 9.1e-12)
    ddk_blocks, d/o 0 .. 120                             worst residual / bound 0.10 .. 0.45 (the 1 x 1 .. 3 x 3 blocks come closest), worst block
                                                         against the oracle 1.1e-16 .. 1.6e-15
The layout and degree-scaling tests compare for equality.

Mutation check.  A library whose G = 2 instantiation alone skips one step of the K loop -- the columns 0 .. 7 of every row tile but the first:
entries off the diagonal only, no address changes -- passes all of tests/test_gpu_filters.py (its one G = 2 case has blocks 0.5 I) and fails
here test_block_kernel_group_seams[296_of_296] with |got - ref| / E = 2.8e14 and [296_of_300_poisoned] with 2.7e14; every other case of this
file passes on it with the figures above.  (Dropping a unit of the unit map instead, e.g. j + 1 in its T > 1 branch, leaves an order
unfiltered, which the 0.5 I test does see.)
"""

import numpy as np
import pytest

import grates_amd as ga
import filters_reference as fr
import inputs
from conftest import relerr
from oracle import shg_oracle as orc

pytestmark = pytest.mark.gpu
info = ga.engine.orderwise_filter_info


def filtered_batch(flt, batch):
    return ga.engine.to_host(flt.filter_batch(batch))


def assert_within_bound(label, got, ref, E):
    """componentwise |got - ref| <= E (exact where E == 0: degrees 0 and 1); returns the worst ratio"""
    ratio = fr.worst_ratio(got, ref, E)
    assert ratio <= 1.0, '{0}: worst |got - ref| / E = {1:.3e}'.format(label, ratio)
    return ratio


def test_host_query_before_the_first_tensor():
    """A fresh process that asks for the dispatch first and computes afterwards.  Found by this file: the query loaded libshg before torch
    was imported, libshg bound to another HIP runtime than torch's, and every launch after it failed with 'no ROCm-capable device is
    detected' (_lib.load imports torch first now)."""
    import subprocess
    import sys
    from conftest import ROOT
    code = ('import numpy as np, grates_amd as ga\n'
            'assert ga.engine.orderwise_filter_info(20, 3)["group"] == 8\n'
            'print(ga.engine.to_host(ga.engine.spd_solve(4.0 * np.eye(2), np.ones((2, 1)))).ravel().tolist())\n')      # (L = 2 I: exact)
    done = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip().endswith('[0.25, 0.25]'), done.stdout + done.stderr


# ---- (a) the block kernel on the reference layout ----------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['poisoned_blocks_40', 'blocks_of_the_degree'])
def test_block_kernel_every_degree_to_40(kind):
    """Degrees 0 .. 40 (G = 8) with 1, 16, 17 and 63 epochs: one, exactly one, two and four epoch groups, the last ones ragged."""
    worst, where = 0.0, None
    for N in range(41):
        blocks = fr.poisoned_blocks(42, 40, N) if kind == 'poisoned_blocks_40' else inputs.orderwise_random_blocks(500 + N, N)
        batch = fr.coefficient_batch(1000 + 100 * N, N, 63)
        ref, E = fr.orderwise_reference(blocks, batch)
        flt = ga.filter.OrderWiseFilter(blocks)
        for B in (1, 16, 17, 63):
            route = info(N, B)
            assert route['via_series'] is False and route['group'] == 8, (N, B, route)
            got = filtered_batch(flt, batch[:B])
            ratio = assert_within_bound('d/o {0}, {1} epochs, {2}'.format(N, B, kind), got, ref[:B], E[:B])
            if ratio > worst:
                worst, where = ratio, (N, B)
    print('block kernel, d/o 0 .. 40, {0}: worst |got - ref| / E = {1:.3f} at (N, B) = {2}'.format(kind, worst, where))


# (Nb, N, B, poisoned, G)
BLOCK_SEAMS = [(143, 143, 17, False, 8), (144, 144, 17, False, 4), (295, 295, 17, False, 4), (296, 296, 17, False, 2),
               (150, 143, 17, True, 8), (300, 150, 17, True, 4), (300, 296, 17, True, 2)]


@pytest.mark.parametrize('Nb,N,B,poisoned,G', BLOCK_SEAMS, ids=['{0}_of_{1}{2}'.format(c[1], c[0], '_poisoned' if c[3] else '') for c in BLOCK_SEAMS])
def test_block_kernel_group_seams(Nb, N, B, poisoned, G):
    """The last degree of G = 8 and of G = 4 and the first of G = 4 and of G = 2, dense blocks; per G one field below the blocks' degree."""
    blocks = fr.poisoned_blocks(77, Nb, N) if poisoned else fr.random_blocks(77, Nb)
    batch = fr.coefficient_batch(2000 + N, N, B)
    route = info(N, B)
    assert route['via_series'] is False and route['group'] == G, route
    got = filtered_batch(ga.filter.OrderWiseFilter(blocks), batch)
    ref, E = fr.orderwise_reference(blocks, batch)
    ratio = assert_within_bound('d/o {0} of {1}'.format(N, Nb), got, ref, E)
    print('block kernel G = {0}, d/o {1} of {2}{3}, {4} epochs: worst |got - ref| / E = {5:.3f}'.format(G, N, Nb, ' poisoned' if poisoned else '', B, ratio))


# ---- (b) the order-major kernel ----------------------------------------------------------------------------------------------------

SERIES_GROUPS = {'0_40': (range(0, 41), 40), '63_66': (range(63, 67), 70), '127_130': (range(127, 131), 135)}


@pytest.mark.parametrize('poisoned', [False, True], ids=['blocks_of_the_degree', 'poisoned_blocks'])
@pytest.mark.parametrize('group', list(SERIES_GROUPS))
def test_order_major_kernel_every_epoch(group, poisoned):
    """1, 33 and 65 epochs (1, 2, 3 slices of 32) with 1e300 in the padding epochs: every epoch compared, the input left as it was."""
    import torch
    degrees, Nb = SERIES_GROUPS[group]
    worst, where = 0.0, None
    for N in degrees:
        blocks = fr.poisoned_blocks(42, Nb, N) if poisoned else inputs.orderwise_random_blocks(500 + N, N)
        batch = fr.coefficient_batch(3000 + 100 * N, N, 65)
        ref, E = fr.orderwise_reference(blocks, batch)
        flt = ga.filter.OrderWiseFilter(blocks)
        for B in (1, 33, 65):
            series = ga.engine.OrderMajorSeries.from_batch(batch[:B])
            assert series.padded_epochs == 32 * (1 + (B - 1) // 32)
            series.data[:, B:] = 1e300
            before = series.data.clone()
            out = flt.filter_series(series)
            assert out is not series and out.max_degree == N and out.epochs == B and out.padded_epochs == series.padded_epochs
            got = ga.engine.to_host(out.to_batch())
            ratio = assert_within_bound('d/o {0} of {1}, {2} epochs'.format(N, Nb if poisoned else N, B), got, ref[:B], E[:B])
            if ratio > worst:
                worst, where = ratio, (N, B)
            assert torch.equal(series.data, before) and bool((series.data[:, B:] == 1e300).all()), (N, B)       # input and its padding untouched
            assert np.array_equal(ga.engine.to_host(series.to_batch()), batch[:B]), (N, B)
    print('order-major kernel, d/o {0}, {1}: worst |got - ref| / E = {2:.3f} at (N, B) = {3}'.format(
        group.replace('_', ' .. '), 'poisoned blocks of d/o {0}'.format(Nb) if poisoned else 'blocks of the degree', worst, where))


# ---- (c) the two routes of shg_orderwise_filter ------------------------------------------------------------------------------------

@pytest.mark.parametrize('Nb,N,poisoned', [(40, 33, False), (144, 144, False), (150, 143, True)], ids=['33_of_40', '144_of_144', '143_of_150_poisoned'])
def test_routes_agree_to_the_bit(Nb, N, poisoned):
    """63 epochs take the kernel on the reference layout, 64 the order-major kernels: the same products in the same order (csrc/filters.hip)."""
    import torch
    blocks = fr.poisoned_blocks(77, Nb, N) if poisoned else fr.random_blocks(77, Nb)
    flt = ga.filter.OrderWiseFilter(blocks)
    x = ga.engine.to_device(fr.coefficient_batch(4000 + N, N, 64))
    assert info(N, 64)['via_series'] is True and info(N, 63)['via_series'] is False and info(N, 63)['group'] == (8 if N <= 143 else 4)
    via_series = flt.filter_batch(x)
    block_kernel = flt.filter_batch(x[0:63])
    series = flt.filter_series(ga.engine.OrderMajorSeries.from_batch(x)).to_batch()
    differing = int((via_series[0:63] != block_kernel).sum())
    print('d/o {0} of {1}: {2} of {3} coefficients differ between the routes'.format(N, Nb, differing, block_kernel.numel()))
    assert torch.equal(via_series[0:63], block_kernel)
    assert torch.equal(via_series[0:63], series[0:63]) and torch.equal(via_series, series)
    assert bool((via_series[:, 2:, :] != x[:, 2:, :]).all())                           # (and they did filter)


# ---- (d) the layout kernels --------------------------------------------------------------------------------------------------------

def test_layout_kernels_whole_map():
    import torch
    for N in range(41):
        rows = fr.order_major_rows(N).ravel()
        for B in (1, 15, 16, 17, 32, 33):
            batch = np.random.default_rng(100 * N + B).standard_normal((B, N + 1, N + 1))
            want = np.empty(((N + 1) ** 2, B))
            want[rows] = batch.reshape(B, -1).T
            x = ga.engine.to_device(batch)
            series = ga.engine.OrderMajorSeries.from_batch(x)
            assert series.data.shape == ((N + 1) ** 2, 32 * (1 + (B - 1) // 32)), (N, B)
            data = ga.engine.to_host(series.data)
            assert np.array_equal(data[:, :B], want), (N, B)
            assert not data[:, B:].any(), (N, B)                                       # pack writes the padding epochs: zero
            assert torch.equal(series.to_batch(), x), (N, B)
            series.data[:, B:] = 1e300
            assert torch.equal(series.to_batch(), x), (N, B)                           # unpack never reads them


# ---- (e) the solvers ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,k', fr.SPD_CASES)
def test_spd_solve_column_tiles(n, k):
    A, B = fr.spd_case(n, k)
    X = ga.engine.to_host(ga.engine.spd_solve(A, B))
    assert X.shape == (n, k)
    bound = fr.solve_bound(n)
    for c0 in range(0, k, 256):                                                        # every tile on its own: a wrong one cannot hide in the norm of another
        res = fr.solve_residual(A, X[:, c0:c0 + 256], B[:, c0:c0 + 256])
        print('spd_solve n = {0}, columns {1} .. {2}: residual {3:.2e} (bound {4:.2e})'.format(n, c0, min(c0 + 256, k) - 1, res, bound))
        assert res <= bound, (n, k, c0)
    cols = fr.solve_residual_columns(A, X, B)
    print('spd_solve n = {0}, k = {1}: worst column {2:.2e}'.format(n, k, float(cols.max())))
    assert np.all(cols <= bound), (n, k, int(np.argmax(cols)))


@pytest.mark.parametrize('Nb', fr.DDK_DEGREES)
def test_ddk_blocks_degrees(Nb):
    """Against orc.ddk_blocks at the 1e-12 of test_ddk_from_synthetic_normals.  np.linalg.solve and scipy's cho_solve agree on these blocks to
    8.5e-16 or better (tests/test_filters_reference_cpu.py): the conditioning does not lift that floor at any of the sizes."""
    normals, w = fr.ddk_case(Nb)
    got = ga.engine.ddk_blocks(normals, w)
    ref = orc.ddk_blocks(normals, 5)
    assert len(got) == 2 * Nb + 1
    worst_res, worst_err = 0.0, 0.0
    for s, (Nk, W, Wref) in enumerate(zip(normals, got, ref)):
        m = (s + 1) >> 1
        A = Nk + np.diag(w[m:])
        bound = fr.solve_bound(Nb + 1 - m)
        res, err = fr.solve_residual(A, W, Nk), relerr(W, Wref)
        worst_res, worst_err = max(worst_res, res / bound), max(worst_err, err)
        assert W.shape == Nk.shape and res <= bound and np.all(fr.solve_residual_columns(A, W, Nk) <= bound), (Nb, s, res, bound)
        assert err < 1e-12, (Nb, s, err)
    print('ddk_blocks d/o {0}: worst residual / bound {1:.2e}, worst block against the oracle {2:.2e}'.format(Nb, worst_res, worst_err))


# ---- (f) degree scaling of a series ------------------------------------------------------------------------------------------------

def test_degree_scale_series_first_degrees():
    for N in (0, 1, 2, 17, 70):
        rows = fr.order_major_rows(N).ravel()
        degree = np.maximum.outer(np.arange(N + 1), np.arange(N + 1))                  # C_nm at [n][m], S_nm at [m-1][n]
        w = 1.0 / (1.0 + np.arange(N + 1))
        for B in (1, 33):
            batch = np.random.default_rng(7 * N + B).standard_normal((B, N + 1, N + 1))
            series = ga.engine.OrderMajorSeries.from_batch(batch)
            for nfirst in sorted({0, 1, 2, N, N + 1}):
                out = ga.engine.degree_scale_series(series, w, nfirst)
                got = ga.engine.to_host(out.data)[:, :B]
                scaled = np.where(degree >= nfirst, batch * w[degree], batch)
                want = np.empty(((N + 1) ** 2, B))
                want[rows] = scaled.reshape(B, -1).T
                assert np.array_equal(got, want), (N, B, nfirst)
                below = rows[(degree < nfirst).ravel()]
                assert np.array_equal(got[below], ga.engine.to_host(series.data)[below, :B]), (N, B, nfirst)    # an exact copy
                assert np.array_equal(ga.engine.to_host(series.to_batch()), batch), (N, B, nfirst)
