"""
The long-double analysis reference (tests/analysis_reference.py) against the oracle's design-matrix least squares, without a GPU,
on every grid of tests/test_gpu_analysis_branches.py: one epoch, the orders [0, 1, 2, 3, N/2, N-1, N] that the oracle can afford
at d/o 128.  The two are independent restatements (separable sums in long double with a refined solve / the full design matrix of
an order in float64), so their agreement pins the reference, and their difference is the spread of a correct float64 analysis.

Measured (max |difference| over the sampled orders / max |oracle|, printed before it is asserted, pytest -s): 1.0e-15 ... 2.4e-14
over all grids, the largest at d/o 128 on 130 x 260 with varying weights (1.6e-14 at d/o 126 on 128 x 256).  The bound asserted
here, 1e-13, is comfortably above that and a decade below the 1e-12 the device is held to.
"""

import numpy as np
import pytest

import analysis_reference as ar
from oracle import shg_oracle as orc

BOUND = 1e-13
CASES = ar.SEAM_CASES + ar.BATCH_CASES + ar.DENSE_CASES


@pytest.mark.parametrize('nlon', [28, 44, 68, 132, 196, 256, 260])
def test_mirrored_meridians(nlon):
    lon = ar.mirrored_meridians(nlon)
    assert lon.shape == (nlon,) and np.all(np.diff(lon) > 0) and lon[0] > -np.pi and lon[-1] < np.pi
    assert np.max(np.abs(lon - ar.plain_meridians(nlon))) < 1e-15                       # the cell-centred equi-angular raster
    j = np.arange(nlon // 4)
    # the three identities of the plan's has_fourfold_symmetry, in its order of evaluation: exactly 0
    assert np.all(lon[nlon - 1 - j] + lon[j] == 0.0)
    assert np.all(lon[nlon // 2 - 1 - j] + np.pi + lon[j] == 0.0)
    assert np.all(lon[nlon // 2 + j] - np.pi - lon[j] == 0.0)


def test_parallels_and_weights():
    for nlat in (16, 17, 67, 130):
        lat = ar.parallels(nlat)
        assert np.all(np.diff(lat) < 0) and abs(lat[0] - (0.5 * np.pi - 0.5 * np.pi / nlat)) < 1e-15
        assert np.max(np.abs(lat + lat[::-1])) < 1e-15
    const, varying = ar.weights('const', 16, 28, 3), ar.weights('varying', 16, 28, 3)
    assert np.all(const == const[:, :1]) and np.all(const > 0)
    assert np.all((varying >= 0.5 * const) & (varying <= 1.5 * const)) and not np.any(np.all(varying == varying[:, :1], axis=1))
    assert np.max(np.abs(varying - varying[::-1])) > 0.1 * const.max()                 # no north-south mirror symmetry
    assert np.array_equal(varying, ar.weights('varying', 16, 28, 3))


def test_cases_cover_the_seams():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        lo, hi = ar.TRANSFORM_DEGREES[c.transform]
        assert lo <= c.N <= hi and c.nlon > 2 * c.N and c.nlat > c.N - c.nmin, c.id
        assert (c.nlon % 4 == 0 and c.shift == 0.0) == c.fourfold, c.id
        # B = 3: the 64-row blocks of the transform straddle epochs and end in a partial block -- except on 128 parallels (d/o 126,
        # the grid without any tail: 3 * 128 rows are six full blocks, each of them inside one epoch)
        assert ((3 * c.nlat) % 64 != 0) == (c.nlat != 128), c.id
        direct = c.N + 1 <= 128 and c.nlat % 2 == 0
        assert c.product == ('gemm' if not direct else 'parity' if (c.nlat % 4 == 0 and c.kind == 'const') else 'operator'), c.id
    assert {c.N for c in ar.SEAM_CASES} >= {64, 65, 96, 97, 126, 127, 128}
    assert any((c.nlon // 4) % 2 == 1 and c.fourfold and c.N > 0 for c in ar.SEAM_CASES)                  # odd quarter domain
    assert any(c.nmin == c.N for c in ar.SEAM_CASES)                                                      # slots with one row


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_reference_against_oracle(case):
    N, nmin = case.N, case.nmin
    vals, area = case.values(1), case.area()
    mer, par = case.meridians(), case.parallels()
    got = ar.analysis(vals, area, nmin, N, mer, par)
    assert got.shape == (1, N + 1, N + 1)
    orders = ar.sample_orders(N)
    ref = orc.analysis_regular(vals[0].ravel(), area.ravel(), nmin, N, mer, par, orc.KernelTable('potential'), orders=orders)
    mask = ar.order_mask(N, nmin, orders)
    err = float(np.max(np.abs(got[0] - ref)[mask]) / np.max(np.abs(ref)))
    print('{0}: reference against the oracle on orders {1}: {2:.2e}'.format(case.id, orders, err))
    assert err < BOUND
    if nmin > 0:
        assert not got[0, :nmin, :nmin].any()
    assert np.all(got[0][ar.order_mask(N, nmin, range(N + 1))] != 0.0)                   # every slot is filled


def test_reference_batch_and_single_grid():
    case = ar.BATCH_CASES[1]
    vals, area = case.values(5), case.area()
    mer, par = case.meridians(), case.parallels()
    out = ar.analysis(vals, area, case.nmin, case.N, mer, par)
    for e in (0, 4):
        one = ar.analysis(vals[e], area, case.nmin, case.N, mer, par)[0]                 # (LAPACK may block one right-hand side differently)
        assert float(np.max(np.abs(one - out[e])) / np.max(np.abs(out[e]))) < 1e-15
    full = orc.analysis_regular(vals[3].ravel(), area.ravel(), case.nmin, case.N, mer, par, orc.KernelTable('potential'))
    assert float(np.max(np.abs(out[3] - full)) / np.max(np.abs(full))) < BOUND
