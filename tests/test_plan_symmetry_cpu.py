"""
The case table tests/plan_symmetry_cases.py against the contract of shg_plan_create, without a GPU:
  * the classification of parallels and meridians, written out here in plain Python as a second statement of
    grates_amd/csrc/plan.hip (has_north_south_symmetry, has_fourfold_symmetry) and synthesis_rot.hip (has_rotation_symmetry,
    rot_layout), reproduces every case's `expect`;
  * every flagged case can tell a working own-table pass from a missing one: evaluating the southern rows from the northern rows'
    geometry (what a pass that read the shared table would compute) misses the independent evaluation by more than 50 x TOL, where
    the device result has to meet TOL (tests/test_gpu_plan_symmetry.py);
  * the accepted-and-unflagged boundary keeps the same shortcut below TOL;
  * the table-level oracle functions equal the grid-level ones bit for bit.
"""

import math

import numpy as np
import pytest

import inputs
import plan_symmetry_cases as psc
from conftest import relerr
from oracle import shg_oracle as orc

TOL = 1e-12            # the bound of tests/test_gpu_synthesis.py


def classify_parallels(N, colat, kn):
    """(accepted, set of flagged northern rows): plan.hip:297-328 restated."""
    nlat = len(colat)
    if nlat < 2 or nlat % 2:
        return False, set()
    flagged = set()
    for i in range(nlat // 2):
        mi = nlat - 1 - i
        dtheta = abs(float(colat[i]) + float(colat[mi]) - math.pi)
        if dtheta > 1e-11:
            return False, set()
        bad = dtheta * (N + 1) > 1e-13
        for n in range(N + 1):
            a, b = float(kn[i][n]), float(kn[mi][n])
            d, s = abs(a - b), max(abs(a), abs(b))
            if d > 1e-10 * s:
                return False, set()
            if d > 5e-14 * s:
                bad = True
        if bad:
            flagged.add(i)
    return True, flagged


def classify_fourfold(lon):
    nlon = len(lon)
    if nlon < 4 or nlon % 4:
        return False
    for j in range(nlon // 4):
        if abs(lon[nlon - 1 - j] + lon[j]) > 3e-15 or abs(lon[nlon // 2 - 1 - j] + math.pi + lon[j]) > 3e-15 or \
                abs(lon[nlon // 2 + j] - math.pi - lon[j]) > 3e-15:
            return False
    return True


def classify_rotation(lon, R):
    """every one of the 2 R images s mu_c + 2 pi k / R of the fundamental domain is a grid column, in whole 128-byte lines"""
    nlon = len(lon)
    if nlon < 192 or nlon % (2 * R) or (nlon // R) % 16:
        return False
    lon = np.asarray(lon, dtype=np.longdouble)
    pi = np.longdouble('3.141592653589793238462643383279502884')
    n2, nR, nd = nlon // 2, nlon // R, nlon // (2 * R)
    for c in range(nd):
        mu = lon[n2 + c]
        for k in range(R):
            for j, target in (((n2 + k * nR + c) % nlon, mu + 2 * pi * k / R), ((n2 + k * nR - 1 - c) % nlon, -mu + 2 * pi * k / R)):
                d = lon[j] - target
                d -= 2 * pi * np.round(d / (2 * pi))
                if abs(float(d)) > 3e-15:
                    return False
    return True


def rotation_slots(R, N):
    """panel slots of the rotation-folded kernel: the orders 1 .. N by class min(m mod R, R - m mod R), each class rounded up to 4"""
    count = {}
    for m in range(1, N + 1):
        r = min(m % R, R - m % R)
        count[r] = count.get(r, 0) + 1
    return sum(-(-c // 4) * 4 for c in count.values())


def shortcut_tables(colat, kn):
    """the southern rows from the northern rows' geometry"""
    colat, kn = colat.copy(), kn.copy()
    nlat = colat.size
    for i in range(nlat // 2):
        colat[nlat - 1 - i] = np.pi - colat[i]
        kn[nlat - 1 - i] = kn[i]
    return colat, kn


def shortcut_error(name, epochs=5):
    N, colat, kn, lon, _ = psc.tables(name)
    scolat, skn = shortcut_tables(colat, kn)
    truth = np.stack([orc.synthesis_tables(inputs.coefficients(6000 + e, N), colat, kn, lon) for e in range(epochs)])
    short = np.stack([orc.synthesis_tables(inputs.coefficients(6000 + e, N), scolat, skn, lon) for e in range(epochs)])
    return relerr(short, truth)


@pytest.mark.parametrize('name', list(psc.CASES))
def test_classification_reproduces_expect(name):
    N, colat, kn, lon, expect = psc.tables(name)
    shape = psc.SHAPES[psc.CASES[name]['shape']]
    assert (lon.size, colat.size) == shape[3:5] and kn.shape == (colat.size, N + 1)
    accepted, flagged = classify_parallels(N, colat, kn)
    assert accepted == expect['north_south']
    assert flagged == expect['flagged']
    assert expect['shortcut_visible'] == bool(flagged)
    fourfold = classify_fourfold(lon)
    assert fourfold == expect['fourfold']
    # the rotation count of the plan's own choice and the counts the kernel can run with: meridians and the 160 KiB of LDS
    counts = tuple(R for R in (10, 9, 6, 3) if classify_rotation(lon, R) and 49152 + 1024 * (rotation_slots(R, N) + 1) <= 160 * 1024)
    assert counts == expect['counts'] and expect['rotations'] == (counts[0] if counts else 0)
    # the paths: K slots of the longitude stage against the panels of the two fused kernels
    K = sum(-(-c // 16) * 16 for c in (N // 2 + 1, (N + 1) // 2, N // 2, (N + 1) // 2)) if fourfold else -(-(2 * N + 1) // 4) * 4
    paths = ['auto', 'staged']
    if fourfold and K * 80 * 8 <= 160 * 1024:
        paths.append('fused')
    if fourfold and accepted and K * 48 * 8 <= 160 * 1024:
        paths.append('fused32')
    if counts:
        paths.append('rot')
    assert sorted(paths) == sorted(expect['paths'])
    # the exactly mirrored tables the case was moved from are accepted and shared
    mcolat, mkn = psc.mirrored(name)
    if colat.size % 2 == 0:
        assert classify_parallels(N, mcolat, mkn) == (True, set())


def test_case_table_covers_the_issue():
    """the row patterns, the three kinds of move, the consumers and the boundaries are all there"""
    cases = psc.CASES.values()
    assert {c['rows'] for c in cases if c['move'] == ('colat', 'kn')} >= {'none', 'single', 'first_block', 'last_block', 'blocks_0_3_last', 'every_other', 'all'}
    assert {c['move'] for c in cases if c['move']} == {('colat',), ('kn',), ('colat', 'kn')}
    assert {c['shape'] for c in cases if c['move']} == set(psc.SHAPES) - {'n45_192x45'}
    assert {c['boundary'] for c in cases if c['boundary']} == {'kn_4e-14', 'colat_2e-11', 'kn_entry_2e-10', 'kn_scaled', 'odd'}
    assert {c['meridians'] for c in cases if c['meridians']} == {1e-15, 1e-14}
    for name in psc.ACCEPTED_FLAGGED:                    # ranks that are not contiguous, a ragged last block, a lone row
        nh = psc.SHAPES[psc.CASES[name]['shape']][4] // 2
        rows = psc.row_pattern(psc.CASES[name]['rows'], nh)
        assert rows and all(0 <= i < nh for i in rows)
    blocks = sorted({i >> 3 for i in psc.row_pattern('blocks_0_3_last', 45)})
    assert blocks == [0, 3, 5] and 45 % 8 != 0


@pytest.mark.parametrize('name', psc.ACCEPTED_FLAGGED)
def test_flagged_cases_tell_a_missing_own_table_pass(name):
    """gap between the shortcut and the truth (> 50 x TOL) beside the bound the device has to meet (TOL)"""
    err = shortcut_error(name)
    print('{0}: shortcut error {1:.2e} = {2:.0f} x TOL; device bound {3:.0e}'.format(name, err, err / TOL, TOL))
    assert err > 50 * TOL


@pytest.mark.parametrize('name', psc.UNFLAGGED_BOUNDARY)
def test_unflagged_boundary_keeps_the_shortcut_below_tol(name):
    err = shortcut_error(name)
    print('{0}: shortcut error {1:.2e}'.format(name, err))
    assert 0.0 < err < TOL


@pytest.mark.parametrize('name', psc.REJECTED)
def test_rejected_cases_need_their_own_rows(name):
    """a plan that took a rejected grid for a symmetric one would be far off (kn_scaled, and the odd grid has no pairing at all)"""
    if psc.CASES[name]['boundary'] == 'odd':
        return
    assert shortcut_error(name, epochs=2) > (1e-3 if psc.CASES[name]['boundary'] == 'kn_scaled' else 2 * TOL)


@pytest.mark.parametrize('shape', ['n45_192x90', 'n17_240x18', 'n33_90x36', 'n45_192x45'])
def test_table_level_oracle_equals_grid_level(shape):
    """synthesis_tables / analysis_tables on the natural, unperturbed tables are synthesis_regular / analysis_regular bit for bit"""
    N, dlon, dlat = psc.SHAPES[shape][0:3]
    lon, parallels, area = orc.geographic_grid(dlon, dlat)
    ker = orc.KernelTable('potential')
    colat, _, kn = orc.kn_table(ker, N, parallels, psc.GM, psc.R_EARTH)
    anm = inputs.coefficients(77, N)
    values = orc.synthesis_regular(anm, lon, parallels, ker)
    assert np.array_equal(orc.synthesis_tables(anm, colat, kn, lon), values)
    n = min(N, 12)                                       # the least squares of a low band of the same grid
    colat, _, kn = orc.kn_table(ker, n, parallels, psc.GM, psc.R_EARTH)
    for nmin, orders in ((0, None), (3, (0, 2, n))):
        ref = orc.analysis_regular(values.ravel(), area.ravel(), nmin, n, lon, parallels, ker, orders=orders)
        assert np.array_equal(orc.analysis_tables(values.ravel(), area.ravel(), nmin, n, colat, kn, lon, orders=orders), ref)
        assert np.any(ref != 0.0)
