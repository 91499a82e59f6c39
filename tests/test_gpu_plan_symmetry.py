"""
Synthesis and analysis on caller-supplied plan tables around the north-south classification of shg_plan_create: the cases of
tests/plan_symmetry_cases.py through engine.Plan(N, colat, kn, lon) itself, against the table-level oracle
(orc.synthesis_tables / orc.analysis_tables: every parallel from its own table row).

Grids whose mirror pairs deviate by an accepted amount get a second table for the mirrored rows of every flagged 8-row block, and
the fused, 32-row and rotation-folded kernels a second pass that reads it.  A pass that read the shared northern table, the wrong
tile or the wrong lane slot would miss the oracle by the case's shortcut error -- more than 50 x TOL for every flagged case
(tests/test_plan_symmetry_cpu.py shows the figure of each case) -- where these tests allow TOL.

Which flagged cases reach the own-table pass of which kernel (shapes of plan_symmetry_cases.SHAPES):
  64-row fused kernel      n45 (all nine flagged cases), n96, n17, n9, n126 (at its slot limit, K = 256)
  32-row fused kernel      the same and n140 (its only fused kernel); blocks_0_3_last moves rows 29 and 30 alone in block 3, one 4-row
                           group of this kernel's own map
  rotation-folded kernel   n45 with 6 and 3 rotations, n96 and n9 with 10, 9, 6 and 3, n17 with 3
  staged kernels           every case, n33 nothing else: they evaluate every row from its own table anyway (the control)

The meridian cases led to one change of the library: has_fourfold_symmetry bounded the sum of two meridians at 2e-15 rad where
has_rotation_symmetry allows 3e-15, so meridians within 1e-15 rad of an equi-angular raster kept the rotation-folded kernel and lost
the 4-fold ones (in 37 of 40 seeded draws); both tests now use 3e-15.
"""

import numpy as np
import pytest

import grates_amd as ga
import inputs
import plan_symmetry_cases as psc
from conftest import relerr
from grates_amd import engine
from oracle import shg_oracle as orc
from test_gpu_synthesis import TOL

pytestmark = pytest.mark.gpu

ShgError = ga._lib.ShgError
EPOCHS = 5
_truth = {}


def coefficients(N, epochs=EPOCHS):
    return np.stack([inputs.coefficients(6000 + e, N) for e in range(epochs)])


def truth(name):
    """synthesis_tables of the case's own tables, EPOCHS epochs"""
    if name not in _truth:
        N, colat, kn, lon, _ = psc.tables(name)
        _truth[name] = np.stack([orc.synthesis_tables(a, colat, kn, lon) for a in coefficients(N)])
    return _truth[name]


def make_plan(name, mirrored=False):
    N, colat, kn, lon, expect = psc.tables(name)
    if mirrored:
        colat, kn = psc.mirrored(name)
    return engine.Plan(N, colat, kn, lon), expect


def meridians_allow(name, R):
    """the meridians of the case are invariant under R rotations in whole 128-byte lines"""
    nlon = psc.SHAPES[psc.CASES[name]['shape']][3]
    moved = psc.CASES[name]['meridians']
    return R in (3, 6, 9, 10) and nlon >= 192 and nlon % (2 * R) == 0 and (nlon // R) % 16 == 0 and (moved is None or moved <= 1e-15)


def routes(name, plan, expect):
    """Sets every path and every rotation count in turn and yields its label; what the plan must refuse is checked to raise."""
    for path in psc.ALL_PATHS:
        if path not in expect['paths']:
            with pytest.raises(ShgError):
                plan.set_path(path)
            continue
        plan.set_path(path)
        if path != 'rot':
            yield path
            continue
        for R in (10, 9, 6, 3, 4, 12):
            if R in expect['counts']:
                plan.set_rotations(R)
                assert plan.info()['rotations'] == R and plan.info()['rotation_symmetry']
                yield 'rot{0}'.format(R)
            elif not meridians_allow(name, R):
                with pytest.raises(ShgError):
                    plan.set_rotations(R)
        plan.set_rotations(0)
        assert plan.info()['rotations'] == expect['rotations']
    if 'rot' not in expect['paths']:
        for R in (10, 9, 6, 3):
            if not meridians_allow(name, R):
                with pytest.raises(ShgError):
                    plan.set_rotations(R)
    plan.set_path('auto')


def set_route(plan, label):
    if label.startswith('rot'):
        plan.set_path('rot')
        plan.set_rotations(int(label[3:]))
    else:
        plan.set_path(label)


def run(plan, batch):
    return engine.to_host(plan.synthesis(batch))


def block_rows(nlat, blocks):
    """mask of the grid rows, north and south, whose 8-row block (counted from the north pole, mirrored in the south) is in `blocks`"""
    i = np.arange(nlat)
    north = np.minimum(i, nlat - 1 - i)
    return np.isin(north >> 3, sorted(blocks))


@pytest.mark.parametrize('name', list(psc.CASES))
def test_plan_info(name):
    plan, expect = make_plan(name)
    info = plan.info()
    assert info['north_south_symmetry'] == expect['north_south']
    assert info['fourfold_symmetry'] == expect['fourfold']
    assert info['rotation_symmetry'] == bool(expect['counts'])
    assert info['rotations'] == expect['rotations']
    assert info['fused'] == (len(expect['paths']) > 2)


@pytest.mark.parametrize('name', list(psc.CASES))
def test_synthesis_values_every_route(name):
    """Every path and rotation count the plan accepts, B = 1 and 5, within TOL of synthesis_tables: the accepted and flagged cases
    (own-table pass), the accepted and shared boundary, the rejected classes (plain variants, the kn-asymmetric one among them) and
    the moved meridians (evaluated at the moved meridians, whichever class they fall in)."""
    plan, expect = make_plan(name)
    batch, ref = coefficients(plan.max_degree), truth(name)
    seen = []
    for label in routes(name, plan, expect):
        for B in (1, EPOCHS):
            err = relerr(run(plan, batch[0:B]), ref[0:B])
            print('{0} {1} B={2}: {3:.2e}'.format(name, label, B, err))
            assert err < TOL, (label, B)
        seen.append(label)
    assert seen == [p for p in ('auto', 'fused', 'fused32') if p in expect['paths']] + ['rot{0}'.format(R) for R in expect['counts']] + ['staged']


@pytest.mark.parametrize('name', psc.ACCEPTED_FLAGGED + ('n45_both_none',))
def test_locality_bit_for_bit(name):
    """Against a plan on the exactly mirrored tables, on the same route: every grid row, north or south, whose 8-row block holds no
    moved mirror is the same to the bit (its tables are the same numbers; the second pass of another block must not touch it); the
    rows of the flagged blocks go through the two-pass form and are held to TOL of synthesis_tables."""
    plan, expect = make_plan(name)
    clean, _ = make_plan(name, mirrored=True)
    assert clean.info()['north_south_symmetry']
    batch, ref = coefficients(plan.max_degree), truth(name)
    flagged = block_rows(plan.nlat, {i >> 3 for i in expect['flagged']})
    assert flagged.any() == bool(expect['flagged'])
    for label in routes(name, plan, expect):
        set_route(clean, label)
        out, base = run(plan, batch), run(clean, batch)
        differ = np.flatnonzero((out[:, ~flagged, :] != base[:, ~flagged, :]).any(axis=(0, 2)))
        assert differ.size == 0, (label, np.flatnonzero(~flagged)[differ])
        if flagged.any():
            assert np.max(np.abs(out - ref)[:, flagged, :]) < TOL * np.max(np.abs(ref)), label
            assert (out[:, flagged, :] != base[:, flagged, :]).any(), label         # the moved mirrors do show in their own rows


@pytest.mark.parametrize('name', ['n45_both_blocks_0_3_last', 'n45_both_every_other', 'n96_both_last_block'])
def test_switching_on_one_plan(name):
    """auto -> fused -> rot with every count -> the plan's own count -> fused32 -> auto on ONE plan: after each switch the result is
    the one of that route on a fresh plan, bit for bit (the second tables are rebuilt with the layout of the new kernel)."""
    plan, expect = make_plan(name)
    batch = coefficients(plan.max_degree)
    fresh = {}

    def on_fresh_plan(label):
        if label not in fresh:
            other, _ = make_plan(name)
            set_route(other, label)
            fresh[label] = run(other, batch)
        return fresh[label]

    assert expect['counts'] and {'fused', 'fused32', 'rot'} <= set(expect['paths'])
    own = 'rot{0}'.format(expect['rotations'])
    assert np.array_equal(run(plan, batch), on_fresh_plan('auto'))
    assert np.array_equal(on_fresh_plan('auto'), on_fresh_plan(own))             # the automatic choice is the rotation-folded kernel
    plan.set_path('fused')
    assert np.array_equal(run(plan, batch), on_fresh_plan('fused'))
    plan.set_path('rot')
    for R in expect['counts'][::-1] + expect['counts']:
        plan.set_rotations(R)
        assert np.array_equal(run(plan, batch), on_fresh_plan('rot{0}'.format(R))), R
    plan.set_rotations(0)
    assert np.array_equal(run(plan, batch), on_fresh_plan(own))
    plan.set_path('fused32')
    assert np.array_equal(run(plan, batch), on_fresh_plan('fused32'))
    plan.set_path('auto')
    assert np.array_equal(run(plan, batch), on_fresh_plan('auto'))
    assert relerr(on_fresh_plan('fused32'), truth(name)) < TOL and relerr(on_fresh_plan('fused'), truth(name)) < TOL


def synthesis_om(plan, series):
    """the C call shg_synthesis_om itself (engine.Plan.synthesis falls back to the reference arrays where it is refused)"""
    import torch
    out = torch.empty((series.epochs, plan.nlat, plan.nlon), dtype=torch.float64, device=plan.device)
    ga._lib.call('shg_synthesis_om', plan._handle, engine._ptr(series.data), series.max_degree, series.epochs, series.padded_epochs,
                 engine._ptr(out), engine._stream())
    return engine.to_host(out)


def series_of(batch, extra):
    """order-major series of the batch, `extra` degrees higher (random coefficients there, which the plan must not read)"""
    B, n1 = batch.shape[0], batch.shape[1]
    wide = np.random.default_rng(77).standard_normal((B, n1 + extra, n1 + extra)) * 1e-10
    wide[:, :n1, :n1] = batch                    # C_nm at [n, m], S_nm at [m-1, n]: the degrees below n1 are the leading block
    return engine.OrderMajorSeries.from_batch(wide)


@pytest.mark.parametrize('name', psc.ACCEPTED_FLAGGED)
def test_order_major_input_flagged(name):
    """shg_synthesis_om on a flagged plan, series degree equal to the plan's and 7 higher: the batch result to the bit on every route
    that reads a series (the rotation-folded and the 64-row fused kernel); the other routes refuse the C call and the wrapper's
    fallback gives the batch result."""
    plan, expect = make_plan(name)
    batch = coefficients(plan.max_degree)
    reading = 0
    for label in routes(name, plan, expect):
        base = run(plan, batch)
        reads = label.startswith('rot') or label == 'fused' or (label == 'auto' and ('rot' in expect['paths'] or 'fused' in expect['paths']))
        for extra in (0, 7):
            series = series_of(batch, extra)
            if reads:
                assert np.array_equal(synthesis_om(plan, series), base), (label, extra)
                reading += 1
            else:
                with pytest.raises(ShgError) as refused:
                    synthesis_om(plan, series)
                assert refused.value.status == -1                                  # SHG_ERR_INVALID
            assert np.array_equal(run(plan, series), base), (label, extra)
        assert relerr(base, truth(name)) < TOL, label
    assert reading > 0 or not ({'rot', 'fused'} & set(expect['paths']))


@pytest.mark.parametrize('name', psc.REJECTED)
def test_order_major_input_rejected(name):
    """No fused kernel reads a series on parallels that are not symmetric about the equator: SHG_ERR_INVALID as include/shg.h
    documents, and the wrapper's fallback gives the right values."""
    plan, expect = make_plan(name)
    batch = coefficients(plan.max_degree)
    for label in routes(name, plan, expect):
        for extra in (0, 7):
            series = series_of(batch, extra)
            with pytest.raises(ShgError) as refused:
                synthesis_om(plan, series)
            assert refused.value.status == -1
            assert relerr(run(plan, series), truth(name)) < TOL, (label, extra)


@pytest.mark.parametrize('name', ['n45_both_blocks_0_3_last', 'n45_both_all', 'n45_kn_scaled'])
def test_analysis_on_caller_tables(name):
    """Plan.analysis with the grid's area weights on a flagged plan and on the kn-asymmetric one, nmin 0 and 3, against
    analysis_tables; the parity split, where the plan takes it, within the defect include/shg.h documents."""
    plan, expect = make_plan(name)
    N, colat, kn, lon, _ = psc.tables(name)
    area = psc.area(name)
    values = np.random.default_rng(31).standard_normal((2, plan.nlat, plan.nlon))
    for nmin in (0, 3):
        out = engine.to_host(plan.analysis(values, area, nmin))
        info = plan.analysis_info()
        assert info['parity_split'] is not None
        if info['parity_split']:
            assert expect['north_south'] and info['parity_defect'] < 5e-12
        for e in range(2):
            ref = orc.analysis_tables(values[e].ravel(), area.ravel(), nmin, N, colat, kn, lon)
            err = relerr(out[e], ref)
            print('{0} nmin={1} epoch {2}: {3:.2e} (parity split {4}, defect {5:.1e})'.format(name, nmin, e, err, info['parity_split'], info['parity_defect']))
            assert err < TOL, (nmin, e)
