"""
Ticket limit on the Legendre stage of the rotation-folded synthesis kernel (shg_plan_set_stage_limit; DESIGN.md 4.1 "Tickets") on the
GPU.  The limit changes the schedule of the workgroups, never what one of them computes: every grid must be bit-identical to the same
plan's grid without a limit, and that one within 1e-12 of the CPU oracle (max|d| / max|ref|).

Plans far below the headline's size: R = 10 / 9 / 6 rotations on 320 / 288 / 192 meridians, d/o 12 and 40, 48 and 50 parallels (50: a
ragged last latitude block), with and without the north-south symmetry, 1 / 5 / 9 / 33 epochs (ragged epoch tiles; 3 to 36 workgroups,
fewer and more than the eight per-XCD queues), and one of 60 workgroups for the limit of one.
"""
import numpy as np
import pytest

import bench
import grates_amd as ga
from conftest import relerr
from oracle import shg_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-12
GM, RE = 3.9860044150e+14, 6.3781363000e+06
EPOCHS = (1, 5, 9, 33)
LIMITS = (1, 2, 8, 1000, -1, -16)            # beside 0; 1000 is above every workgroup count of this file


def small_grid(nlon, nlat, symmetric):
    mer = np.linspace(-np.pi, np.pi, nlon, endpoint=False) + np.pi / nlon
    par = np.pi / 2 - (np.arange(nlat) + 0.5) * np.pi / nlat
    if not symmetric:
        par[nlat - 3] += 1e-6
    return ga.grid.RegularGrid(mer, par)


def tables(grid, N, kernel='potential'):
    colat, _, kn = ga.gravityfield.surface_factors(ga.kernel.get_kernel(kernel), N, grid.parallels, GM, RE, grid.semimajor_axis, grid.flattening)
    return colat, kn, grid.meridians


def rot_plan(grid, N, R, symmetric, kernel='potential'):
    plan = ga.engine.Plan(N, *tables(grid, N, kernel))
    plan.set_path('rot')
    info = plan.info()
    assert info['rotations'] == R and info['north_south_symmetry'] == symmetric, info
    return plan


def run(plan, batch):
    return ga.engine.to_host(plan.synthesis(batch))


@pytest.mark.parametrize('symmetric', [True, False])
@pytest.mark.parametrize('nlat', [48, 50])
@pytest.mark.parametrize('N', [12, 40])
@pytest.mark.parametrize('R,nlon', [(10, 320), (9, 288), (6, 192)])
def test_limits_change_no_bit(R, nlon, N, nlat, symmetric):
    grid = small_grid(nlon, nlat, symmetric)
    plan = rot_plan(grid, N, R, symmetric)
    batch = bench.coefficient_batch(4000 + N, max(EPOCHS), N)
    pot = orc.KernelTable('potential')
    ref = np.stack([orc.synthesis_regular(batch[e], grid.meridians, grid.parallels, pot) for e in range(max(EPOCHS))])
    for B in EPOCHS:
        plan.set_stage_limit(0)
        base = run(plan, batch[:B])
        assert base.shape == (B, nlat, nlon)
        err = relerr(base, ref[:B])
        assert err < TOL, (B, err)
        for limit in LIMITS:
            plan.set_stage_limit(limit)
            assert np.array_equal(run(plan, batch[:B]), base), (B, limit)


def test_limit_of_one_hands_over_in_normal_time():
    """60 workgroups, one in the stage per queue: every ticket but the first of a queue waits for the one before it, so every hand-over
    path runs.  A wait that ended on its time-out instead (milliseconds per waiter) would pass the comparison above; it fails here: the
    launches with the limit take less than 50 times what they take without it."""
    import torch
    grid = small_grid(320, 50, True)
    plan = rot_plan(grid, 12, 10, True)
    batch = ga.engine.to_device(bench.coefficient_batch(4100, 60, 12))          # 15 epoch tiles x 4 latitude blocks
    out = torch.empty((60, 50, 320), dtype=torch.float64, device='cuda')
    launches = 20

    def timed(limit):
        plan.set_stage_limit(limit)
        for _ in range(3):
            plan.synthesis(batch, out=out)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(launches):
            plan.synthesis(batch, out=out)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / launches, ga.engine.to_host(out)

    t0, base = timed(0)
    t1, got = timed(1)
    print('limit 0: {0:.1f} us per launch, limit 1: {1:.1f} us'.format(1e3 * t0, 1e3 * t1))
    assert np.array_equal(got, base)
    assert t1 < 50 * t0, (t0, t1)


def test_repeated_launches_find_the_queues_at_zero():
    """Two launches in a row, another batch size (the block map is rebuilt), the limit changed between launches: all as without a limit."""
    grid = small_grid(288, 50, True)
    plan = rot_plan(grid, 40, 9, True)
    batch = bench.coefficient_batch(4200, 33, 40)
    base = {B: run(plan, batch[:B]) for B in (33, 9, 5)}
    plan.set_stage_limit(2)
    for B in (33, 33, 9, 9, 33, 5):
        assert np.array_equal(run(plan, batch[:B]), base[B]), B
    for limit, B in ((1, 33), (8, 33), (-1, 9), (1, 9), (0, 33), (3, 33), (3, 5), (-16, 33)):
        plan.set_stage_limit(limit)
        assert np.array_equal(run(plan, batch[:B]), base[B]), (limit, B)
        assert np.array_equal(run(plan, batch[:B]), base[B]), (limit, B)
