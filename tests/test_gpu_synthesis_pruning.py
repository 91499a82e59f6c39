"""
Order pruning of the rotation-folded synthesis kernel on the GPU: latitude blocks next to a pole keep the
orders up to their cut-off level only.  Pruned grids against the same plan with pruning off and against the CPU oracle
(tolerance of SURVEY.md 8d: max|d| / max|ref| <= 1e-12), on the headline plan with a ragged epoch tile, on plans made of polar
parallels only (every rotation count, three degrees), and without the north-south symmetry.

Pruned against unpruned: the dropped terms are below 1e-30 of a parallel's largest term, so the bound is 1e-20 of the field's
maximum (ten orders of magnitude above what 1e-30 allows for 96 dropped terms, eight below the oracle tolerance).  Measured on
MI355X: max|pruned - unpruned| / max|ref| = 0 in every case of this file, the grids are bit-identical; the headline case therefore
asserts equality, the others the bound.
"""
import numpy as np
import pytest

import bench
import grates_amd as ga
from conftest import relerr
from oracle import shg_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-12
PRUNE_TOL = 1e-20
GM, RE = 3.9860044150e+14, 6.3781363000e+06


def love():
    return ga.data.load_love_numbers()[0]


def tables(grid, N, kernel='ewh'):
    colat, _, kn = ga.gravityfield.surface_factors(ga.kernel.get_kernel(kernel), N, grid.parallels, GM, RE, grid.semimajor_axis, grid.flattening)
    return colat, kn, grid.meridians


def both(plan, batch):
    """grids with pruning on and off (host arrays)"""
    assert plan.info()['order_pruning']                             # the default
    plan.set_order_pruning(True)
    assert plan.info()['order_pruning']
    on = ga.engine.to_host(plan.synthesis(batch))
    plan.set_order_pruning(False)
    assert not plan.info()['order_pruning']
    off = ga.engine.to_host(plan.synthesis(batch))
    plan.set_order_pruning(True)
    return on, off


def test_pruned_against_unpruned_and_oracle():
    """d/o 96 -> 0.25 degree, R = 10, five epochs (epoch tiles of 4 + 1)."""
    grid = ga.grid.GeographicGrid(0.25, 0.25)
    batch = bench.coefficient_batch(1000, 5, 96)
    plan = ga.engine.Plan(96, *tables(grid, 96))
    info = plan.info()
    assert info['rotations'] == 10 and info['path'] in (0, 6) and info['order_pruning']
    assert info['order_cutoffs'][:11] == [39, 49, 49, 59, 69, 69, 79, 79, 89, 89, 89] and set(info['order_cutoffs'][11:]) == {96}
    on, off = both(plan, batch)
    ker = orc.KernelTable('ewh', love())
    scale = 0.0
    for e in (0, 4):
        ref = orc.synthesis_regular(batch[e], grid.meridians, grid.parallels, ker)
        scale = max(scale, float(np.max(np.abs(ref))))
        assert relerr(on[e], ref) < TOL, e
        assert relerr(off[e], ref) < TOL, e
    delta = float(np.max(np.abs(on - off))) / scale
    print('pruned against unpruned: max|d| / max|ref| = {0:.3e}'.format(delta))
    assert delta <= PRUNE_TOL
    assert np.array_equal(on, off)                                  # measured 0: bit-identical


def polar_grid(shift=None):
    g = ga.grid.GeographicGrid(0.25, 0.25)
    par = np.concatenate([g.parallels[:16], g.parallels[-16:]])       # the 16 parallels next to each pole: two symmetric blocks
    if shift is not None:
        par[shift] += 1e-6
    return ga.grid.RegularGrid(g.meridians, par)


@pytest.fixture(scope='module')
def polar_cases():
    """(grid, batch, oracle grids) per degree, shared by the rotation counts"""
    grid, ker, out = polar_grid(), orc.KernelTable('ewh', love()), {}
    for N in (96, 40, 12):
        batch = bench.coefficient_batch(2000 + N, 4, N)
        out[N] = (grid, batch, np.stack([orc.synthesis_regular(batch[e], grid.meridians, grid.parallels, ker) for e in range(4)]))
    return out


@pytest.mark.parametrize('R', [10, 9, 6, 3])
@pytest.mark.parametrize('N', [96, 40, 12])
def test_polar_plan_every_rotation_count(polar_cases, N, R):
    grid, batch, ref = polar_cases[N]
    plan = ga.engine.Plan(N, *tables(grid, N))
    plan.set_rotations(R)
    info = plan.info()
    assert info['rotations'] == R and info['north_south_symmetry'] and len(info['order_cutoffs']) == 2
    if N == 12:
        assert info['order_cutoffs'] == [12, 12]
    else:
        assert all(level < N for level in info['order_cutoffs']), info['order_cutoffs']
    on, off = both(plan, batch)
    assert on.shape == (4, 32, 1440)
    assert relerr(on, ref) < TOL
    assert relerr(off, ref) < TOL
    delta = float(np.max(np.abs(on - off)) / np.max(np.abs(ref)))
    print('d/o {0}, R = {1}: pruned against unpruned {2:.3e}'.format(N, R, delta))
    assert delta <= PRUNE_TOL


@pytest.mark.parametrize('R', [10, 9, 6, 3])
def test_polar_plan_without_north_south_symmetry(R):
    grid = polar_grid(shift=20)
    batch = bench.coefficient_batch(3000, 4, 96)
    ker = orc.KernelTable('ewh', love())
    ref = np.stack([orc.synthesis_regular(batch[e], grid.meridians, grid.parallels, ker) for e in range(4)])
    plan = ga.engine.Plan(96, *tables(grid, 96))
    plan.set_rotations(R)
    info = plan.info()
    assert not info['north_south_symmetry'] and info['rotations'] == R
    assert info['order_cutoffs'] == [49, 49]                        # blocks of 16 consecutive parallels
    on, off = both(plan, batch)
    assert relerr(on, ref) < TOL
    assert relerr(off, ref) < TOL
    assert float(np.max(np.abs(on - off)) / np.max(np.abs(ref))) <= PRUNE_TOL
