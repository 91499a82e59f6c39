"""
The half column tile of the rotation-folded synthesis kernel (shg_plan_set_half_tile_fold; DESIGN.md 4.1 "The half column tile") on the
GPU.  Where the fundamental domain has nd = nlon / (2 R) = 8 mod 16 columns, the last column tile runs on the 16 real columns
nd - 8 .. nd + 7 and stores its R ascending images only: the descending image k of the columns c = nd - 8 .. nd - 1 is the ascending image
k - 1 of the columns 2 nd - 1 - c.  With the switch off that tile forms all 2 R images like every other tile.

Plans far below the headline's size, built from custom meridians: R = 10 / 9 / 6 on 480 / 432 / 288 meridians (nd = 24, 1.5 tiles), R = 3
on 240 (nd = 40, 2.5 tiles) and, as the control without a half tile, R = 3 on 192 (nd = 32); d/o 12 and 40; 5 epochs (a ragged epoch
tile); 24 parallels symmetric about the equator (the second latitude block is partial) and 20 shifted parallels (the plain variant).
Every grid is held against the CPU oracle (max|d| / max|ref| < 1e-12) with the switch on and off; the two agree bit for bit
outside the 8 R columns of the former descending images and within the same tolerance inside them.
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
B = 5
HALF_TILE = [(10, 480), (9, 432), (6, 288), (3, 240)]
CONTROL = [(3, 192)]


def small_grid(nlon, symmetric):
    mer = np.linspace(-np.pi, np.pi, nlon, endpoint=False) + np.pi / nlon
    nlat = 24 if symmetric else 20
    par = np.pi / 2 - (np.arange(nlat) + 0.5) * np.pi / nlat
    if not symmetric:
        par = par + 0.013                    # all parallels shifted north: no parallel has a mirror image
    return ga.grid.RegularGrid(mer, par)


def rot_plan(grid, N, R, symmetric):
    colat, _, kn = ga.gravityfield.surface_factors(ga.kernel.get_kernel('potential'), N, grid.parallels, GM, RE, grid.semimajor_axis, grid.flattening)
    plan = ga.engine.Plan(N, colat, kn, grid.meridians)
    plan.set_rotations(R)
    plan.set_path('rot')
    info = plan.info()
    assert info['rotations'] == R and info['north_south_symmetry'] == symmetric, info
    return plan


def run_into_nan(plan, batch, shape):
    """The grids of `batch`, written into a tensor that was all NaN: whatever the kernel does not store stays NaN."""
    import torch
    out = torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')
    plan.synthesis(ga.engine.to_device(batch), out=out)
    return ga.engine.to_host(out)


def former_descending_columns(R, nlon):
    """The columns that the descending images of c = nd - 8 .. nd - 1 write with the switch off."""
    nd, n2, nR = nlon // (2 * R), nlon // 2, nlon // R
    return sorted({(n2 + k * nR - 1 - c) % nlon for k in range(R) for c in range(nd - 8, nd)})


@pytest.mark.parametrize('symmetric', [True, False])
@pytest.mark.parametrize('N', [12, 40])
@pytest.mark.parametrize('R,nlon', HALF_TILE + CONTROL)
def test_half_tile_fold(R, nlon, N, symmetric):
    grid = small_grid(nlon, symmetric)
    nlat = grid.parallels.size
    half = (R, nlon) in HALF_TILE
    assert (nlon // (2 * R)) % 16 == (8 if half else 0)
    plan = rot_plan(grid, N, R, symmetric)
    batch = bench.coefficient_batch(5000 + N, B, N)
    pot = orc.KernelTable('potential')
    ref = np.stack([orc.synthesis_regular(batch[e], grid.meridians, grid.parallels, pot) for e in range(B)])
    scale = np.max(np.abs(ref))

    assert plan.info()['half_tile_fold'] == half                       # on by default wherever there is a half tile
    on = run_into_nan(plan, batch, (B, nlat, nlon))
    plan.set_half_tile_fold(False)
    assert not plan.info()['half_tile_fold']
    off = run_into_nan(plan, batch, (B, nlat, nlon))
    plan.set_half_tile_fold(True)
    assert plan.info()['half_tile_fold'] == half

    # 1. coverage: every grid point is stored
    assert not np.isnan(on).any(), np.argwhere(np.isnan(on))[:8]
    assert not np.isnan(off).any(), np.argwhere(np.isnan(off))[:8]
    # 2. oracle
    err_on, err_off = relerr(on, ref), relerr(off, ref)
    print('R {0} nlon {1} N {2} symmetric {3}: fold on {4:.2e}, off {5:.2e}'.format(R, nlon, N, symmetric, err_on, err_off))
    assert err_on < TOL and err_off < TOL, (err_on, err_off)
    # 3. on against off
    if half:
        cols = former_descending_columns(R, nlon)
        assert len(cols) == 8 * R
        rest = np.setdiff1d(np.arange(nlon), cols)
        assert np.array_equal(on[:, :, rest], off[:, :, rest])
        diff = float(np.max(np.abs(on[:, :, cols] - off[:, :, cols])) / scale)
        print('   former descending columns: max|on - off| / max|ref| = {0:.2e}'.format(diff))
        assert diff < TOL, diff
    else:
        assert np.array_equal(on, off)
    # 4. partial batches, fold on
    for nb in (1, 2, 3):
        part = run_into_nan(plan, batch[:nb], (nb, nlat, nlon))
        assert np.array_equal(part, on[:nb]), nb
