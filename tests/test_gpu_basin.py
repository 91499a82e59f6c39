"""
Basin masks and basin statistics on the GPU against the reference (tests/golden/g20_basin.npz, tests/golden/make_golden_basin.py):
masks equal the reference at every point whose answer does not depend on the reference's own rounding (the fixture's fragile set),
the planar winding number everywhere; basin_statistics agrees with the host Grid.mean / rms / std of the same grids.
"""
import datetime

import numpy as np
import pytest

import basin_inputs as bi
import grates_amd as ga

pytestmark = pytest.mark.gpu

GRID_CASES = ('star500', 'star2000', 'antimeridian', 'southpole', 'multi', 'closed', 'reversed', 'buffer_pos', 'buffer_neg')


def _polygons(g, tag):
    parts = sorted(k for k in g if k.startswith('poly_{0}_'.format(tag)))
    return [g[k] for k in parts] if len(parts) > 1 else g[parts[0]]


def _basin(g, tag):
    star = g['poly_star500_0']
    if tag == 'closed':
        return ga.grid.Basin(np.append(star, star[:1], axis=0)), None
    if tag == 'reversed':
        return ga.grid.Basin(star[::-1].copy()), None
    if tag.startswith('buffer'):
        return ga.grid.Basin(star), 200e3 if tag == 'buffer_pos' else -200e3
    return ga.grid.Basin(_polygons(g, tag)), None


def _check(g, tag, mask):
    n = int(g['count_' + tag][0])
    ref = np.unpackbits(g['mask_' + tag], count=n).astype(bool)
    fragile = np.unpackbits(g['fragile_' + tag], count=n).astype(bool)
    mask = np.asarray(mask).ravel()
    assert mask.dtype == bool and mask.size == n
    assert fragile.sum() < 1e-3 * n, tag
    bad = np.flatnonzero((mask != ref) & ~fragile)
    assert bad.size == 0, '{0}: {1} points differ from the reference outside the fragile set, e.g. {2}'.format(tag, bad.size, bad[:5])
    assert np.count_nonzero(ref) > 0 or tag == 'buffer_neg'


@pytest.mark.parametrize('tag', GRID_CASES)
def test_grid_masks_match_reference(golden, tag):
    g = golden('g20_basin')
    grid = ga.grid.GeographicGrid(0.5, 0.5)
    basin, buffer = _basin(g, tag)
    _check(g, tag, grid.create_mask(basin, buffer))


def test_extent_gauss_and_point_list_masks(golden):
    g = golden('g20_basin')
    box = ga.grid.Basin.from_extent(*bi.EXTENT)
    meridians, parallels = bi.edge_grid_axes()
    _check(g, 'extent', ga.grid.RegularGrid(meridians, parallels).create_mask(box))
    star = ga.grid.Basin(g['poly_star500_0'])
    lon, lat = bi.scattered_points()
    _check(g, 'irregular', star.contains_points(lon, lat))
    _check(g, 'irregular', ga.grid.IrregularGrid(lon, lat).create_mask(star))
    _check(g, 'gauss', ga.grid.GaussGrid(bi.GAUSS_PARALLELS).create_mask(star))


def test_module_functions_and_scalars(golden):
    g = golden('g20_basin')
    star = g['poly_star500_0']
    grid = ga.grid.GeographicGrid(0.5, 0.5)
    _check(g, 'star500', ga.grid.spherical_pip(star, grid.longitude, grid.latitude))
    # the buffer alone: points of the +200 km mask that the polygon itself does not contain
    pib = ga.grid.spherical_pib(star, grid.longitude, grid.latitude, 200e3)
    inside = ga.grid.spherical_pip(star, grid.longitude, grid.latitude)
    _check(g, 'buffer_pos', inside | pib)
    winding = ga.grid.winding_number(star, grid.longitude, grid.latitude)
    assert np.array_equal(winding, np.unpackbits(g['winding'], count=grid.point_count).astype(bool))
    slon, slat = bi.scalar_points()
    basin = ga.grid.Basin(star)
    got = [basin.contains_points(x, y) for x, y in zip(slon, slat)]
    assert all(r.shape == (1,) for r in got)
    assert np.array_equal(np.concatenate(got), g['scalar_inside'])
    assert np.array_equal(basin.contains_points(slon, slat[0]), g['scalar_lat'])


def test_tensor_mask_equals_host_mask(golden):
    import torch
    g = golden('g20_basin')
    grid = ga.grid.GeographicGrid(0.5, 0.5)
    basin = ga.grid.Basin(_polygons(g, 'multi'))
    t = grid.create_mask(basin, as_tensor=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bool and tuple(t.shape) == (grid.point_count,)
    assert np.array_equal(t.cpu().numpy(), grid.create_mask(basin))
    # separable grid tables and the point list of the same grid give the same answer
    assert np.array_equal(t.cpu().numpy(), basin.contains_points(grid.longitude, grid.latitude))


def test_statistics_match_reference_fixture(golden):
    import torch
    g = golden('g20_basin')
    grid = ga.grid.GeographicGrid(bi.STATS_STEP, bi.STATS_STEP)
    values = torch.from_numpy(bi.stats_values(grid.point_count)).cuda()[None, :]
    masks = np.stack([np.unpackbits(g['stats_mask_' + tag], count=grid.point_count).astype(bool) for tag in ('star500', 'multi')])
    mean, rms, std = grid.basin_statistics(values, masks)
    for b, tag in enumerate(('star500', 'multi')):
        got = np.array([mean[0, b].item(), rms[0, b].item(), std[0, b].item()])
        np.testing.assert_allclose(got, g['stats_' + tag], rtol=1e-13, atol=0)


def _star_masks(grid):
    """16 basins on the grid: 8 disjoint stars and 8 that overlap them or each other"""
    import torch
    basins = []
    for k in range(8):
        basins.append(bi.star(300, -150.0 + 40.0 * k, -40.0 + 10.0 * k, 0.25, 100 + k))
    for k in range(8):
        basins.append(bi.star(200, -140.0 + 40.0 * k, -35.0 + 10.0 * k, 0.35, 200 + k))
    return torch.stack([grid.create_mask(ga.grid.Basin(b), as_tensor=True) for b in basins])


def _host_stats(grid, values, masks):
    """host mean, rms, std per mask, and the weighted mean of |v|: the scale of the mean's sum (a mean far below it is a sum
    that cancels, whose relative error any summation order magnifies by that ratio)"""
    g, a = grid.copy(), grid.copy()
    g.values, a.values = values.ravel(), np.abs(values.ravel())
    return np.array([[g.mean(m), g.rms(m), g.std(m), a.mean(m)] for m in masks])


def _relerr(a, b):
    return np.max(np.abs(a - b) / np.abs(b))


def _mean_err(a, ref):
    return np.max(np.abs(a - ref[:, 0]) / ref[:, 3])


def test_full_size_series_statistics():
    import torch
    T, N = 240, 96
    rng = np.random.default_rng(96)
    series = []
    for e in range(T):
        gf = ga.gravityfield.PotentialCoefficients()
        gf.anm = rng.standard_normal((N + 1, N + 1)) * 1e-10
        gf.epoch = datetime.datetime(2002, 4, 1) + datetime.timedelta(days=30 * e)
        series.append(gf)
    grid = ga.grid.GeographicGrid(0.25, 0.25)
    values = ga.gravityfield.TimeSeries(series).to_grid(grid, as_tensor=True)
    assert tuple(values.shape) == (T, 720, 1440)
    masks = _star_masks(grid)
    counts = masks.sum(dim=1).cpu().numpy()
    assert counts.min() > 100 and (masks.sum(dim=0) > 1).any()        # non-empty, and some points in two basins
    mean, rms, std = grid.basin_statistics(values, masks)
    assert tuple(mean.shape) == (T, 16) and mean.dtype == torch.float64 and mean.is_cuda
    mean2, rms2, std2 = grid.basin_statistics(values, masks)
    for a, b in ((mean, mean2), (rms, rms2), (std, std2)):
        assert torch.equal(a, b)                                        # bitwise reproducible
    gmean, grms, gstd = grid.basin_statistics(values.reshape(T, -1))     # all points
    assert tuple(gmean.shape) == (T, 1)
    host_masks = masks.cpu().numpy()
    offset = 1e6 * float(gstd[0, 0])
    shifted = values + offset
    smean, srms, sstd = grid.basin_statistics(shifted, masks)
    for e in (0, 119, 239):
        v = values[e].cpu().numpy()
        ref = _host_stats(grid, v, host_masks)
        assert _mean_err(mean[e].cpu().numpy(), ref) <= 1e-13, e
        assert _relerr(rms[e].cpu().numpy(), ref[:, 1]) <= 1e-13, e
        assert _relerr(std[e].cpu().numpy(), ref[:, 2]) <= 1e-12, e
        ref_all = _host_stats(grid, v, [None])[0]
        assert abs(gmean[e, 0].item() - ref_all[0]) <= 1e-13 * ref_all[3], e
        np.testing.assert_allclose(grms[e, 0].item(), ref_all[1], rtol=1e-13, atol=0)
        np.testing.assert_allclose(gstd[e, 0].item(), ref_all[2], rtol=1e-12, atol=0)
        sref = _host_stats(grid, shifted[e].cpu().numpy(), host_masks)
        assert _relerr(sstd[e].cpu().numpy(), sref[:, 2]) <= 1e-12, e
        assert _mean_err(smean[e].cpu().numpy(), sref) <= 1e-13, e


def test_statistics_edge_cases_and_argument_errors():
    import torch
    grid = ga.grid.GeographicGrid(5.0, 5.0)
    P = grid.point_count
    values = torch.randn((3, P), dtype=torch.float64, device='cuda')
    masks = torch.zeros((2, P), dtype=torch.bool, device='cuda')
    masks[1, :10] = True
    mean, rms, std = grid.basin_statistics(values, masks)
    assert torch.isnan(mean[:, 0]).all() and torch.isnan(rms[:, 0]).all() and torch.isnan(std[:, 0]).all()
    assert torch.isfinite(mean[:, 1]).all()
    # an IrregularGrid without explicit areas: equal weights
    pts = ga.grid.IrregularGrid(grid.longitude, grid.latitude)
    m, r, s = pts.basin_statistics(values, masks[1])
    h = pts.copy()
    h.values = values[2].cpu().numpy()
    np.testing.assert_allclose([m[2, 0].item(), r[2, 0].item(), s[2, 0].item()],
                               [h.mean(masks[1].cpu().numpy()), h.rms(masks[1].cpu().numpy()), h.std(masks[1].cpu().numpy())], rtol=1e-13)
    with pytest.raises(ValueError):
        grid.basin_statistics(values[:, :-1].contiguous(), masks)                # wrong P
    with pytest.raises(ValueError):
        grid.basin_statistics(values.float(), masks)                              # not float64
    with pytest.raises(ValueError):
        grid.basin_statistics(torch.randn((P, 3), dtype=torch.float64, device='cuda').T, masks)   # not contiguous
    with pytest.raises(ValueError):
        grid.basin_statistics(values, masks[:, :-1])                              # mask of the wrong size
    with pytest.raises(ValueError):
        grid.basin_statistics(values, torch.ones((65, P), dtype=torch.bool, device='cuda'))
    with pytest.raises(ValueError):
        grid.basin_statistics(values.cpu(), masks)                               # host values
