"""
Golden vectors of the basin geometry and basin statistics (g20_basin.npz).  Run once where the reference is available:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_basin.py

Like make_golden.py it imports the reference package with empty stand-ins for netCDF4 / h5py and stores only seeds, inputs and
reference outputs.  Masks are stored with np.packbits.  For every mask case a `fragile` bitmap marks the points whose reference
answer changes when the point's longitude or latitude moves by +-4 ulp (four more reference runs): there the reference's own
rounding -- its cap test and buffer products go through BLAS -- decides, and a device result may differ.
"""

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

for _name, _attr in (('netCDF4', 'Dataset'), ('h5py', 'File')):
    if _name not in sys.modules:
        _mod = types.ModuleType(_name)
        setattr(_mod, _attr, None)
        sys.modules[_name] = _mod
sys.dont_write_bytecode = True
sys.path.insert(0, '/root/reference')
import grates  # noqa: E402

sys.path.insert(0, HERE)
import basin_inputs as bi  # noqa: E402


def shifted(x, ulps):
    out = np.array(x, dtype=float, copy=True)
    for _ in range(abs(ulps)):
        out = np.nextafter(out, np.inf if ulps > 0 else -np.inf)
    return out


def mask_and_fragile(basin, lon, lat, buffer=None):
    base = basin.contains_points(lon, lat, buffer)
    fragile = np.zeros(base.shape, dtype=bool)
    for dlon, dlat in ((4, 0), (-4, 0), (0, 4), (0, -4)):
        fragile |= basin.contains_points(shifted(lon, dlon), shifted(lat, dlat), buffer) != base
    return base, fragile


def main():
    out = {}

    def store(tag, mask, fragile):
        out['mask_' + tag] = np.packbits(mask)
        out['fragile_' + tag] = np.packbits(fragile)
        out['count_' + tag] = np.array([mask.size, np.count_nonzero(mask), np.count_nonzero(fragile)])
        print('{0:12s} points {1:8d} inside {2:7d} fragile {3:4d}'.format(tag, mask.size, np.count_nonzero(mask), np.count_nonzero(fragile)))

    g05 = grates.grid.GeographicGrid(0.5, 0.5)
    polys = bi.polygons()
    for tag, p in polys.items():
        for k, part in enumerate(p if isinstance(p, list) else [p]):
            out['poly_{0}_{1}'.format(tag, k)] = part
    for tag in ('star500', 'star2000', 'antimeridian', 'southpole', 'multi'):
        p = polys[tag]
        basin = grates.grid.Basin(p)
        store(tag, *mask_and_fragile(basin, g05.longitude, g05.latitude))
    star = polys['star500']
    for tag, buffer in (('buffer_pos', 200e3), ('buffer_neg', -200e3)):
        store(tag, *mask_and_fragile(grates.grid.Basin(star), g05.longitude, g05.latitude, buffer))
    store('closed', *mask_and_fragile(grates.grid.Basin(np.append(star, star[:1], axis=0)), g05.longitude, g05.latitude))
    store('reversed', *mask_and_fragile(grates.grid.Basin(star[::-1].copy()), g05.longitude, g05.latitude))

    box = grates.grid.Basin.from_extent(*bi.EXTENT)
    out['extent_polygon'] = np.asarray(box._Basin__polygons[0])
    out['extent_bounding_box'] = np.array(box.bounding_box())
    out['multi_bounding_box'] = np.array(grates.grid.Basin(polys['multi']).bounding_box())
    meridians, parallels = bi.edge_grid_axes()
    rg = grates.grid.RegularGrid(meridians, parallels)
    store('extent', *mask_and_fragile(box, rg.longitude, rg.latitude))

    lon, lat = bi.scattered_points()
    store('irregular', *mask_and_fragile(grates.grid.Basin(star), lon, lat))
    gg = grates.grid.GaussGrid(bi.GAUSS_PARALLELS)
    store('gauss', *mask_and_fragile(grates.grid.Basin(star), gg.longitude, gg.latitude))

    out['winding'] = np.packbits(grates.grid.winding_number(star, g05.longitude, g05.latitude))

    slon, slat = bi.scalar_points()
    out['scalar_inside'] = np.array([grates.grid.Basin(star).contains_points(x, y)[0] for x, y in zip(slon, slat)])
    # a scalar latitude against an array of longitudes (the reference's geodetic2cartesian cannot stack a scalar row with array
    # rows, so the latitude is broadcast here)
    out['scalar_lat'] = grates.grid.Basin(star).contains_points(slon, np.full(slon.shape, slat[0]))

    # area-weighted statistics of one grid with seeded values (grates/grid.py:174-260)
    sg = grates.grid.GeographicGrid(bi.STATS_STEP, bi.STATS_STEP)
    sg.values = bi.stats_values(sg.point_count)
    for tag in ('star500', 'multi'):
        m = grates.grid.Basin(polys[tag]).contains_points(sg.longitude, sg.latitude)
        out['stats_mask_' + tag] = np.packbits(m)
        out['stats_' + tag] = np.array([sg.mean(m), sg.rms(m), sg.std(m)])
    path = os.path.join(HERE, 'g20_basin.npz')
    np.savez_compressed(path, **out)
    print('g20_basin {0:.1f} KB'.format(os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
