"""
CPU checks of the basin API: the names of the reference's basin geometry exist with compatible signatures (the rule of
tests/test_api_signatures.py), the host-only parts (from_extent, bounding_box) are bit-equal to the reference, and the new C entry
points reject bad arguments before any HIP call.
"""
import ctypes

import numpy as np
import pytest

import grates_amd as ga
from test_api_signatures import API, compatible, params_of

BASIN_FUNCTIONS = ('spherical_pip', 'spherical_pib', 'winding_number')


@pytest.mark.parametrize('name', BASIN_FUNCTIONS)
def test_basin_function_signatures(name):
    assert hasattr(ga.grid, name), 'grid.{0} is missing'.format(name)
    why = compatible(API['modules']['grid'][name]['signature'], params_of(getattr(ga.grid, name)))
    assert why is None, why


def test_basin_class_and_create_mask_signatures():
    import inspect
    assert inspect.isclass(getattr(ga.grid, 'Basin', None)), 'grid.Basin is missing'
    for mname, mrec in API['modules']['grid']['Basin']['members'].items():
        member = inspect.getattr_static(ga.grid.Basin, mname)
        if mrec and isinstance(mrec[0], str):
            assert type(member).__name__ == mrec[0], mname
            ref, own = mrec[1:], params_of(member.__func__)
        else:
            ref, own = mrec, params_of(getattr(ga.grid.Basin, mname))
        assert compatible(ref, own) is None, (mname, compatible(ref, own))
    ref = API['modules']['grid']['Grid']['members']['create_mask']
    for cls in (ga.grid.Grid, ga.grid.RegularGrid, ga.grid.GeographicGrid, ga.grid.IrregularGrid):
        assert compatible(ref, params_of(cls.create_mask)) is None, cls
    assert callable(getattr(ga.grid.Grid, 'basin_statistics', None))


def test_from_extent_and_bounding_box_match_reference(golden):
    g = golden('g20_basin')
    import basin_inputs as bi
    box = ga.grid.Basin.from_extent(*bi.EXTENT)
    poly = box._Basin__polygons[0]
    assert poly.tobytes() == g['extent_polygon'].tobytes()
    assert np.array(box.bounding_box()).tobytes() == g['extent_bounding_box'].tobytes()
    multi = [g['poly_multi_{0}'.format(k)] for k in range(3)]
    assert np.array(ga.grid.Basin(multi).bounding_box()).tobytes() == g['multi_bounding_box'].tobytes()


def _error(lib):
    return lib.shg_last_error().decode()


def test_basin_entry_points_reject_bad_arguments():
    from grates_amd import _lib
    lib = _lib.load()
    frame = (ctypes.c_double * 5)()
    fp = ctypes.cast(frame, ctypes.c_void_p)
    dummy = ctypes.c_void_p(0x1000)                      # never dereferenced: validation fails first
    for name in ('shg_basin_pip', 'shg_basin_buffer'):
        assert getattr(lib, name)(0, None, 0, None, dummy, -1, fp, 3, dummy, 1, dummy, dummy, None) == -1
        assert 'negative size' in _error(lib), name
        assert getattr(lib, name)(2, None, 3, None, None, 6, fp, 3, dummy, 1, dummy, dummy, None) == -1
        assert 'NULL pointer' in _error(lib), name
        assert getattr(lib, name)(2, dummy, 3, dummy, None, 7, fp, 3, dummy, 1, dummy, dummy, None) == -1
        assert '7 points where the grid has 2 x 3' in _error(lib), name
        assert getattr(lib, name)(0, None, 0, None, dummy, 10, None, 3, dummy, 1, dummy, dummy, None) == -1
        assert 'NULL pointer' in _error(lib), name
    assert lib.shg_basin_buffer(0, None, 0, None, dummy, 10, fp, 3, dummy, 2, dummy, dummy, None) == -1
    assert 'value must be 0 or 1' in _error(lib)
    assert lib.shg_winding_number(-1, dummy, dummy, dummy, 4, dummy, None) == -1
    assert 'negative size' in _error(lib)
    assert lib.shg_winding_number(3, dummy, None, dummy, 4, dummy, None) == -1
    assert 'NULL pointer' in _error(lib)
    assert lib.shg_mask_pack(dummy, 65, 10, dummy, None) == -1
    assert 'at most 64' in _error(lib)
    assert lib.shg_mask_pack(dummy, 3, -1, dummy, None) == -1
    assert 'negative size' in _error(lib)
    with pytest.raises(_lib.ShgError, match='65 masks, 1 to 64 are supported'):
        _lib.call('shg_basin_statistics', dummy, 4, 10, dummy, dummy, 65, dummy, None)
    with pytest.raises(_lib.ShgError, match='NULL pointer'):
        _lib.call('shg_basin_statistics', None, 4, 10, dummy, dummy, 2, dummy, None)
    with pytest.raises(_lib.ShgError, match='negative size'):
        _lib.call('shg_basin_statistics', dummy, -4, 10, dummy, dummy, 2, dummy, None)
    with pytest.raises(_lib.ShgError, match='no points'):
        _lib.call('shg_basin_statistics', dummy, 4, 0, dummy, dummy, 2, dummy, None)
