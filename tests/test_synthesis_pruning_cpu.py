"""
Order pruning of the rotation-folded synthesis kernel, host side (no device): the cut-off level of every latitude block and the
per-level tables, through the device-free entry points shg_rot_order_cutoffs / shg_rot_level_tables.

* the levels of the headline plan (ewh, d/o 96, 0.25 degree) are the ones DESIGN.md 4.1 (b) priced, monotone from the pole to the
  equator, and N from the twelfth block on; d/o 12 prunes nothing;
* the tables of the top level are byte-equal to the unpruned kernel's tables, rebuilt here from their documented rules (class
  layout, zero padding to whole k-steps, trig stream with a spare piece, work items dealt longest first to the wave with the
  fewest items) with the C library's cos / sin; a lower level holds the front of the same order sequence.
"""
import ctypes
import math

import numpy as np
import pytest

import grates_amd as ga
from grates_amd import _lib

GM, RE = 3.9860044150e+14, 6.3781363000e+06
DESIGN_LEVELS = [39, 49, 49, 59, 69, 69, 79, 79, 89, 89, 89]      # first eleven of the 45 blocks


def tables(parallels, N, kernel, grid):
    colat, _, kn = ga.gravityfield.surface_factors(ga.kernel.get_kernel(kernel), N, parallels, GM, RE, grid.semimajor_axis, grid.flattening)
    return np.ascontiguousarray(colat, dtype=np.float64), np.ascontiguousarray(kn, dtype=np.float64)


def cutoffs(N, colat, kn):
    levels, n = (ctypes.c_int * 4096)(), ctypes.c_int(0)
    _lib.call('shg_rot_order_cutoffs', N, colat.size, ctypes.c_void_p(colat.ctypes.data), ctypes.c_void_p(kn.ctypes.data), levels, 4096, ctypes.byref(n))
    return [levels[i] for i in range(n.value)]


def level_tables(R, N, level, ns, lon):
    lon = np.ascontiguousarray(lon, dtype=np.float64)
    header = (ctypes.c_int32 * 24)()
    args = (R, N, level, 1 if ns else 0, lon.size, ctypes.c_void_p(lon.ctypes.data), header)
    _lib.call('shg_rot_level_tables', *args, None, 0, None, 0)
    trig, items = np.empty(header[4] * 128, dtype=np.float64), np.empty(header[5] * 4, dtype=np.int32)
    _lib.call('shg_rot_level_tables', *args, ctypes.c_void_p(trig.ctypes.data), trig.size, items.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), items.size)
    return list(header), trig, items


@pytest.fixture(scope='module')
def quarter_degree():
    return ga.grid.GeographicGrid(0.25, 0.25)


def test_cutoffs_of_the_headline_plan(quarter_degree):
    g = quarter_degree
    lv = cutoffs(96, *tables(g.parallels, 96, 'ewh', g))
    assert len(lv) == 45                                          # 360 northern parallels in blocks of 8 (a pair of parallels shares its level)
    assert lv[:11] == DESIGN_LEVELS
    assert all(x == 96 for x in lv[11:])
    assert all(a <= b for a, b in zip(lv, lv[1:]))
    # the rule sees kn and the colatitudes only; mirrored parallels give the same levels in the same blocks
    assert cutoffs(96, *tables(g.parallels[::-1].copy(), 96, 'ewh', g)) == lv
    # levels end at 9, 19, ... or at N
    for N in (40, 12):
        lvn = cutoffs(N, *tables(g.parallels, N, 'ewh', g))
        assert all(x == N or (x + 1) % 10 == 0 for x in lvn) and all(a <= b for a, b in zip(lvn, lvn[1:]))
        assert (N == 12) == all(x == N for x in lvn), (N, lvn[:6])


def test_cutoffs_without_north_south_symmetry(quarter_degree):
    g = quarter_degree
    par = np.concatenate([g.parallels[:16], g.parallels[-16:]])
    sym = cutoffs(96, *tables(par, 96, 'ewh', g))
    assert sym == [39, 49]
    par[20] += 1e-6                                                 # blocks of 16 consecutive parallels instead of 8 pairs
    assert cutoffs(96, *tables(par, 96, 'ewh', g)) == [49, 49]


# ---- the unpruned kernel's tables from their rules

def order_class(R, m):
    rho = m % R
    r, sign = (rho, 1) if 2 * rho <= R else (R - rho, -1)
    if R % 2 == 0:
        return (0 if r == 0 else 1 if 2 * r == R else r + 1), sign
    return r, sign


def layout(R, top):
    nc = R // 2 + 1
    cnt = [0] * 6
    for m in range(1, top + 1):
        cnt[order_class(R, m)[0]] += 1
    nk = [(c + 3) // 4 for c in cnt]
    start = [4 * sum(nk[:c]) for c in range(nc)]
    slot, nxt = {}, list(start)
    for m in range(1, top + 1):
        c = order_class(R, m)[0]
        slot[m] = nxt[c]
        nxt[c] += 1
    slot[0] = 4 * sum(nk)
    return nk, cnt, slot


def trig_stream(R, top, lon):
    nlon = lon.size
    nd = nlon // (2 * R)
    nct = (nd + 15) // 16
    nk, _, slot = layout(R, top)
    npieces = sum(nk)
    by_slot = {s: m for m, s in slot.items() if m >= 1}
    tab = np.zeros((nct * npieces + 1) * 128)
    for ct in range(nct):
        for ks in range(npieces):
            for lane in range(64):
                m, c = by_slot.get(4 * ks + lane // 16), 16 * ct + lane % 16
                if m is None or c >= nd:
                    continue
                arg = float(m) * float(lon[nlon // 2 + c])
                tab[((ct * npieces + ks) * 64 + lane) * 2] = math.cos(arg)
                tab[((ct * npieces + ks) * 64 + lane) * 2 + 1] = order_class(R, m)[1] * math.sin(arg)
    return tab


def item_table(R, N, top, ns, waves=8):
    od = 16 if ns else 8
    qoff, q = [], 0
    for m in range(N + 1):
        qoff.append(q)
        q += (N + 1 - m + od - 1) // od
    slot = layout(R, top)[2]
    rec = [[] for _ in range(waves)]
    for m in range(top + 1):
        w = min(range(waves), key=lambda v: (len(rec[v]), v))
        cnt = N + 1 - m
        n_oct = (cnt + od - 1) // od
        for j0 in range(0, n_oct, 2):
            o0 = qoff[m] + j0
            rec[w].append([o0, o0 + (1 if j0 + 1 < n_oct else 0), slot[m], 1 | (2 if (j0 + 1) * od < cnt else 0) | (4 if j0 + 2 >= n_oct else 0)])
    ntrip = (max(len(r) for r in rec) + 3) // 4
    nrec = 4 * ntrip + 8
    table = np.zeros((waves, nrec, 4), dtype=np.int32)
    for w in range(waves):
        pad = rec[w][0][0] if rec[w] else 0
        table[w, :, 0:2] = pad
        if rec[w]:
            table[w, :len(rec[w])] = rec[w]
    return table.ravel(), nrec, ntrip


@pytest.mark.parametrize('R,N,ns', [(10, 96, True), (9, 96, True), (6, 40, False), (3, 12, True)])
def test_top_level_tables_are_the_unpruned_ones(quarter_degree, R, N, ns):
    lon = np.ascontiguousarray(quarter_degree.meridians, dtype=np.float64)
    header, trig, items = level_tables(R, N, N, ns, lon)
    nk, cnt, slot = layout(R, N)
    ref_items, nrec, ntrip = item_table(R, N, N, ns)
    ref_trig = trig_stream(R, N, lon)
    assert header[:6] == [sum(nk), slot[0], nrec, ntrip, ref_trig.size // 128, ref_items.size // 4]
    assert header[8:14] == nk and header[14:20] == cnt
    assert trig.tobytes() == ref_trig.tobytes()
    assert items.tobytes() == ref_items.tobytes()


def test_lower_levels_hold_the_front_of_the_order_sequence(quarter_degree):
    lon = np.ascontiguousarray(quarter_degree.meridians, dtype=np.float64)
    R, N = 10, 96
    full_slots = layout(R, N)[0]
    for level in (39, 49, 89):
        header, trig, items = level_tables(R, N, level, True, lon)
        nk, cnt, slot = layout(R, level)
        assert header[8:14] == nk and header[14:20] == cnt and header[1] == slot[0] == 4 * header[0]
        assert all(a <= b for a, b in zip(nk, full_slots)) and sum(cnt) == level
        assert trig.tobytes() == trig_stream(R, level, lon).tobytes()
        assert trig.size == (5 * header[0] + 1) * 128                 # five column tiles and the spare piece
        ref_items, nrec, ntrip = item_table(R, N, level, True)
        assert items.tobytes() == ref_items.tobytes() and header[2:4] == [nrec, ntrip]
        recs = items.reshape(8, nrec, 4)
        valid = recs[recs[:, :, 3] != 0]
        assert valid[:, 2].max() == header[1] and valid[:, 2].min() == 0      # panel slots within the level's panel, order 0 behind them
