"""
Caller-supplied plan tables around the north-south classification of shg_plan_create (grates_amd/csrc/plan.hip:
has_north_south_symmetry, has_fourfold_symmetry; synthesis_rot.hip: has_rotation_symmetry) as one table of named cases, shared by
tests/test_plan_symmetry_cpu.py (the classification restated in plain Python and the sensitivity of every case, no GPU) and
tests/test_gpu_plan_symmetry.py (every case run on the device).  NumPy and the CPU oracle only, seeded.

A grid with an even number of parallels falls into one of three classes:
  rejected              a mirror pair deviates by more than 1e-11 rad in colatitude or 1e-10 relative in a kn entry: plain kernels
  accepted and flagged  above 1e-13 / (N + 1) rad or 5e-14 relative in kn: every 8-row block of northern parallels that holds such
                        a row gets a second table for its mirrored rows (a second pass of the fused kernels)
  accepted and shared   the southern rows are (-1)^(n-m) times the northern table

Every case starts from a natural grid (orc.geographic_grid with orc.kn_table of the potential kernel) whose southern half is
replaced by the EXACT mirror of the northern half (colat[nlat-1-i] = fl(pi - colat[i]): the sum of a pair is pi or pi + 1 ulp,
4.4e-16 (N + 1) < 1e-13 for every degree here; kn[nlat-1-i] = kn[i]), and then moves the mirrors of some northern rows:
  accepted moves     colatitude by +-(4 .. 8)e-12 rad, kn by a factor 1 +- (6 .. 8)e-11 (one sign per row, so that the move shows
                     in the row's values and does not average out over the degrees)
  boundary moves     as named in the case
`tables(name)` gives (N, colat, kn, lon, expect); expect holds
  north_south        the plan accepts the grid as symmetric about the equator
  flagged            the set of northern rows that the plan must flag (= the rows whose mirror was moved by an accepted amount)
  shortcut_visible   evaluating the southern rows from the northern rows' geometry misses the truth by more than 50 x 1e-12
  fourfold           the meridians have the 4-fold symmetry
  rotations          the rotation count of the plan's own choice (0: the rotation-folded kernel does not apply)
  counts             every rotation count that the rotation-folded kernel can run with on this plan
  paths              the paths that shg_plan_set_path accepts
`mirrored(name)` gives the exactly mirrored (colat, kn) the case was moved from, `area(name)` the grid's area weights.

The expectations of SHAPES are written out by hand:
  K slots of the 4-fold longitude stage = sum of the four order groups {N/2+1, (N+1)/2, N/2, (N+1)/2} rounded up to 16
    d/o 9, 17: 64   d/o 45: 128   d/o 96: 64 + 3 * 48 = 208   d/o 126: 4 * 64 = 256   d/o 140: 4 * 80 = 320
  fused (64-row panel, 80 doubles a slot): K <= 256;  fused32 (48 doubles a slot, needs the north-south symmetry): K <= 426
  rotation counts R in {10, 9, 6, 3} (preferred in this order): nlon >= 192, nlon % 2R == 0, (nlon / R) % 16 == 0
    1440: 10, 9, 6, 3    192: 6, 3    240: 3    180, 90: none
  and a panel of at most 111 slots (49152 bytes of rings + 1024 (slots + 1) <= 160 KiB); slots = sum over the classes
  min(m mod R, R - m mod R) of the orders 1 .. N, each class rounded up to 4:  d/o 126, R = 3: 44 + 84 = 128 slots: does not fit.
"""

import numpy as np

from oracle import shg_oracle as orc

GM, R_EARTH = orc.GM_DEFAULT, orc.R_DEFAULT

ALL_PATHS = ('auto', 'fused', 'fused32', 'rot', 'staged')

# name: (N, dlon, dlat, nlon, nlat, fourfold, rotation counts (preferred first), paths on an accepted grid)
SHAPES = {
    'n96_1440x36': (96, 0.25, 5.0, 1440, 36, True, (10, 9, 6, 3), ('auto', 'fused', 'fused32', 'rot', 'staged')),
    'n45_192x90': (45, 1.875, 2.0, 192, 90, True, (6, 3), ('auto', 'fused', 'fused32', 'rot', 'staged')),      # nh = 45: ragged last block
    'n17_240x18': (17, 1.5, 10.0, 240, 18, True, (3,), ('auto', 'fused', 'fused32', 'rot', 'staged')),          # nh = 9: one block and one row
    'n126_240x120': (126, 1.5, 1.5, 240, 120, True, (), ('auto', 'fused', 'fused32', 'staged')),                # K = 256: the slot limit of fused
    'n140_180x90': (140, 2.0, 2.0, 180, 90, True, (), ('auto', 'fused32', 'staged')),                           # K = 320: the 32-row kernel only
    'n9_1440x2': (9, 0.25, 90.0, 1440, 2, True, (10, 9, 6, 3), ('auto', 'fused', 'fused32', 'rot', 'staged')),  # nh = 1
    'n33_90x36': (33, 4.0, 5.0, 90, 36, False, (), ('auto', 'staged')),                                         # nlon % 4 != 0: staged, the control
    'n45_192x45': (45, 1.875, 4.0, 192, 45, True, (6, 3), ('auto', 'fused', 'fused32', 'rot', 'staged')),      # odd number of parallels
}

CASES = {}


def case(name, shape, rows='none', move=(), seed=0, boundary=None, meridians=None):
    """rows: pattern of the northern rows whose mirrors move (row_pattern); move: subset of ('colat', 'kn') for the accepted
    moves; boundary: name of a class-boundary move instead; meridians: largest move of a meridian in rad."""
    assert name not in CASES and shape in SHAPES
    CASES[name] = dict(name=name, shape=shape, rows=rows, move=tuple(move), seed=seed, boundary=boundary, meridians=meridians)


def row_pattern(pattern, nh):
    """The northern rows of a pattern; blocks are the 8-row blocks counted from the north pole, the last one may be ragged."""
    nblocks = -(-nh // 8)
    block = lambda b: list(range(8 * b, min(8 * b + 8, nh)))
    if pattern == 'none':
        return []
    if pattern == 'all':
        return list(range(nh))
    if pattern == 'single':                      # one row in the middle of a block that is not the first
        return [min(8 * (nblocks // 2) + 3, nh - 1)]
    if pattern == 'first_block':
        return block(0)
    if pattern == 'last_block':
        return block(nblocks - 1)
    if pattern == 'blocks_0_3_last':             # ranks 0, 1, 2 at blocks that are not neighbours; block 3 with two rows of its second
        assert nblocks >= 6                      # half only (one 4-row group of the 32-row kernel's own map), the last with its last row
        return block(0) + [29, 30] + [nh - 1]
    if pattern == 'every_other':
        return [i for b in range(0, nblocks, 2) for i in block(b)]
    raise ValueError(pattern)


def natural(shape):
    """(N, colat, kn, lon, area) of the shape's grid with the southern half replaced by the exact mirror of the northern half."""
    N, dlon, dlat, nlon, nlat = SHAPES[shape][0:5]
    lon, parallels, area = orc.geographic_grid(dlon, dlat)
    assert lon.size == nlon and parallels.size == nlat
    colat, _, kn = orc.kn_table(orc.KernelTable('potential'), N, parallels, GM, R_EARTH)
    colat, kn = colat.copy(), kn.copy()
    for i in range(nlat // 2):
        colat[nlat - 1 - i] = np.pi - colat[i]
        kn[nlat - 1 - i] = kn[i]
    return N, colat, kn, lon, area


def mirrored(name):
    _, colat, kn, _, _ = natural(CASES[name]['shape'])
    return colat, kn


def area(name):
    return natural(CASES[name]['shape'])[4]


def tables(name):
    c = CASES[name]
    N, colat, kn, lon, _ = natural(c['shape'])
    _, _, _, nlon, nlat, fourfold, counts, paths = SHAPES[c['shape']]
    nh = nlat // 2
    rng = np.random.default_rng(c['seed'])
    north_south, flagged = nlat % 2 == 0, set()
    rows = row_pattern(c['rows'], nh)
    if c['boundary'] is None:
        for i in rows:
            mi = nlat - 1 - i
            if 'colat' in c['move']:
                colat[mi] += rng.choice((-1.0, 1.0)) * rng.uniform(4e-12, 8e-12)
            if 'kn' in c['move']:
                kn[mi] *= 1.0 + rng.choice((-1.0, 1.0)) * rng.uniform(6e-11, 8e-11, N + 1)
        if c['move']:
            flagged = set(rows)
    elif c['boundary'] == 'kn_4e-14':            # accepted and shared: below 5e-14 relative in kn, colatitudes untouched
        for i in rows:
            kn[nlat - 1 - i] *= 1.0 + rng.uniform(-4e-14, 4e-14, N + 1)
    elif c['boundary'] == 'colat_2e-11':         # one pair beyond 1e-11 rad
        colat[nlat - 1 - rows[0]] += 2e-11
        north_south = False
    elif c['boundary'] == 'kn_entry_2e-10':      # one entry of one row beyond 1e-10 relative
        kn[nlat - 1 - rows[0], N // 2] *= 1.0 + 2e-10
        north_south = False
    elif c['boundary'] == 'kn_scaled':           # hemisphere-dependent degree factors on exactly mirrored colatitudes
        kn[nlat - nh:] *= 1.0 + 1e-3 * np.arange(N + 1)
        north_south = False
    elif c['boundary'] == 'odd':
        assert nlat % 2 == 1
    else:
        raise ValueError(c['boundary'])
    if c['meridians'] is not None:
        lon = lon + rng.uniform(-c['meridians'], c['meridians'], nlon)
        if c['meridians'] > 1e-15:               # both meridian tests bound a pair of meridians at 3e-15 rad
            fourfold, counts = False, ()
    if not fourfold:
        paths = ('auto', 'staged')
    if not north_south:
        paths = tuple(p for p in paths if p != 'fused32')
    if not counts:
        paths = tuple(p for p in paths if p != 'rot')
    expect = dict(north_south=north_south, flagged=flagged, shortcut_visible=bool(flagged), fourfold=fourfold,
                  rotations=counts[0] if counts else 0, counts=tuple(counts), paths=paths)
    return N, colat, kn, lon, expect


# ---- flag patterns with an accepted deviation (d/o 45 on 192 x 90: nh = 45, blocks 0 .. 5, the last with 5 rows) -----------------------
for k, pattern in enumerate(('none', 'single', 'first_block', 'last_block', 'blocks_0_3_last', 'every_other', 'all')):
    case('n45_both_' + pattern, 'n45_192x90', pattern, ('colat', 'kn'), seed=100 + k)
case('n45_colat_blocks_0_3_last', 'n45_192x90', 'blocks_0_3_last', ('colat',), seed=110)
case('n45_kn_all', 'n45_192x90', 'all', ('kn',), seed=111)
# ---- shapes that reach every consumer --------------------------------------------------------------------------------------------------
case('n96_both_all', 'n96_1440x36', 'all', ('colat', 'kn'), seed=120)                    # rotation counts 10, 9, 6, 3; fused; fused32
case('n96_both_last_block', 'n96_1440x36', 'last_block', ('colat', 'kn'), seed=121)      # rows 16, 17
case('n96_colat_single', 'n96_1440x36', 'single', ('colat',), seed=122)                  # row 11
case('n17_both_all', 'n17_240x18', 'all', ('colat', 'kn'), seed=130)
case('n17_both_last_block', 'n17_240x18', 'last_block', ('colat', 'kn'), seed=131)       # row 8 alone
case('n126_both_blocks_0_3_last', 'n126_240x120', 'blocks_0_3_last', ('colat', 'kn'), seed=140)
case('n126_both_all', 'n126_240x120', 'all', ('colat', 'kn'), seed=141)
case('n140_both_blocks_0_3_last', 'n140_180x90', 'blocks_0_3_last', ('colat', 'kn'), seed=150)
case('n140_both_every_other', 'n140_180x90', 'every_other', ('colat', 'kn'), seed=151)
case('n9_both_all', 'n9_1440x2', 'all', ('colat', 'kn'), seed=160)
case('n33_both_all', 'n33_90x36', 'all', ('colat', 'kn'), seed=170)
# ---- class boundaries ---------------------------------------------------------------------------------------------------------------
case('n45_kn_4e-14', 'n45_192x90', 'all', boundary='kn_4e-14', seed=200)
case('n126_kn_4e-14', 'n126_240x120', 'all', boundary='kn_4e-14', seed=201)
case('n45_colat_2e-11', 'n45_192x90', 'single', boundary='colat_2e-11', seed=202)
case('n45_kn_entry_2e-10', 'n45_192x90', 'single', boundary='kn_entry_2e-10', seed=203)
case('n45_kn_scaled', 'n45_192x90', boundary='kn_scaled', seed=204)
case('n96_kn_scaled', 'n96_1440x36', boundary='kn_scaled', seed=205)
case('n140_kn_scaled', 'n140_180x90', boundary='kn_scaled', seed=206)
case('n45_odd', 'n45_192x45', boundary='odd', seed=207)
# ---- meridians ------------------------------------------------------------------------------------------------------------------------
case('n45_lon_1e-15', 'n45_192x90', meridians=1e-15, seed=300)
case('n45_lon_1e-14', 'n45_192x90', meridians=1e-14, seed=301)
case('n96_lon_1e-15', 'n96_1440x36', meridians=1e-15, seed=302)
case('n96_lon_1e-14', 'n96_1440x36', meridians=1e-14, seed=303)

ACCEPTED_FLAGGED = tuple(n for n, c in CASES.items() if c['boundary'] is None and c['move'] and c['rows'] != 'none')
REJECTED = tuple(n for n, c in CASES.items() if c['boundary'] in ('colat_2e-11', 'kn_entry_2e-10', 'kn_scaled', 'odd'))
UNFLAGGED_BOUNDARY = tuple(n for n, c in CASES.items() if c['boundary'] == 'kn_4e-14')
MERIDIANS = tuple(n for n, c in CASES.items() if c['meridians'] is not None)
