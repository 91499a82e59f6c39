"""Seeded inputs of the fixture of the point functionals at epochs (tests/golden/make_golden_points_at.py -> g32_points_at.npz) and
of the tests that replay it.  Positions, epochs and reference values are stored in the fixture; the fields are rebuilt from the
numbers below (acceleration_inputs.coefficients)."""

import datetime

import numpy as np

import acceleration_inputs as ai

GM, R = ai.GM, ai.R
SERIES_START = datetime.datetime(2008, 1, 1)
SERIES_STEP = datetime.timedelta(hours=3)
SERIES_FIELDS = 9
REFERENCE_EPOCH = datetime.datetime(2005, 1, 1)                  # of the trend and the cycles
PERIODS = (365.25, 182.625)                                      # annual and semi-annual cycle [days]
SCATTERED = 47                                                   # positions beside acceleration_inputs.special_positions()

# tag: (max degree, seed, with trend and cycles)
CASES = {
    'series60': (60, 3201, False),
    'model31': (31, 3202, True),
}


def series_epochs():
    return [SERIES_START + k * SERIES_STEP for k in range(SERIES_FIELDS)]


def series_coefficients(tag):
    """anm [9, N+1, N+1] of the series: 'static' fields of consecutive seeds (field 0 included)"""
    N, seed, _ = CASES[tag]
    return np.stack([ai.coefficients(N, 'static', seed + k) for k in range(SERIES_FIELDS)])


def model_coefficients(tag):
    """anm [5, N+1, N+1] of the 'anomaly' trend, annual cosine and sine, semi-annual cosine and sine"""
    N, seed, _ = CASES[tag]
    return np.stack([ai.coefficients(N, 'anomaly', seed + 100 + k) for k in range(5)])


def positions(tag):
    _, seed, _ = CASES[tag]
    return np.vstack((ai.special_positions(), ai.scattered_positions(SCATTERED, seed + 1000)))


def epochs(tag):
    """one epoch per position, unsorted: the last and the first node, two interior nodes, 5 microseconds behind a node, then whole
    seconds scattered over the series"""
    _, seed, _ = CASES[tag]
    nodes = series_epochs()
    fixed = [nodes[-1], nodes[0], nodes[3], nodes[5], nodes[2] + datetime.timedelta(microseconds=5)]
    count = ai.special_positions().shape[0] + SCATTERED - len(fixed)
    span = int((nodes[-1] - nodes[0]).total_seconds())
    seconds = np.random.default_rng(seed + 2000).integers(0, span + 1, count)
    return fixed + [nodes[0] + datetime.timedelta(seconds=int(s)) for s in seconds]


def mjd(epoch):
    """modified Julian date in the convention of grates_amd.utilities._mjd: whole days + seconds / 86400, microseconds dropped"""
    delta = epoch - datetime.datetime(1858, 11, 17)
    return delta.days + delta.seconds / 86400.0


def field(anm, epoch=None, module=None):
    """PotentialCoefficients of `module`.gravityfield (default: grates_amd) with the coefficients anm"""
    if module is None:
        import grates_amd as module
    gf = module.gravityfield.PotentialCoefficients(GM, R)
    gf.anm = anm.copy()
    gf.epoch = epoch
    return gf


def constituents(tag, module=None):
    """the constituents of the case with the classes of `module`.gravityfield: [TimeSeries] or [Trend, Oscillation (annual),
    Oscillation (semi-annual), TimeSeries]"""
    if module is None:
        import grates_amd as module
    gfm = module.gravityfield
    series = gfm.TimeSeries([field(anm, epoch, module) for anm, epoch in zip(series_coefficients(tag), series_epochs())])
    if not CASES[tag][2]:
        return [series]
    m = [field(anm, None, module) for anm in model_coefficients(tag)]
    return [gfm.Trend(m[0], REFERENCE_EPOCH), gfm.Oscillation(m[1], m[2], PERIODS[0], REFERENCE_EPOCH),
            gfm.Oscillation(m[3], m[4], PERIODS[1], REFERENCE_EPOCH), series]
