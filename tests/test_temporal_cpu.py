"""
Time-variable parameters on the host (lstsq.TemporalParameters, lstsq.temporal_blocks, engine.check_window_runs): the constructors
against the expressions they restate, bit for bit; every ValueError, with no GPU present; and the block and slot planner against a
point-by-point enumeration of all short sequences of window starts.
"""
import datetime
import itertools

import numpy as np
import pytest

import points_at_inputs as pi
import temporal_inputs as ti
import whitening_inputs as wi

import grates_amd as ga

ls = ga.lstsq


# ---- 1: constructor bits -------------------------------------------------------------------------------------------------------------
def test_linear_reproduces_the_interpolation_windows():
    series = pi.constituents('series60')[0]
    nodes = pi.series_epochs()
    as_datetimes = pi.epochs('series60')
    as_mjd = np.array([pi.mjd(epoch) for epoch in as_datetimes])
    for epochs, node_forms in ((as_datetimes, (nodes,)), (as_mjd, (nodes, np.array([pi.mjd(epoch) for epoch in nodes])))):
        first, weights = series.interpolation_windows(epochs)
        for form in node_forms:
            temporal = ls.TemporalParameters.linear(form, epochs)
            assert temporal.field_count == pi.SERIES_FIELDS and temporal.factors.shape == (len(epochs), 2)
            assert temporal.first.dtype == np.int64 and np.array_equal(temporal.first, first)
            assert temporal.factors.dtype == np.float64 and np.array_equal(temporal.factors, weights)
    assert np.array_equal(first[:5], [7, 0, 2, 4, 1])                  # MJD: the last node, the first, two interior nodes, a node again
    mixed = ls.TemporalParameters.linear(np.array([pi.mjd(epoch) for epoch in nodes]), as_datetimes)      # datetimes against MJD nodes
    assert np.array_equal(mixed.first, first) and np.array_equal(mixed.factors, weights)


def test_harmonic_reproduces_trend_and_oscillation():
    gf = pi.field(np.zeros((3, 3)))
    trend = ga.gravityfield.Trend(gf, pi.REFERENCE_EPOCH)
    cycles = [ga.gravityfield.Oscillation(gf, gf, period, pi.REFERENCE_EPOCH) for period in pi.PERIODS]
    as_datetimes = pi.epochs('model31')
    as_mjd = np.array([pi.mjd(epoch) for epoch in as_datetimes])
    for epochs in (as_datetimes, as_mjd):
        temporal = ls.TemporalParameters.harmonic(epochs, pi.REFERENCE_EPOCH, periods=pi.PERIODS)
        assert temporal.field_count == 6 and temporal.factors.shape == (len(epochs), 6) and not temporal.first.any()
        assert np.array_equal(temporal.factors[:, 0], np.ones(len(epochs)))
        assert np.array_equal(temporal.factors[:, 1:2], trend.weights_at(epochs))
        assert np.array_equal(temporal.factors[:, 2:4], cycles[0].weights_at(epochs))
        assert np.array_equal(temporal.factors[:, 4:6], cycles[1].weights_at(epochs))
        bare = ls.TemporalParameters.harmonic(epochs, pi.REFERENCE_EPOCH, periods=pi.PERIODS[1:], trend=False, static=False)
        assert bare.field_count == 2 and np.array_equal(bare.factors, cycles[1].weights_at(epochs))
        decade = ls.TemporalParameters.harmonic(epochs, pi.REFERENCE_EPOCH, static=False, time_scale=3652.5)
        assert np.array_equal(decade.factors, ga.gravityfield.Trend(gf, pi.REFERENCE_EPOCH, 3652.5).weights_at(epochs))


def test_constant_against_a_loop():
    edges = np.array([10.0, 11.0, 11.5, 14.0])
    rng = np.random.default_rng(3401)
    epochs = np.concatenate(([10.0, 11.0, 11.5, np.nextafter(14.0, 0.0), np.nextafter(11.0, 0.0)], rng.uniform(10.0, 14.0, 40)))
    expected = np.array([max(k for k in range(3) if edges[k] <= t) for t in epochs])
    assert all(edges[k] <= t < edges[k + 1] for k, t in zip(expected, epochs))
    temporal = ls.TemporalParameters.constant(edges, epochs)
    assert temporal.field_count == 3 and np.array_equal(temporal.first, expected) and np.array_equal(temporal.factors, np.ones((45, 1)))
    assert list(temporal.first[:5]) == [0, 1, 2, 2, 0]                 # an epoch on an edge belongs to the interval that starts there
    start = datetime.datetime(2010, 1, 1)
    stamps = [start + datetime.timedelta(days=k) for k in (0, 1, 3)]
    times = [start, start + datetime.timedelta(days=1), start + datetime.timedelta(days=1) - datetime.timedelta(microseconds=1),
             start + datetime.timedelta(days=2, hours=23)]
    assert list(ls.TemporalParameters.constant(stamps, times).first) == [0, 1, 0, 1]
    assert list(ls.TemporalParameters.constant(stamps, np.array([pi.mjd(t) for t in times[:2]])).first) == [0, 1]


def test_fields_reshapes_the_solution():
    temporal = ls.TemporalParameters(np.zeros(3, dtype=int), np.ones((3, 2)), 4)
    x = np.arange(20.0)
    assert np.array_equal(temporal.fields(x), x.reshape(4, 5)) and np.array_equal(temporal.fields(x[:, None]), x.reshape(4, 5))
    with pytest.raises(ValueError, match='B = 4'):
        temporal.fields(np.zeros(21))


# ---- 2: error paths --------------------------------------------------------------------------------------------------------------------
def _raises(match, function, *args, **kwargs):
    with pytest.raises(ValueError, match=match):
        function(*args, **kwargs)


def test_constructor_errors():
    first, factors = np.zeros(5, dtype=np.int64), np.ones((5, 2))
    _raises('shape \\(M, W\\)', ls.TemporalParameters, first, np.ones(5), 3)
    _raises('window of 17 fields', ls.TemporalParameters, first, np.ones((5, 17)), 20)
    _raises('window of 0 fields', ls.TemporalParameters, first, np.ones((5, 0)), 3)
    _raises('integer array of shape \\(5,\\)', ls.TemporalParameters, first[:4], factors, 3)
    _raises('integer array of shape \\(5,\\)', ls.TemporalParameters, first.astype(float), factors, 3)
    _raises('only 1 fields', ls.TemporalParameters, first, factors, 1)
    _raises('fields must be an integer', ls.TemporalParameters, first, factors, 2.5)
    _raises('first\\[3\\] is 2, outside 0 .. 1', ls.TemporalParameters, np.array([0, 1, 0, 2, 0]), factors, 3)
    _raises('first\\[1\\] is -1', ls.TemporalParameters, np.array([0, -1, 0, 0, 0]), factors, 3)
    for bad in (np.nan, np.inf):
        spoiled = factors.copy()
        spoiled[2, 1] = bad
        _raises('factors must be finite', ls.TemporalParameters, first, spoiled, 3)
    _raises('model must be None', ls.TemporalParameters, first, factors, 3, model='white')
    arcs = ls.ArcParameters(ls.arc_basis(None, 5, degree=0))
    _raises('arc elimination under temporal parameters is not built yet', ls.TemporalParameters, first, factors, 3, model=arcs)
    _raises('not built yet', ls.TemporalParameters.linear, np.array([0.0, 1.0]), np.array([0.5]), model=arcs)
    signed = ls.TemporalParameters(first, -factors, 2)                 # signed factors are legal
    assert signed.field_count == 2 and signed.model is None


def test_epoch_errors():
    nodes = np.array([1.0, 2.0, 3.0])
    _raises('epoch 1 \\(MJD 3.5\\) lies outside the series', ls.TemporalParameters.linear, nodes, np.array([1.0, 3.5]))
    _raises('epoch 0 .* lies outside the series', ls.TemporalParameters.linear, pi.series_epochs(), [pi.SERIES_START - datetime.timedelta(seconds=1)])
    _raises('at least two data points', ls.TemporalParameters.linear, nodes[:1], np.array([1.0]))
    _raises('nodes must ascend strictly', ls.TemporalParameters.linear, np.array([1.0, 1.0, 2.0]), np.array([1.0]))
    _raises('not finite', ls.TemporalParameters.linear, nodes, np.array([np.nan]))
    _raises('float64 array', ls.TemporalParameters.linear, nodes, np.array([1, 2]))
    _raises('epoch 2 \\(MJD 3.0\\) lies outside the edges', ls.TemporalParameters.constant, nodes, np.array([1.0, 2.5, 3.0]))       # half-open: e_B is outside
    _raises('epoch 0 .* lies outside the edges', ls.TemporalParameters.constant, nodes, np.array([0.5]))
    _raises('at least two and ascend strictly', ls.TemporalParameters.constant, nodes[:1], np.array([1.0]))
    _raises('at least two and ascend strictly', ls.TemporalParameters.constant, nodes[::-1].copy(), np.array([1.0]))
    _raises('no column at all', ls.TemporalParameters.harmonic, nodes, pi.REFERENCE_EPOCH, trend=False, static=False)
    _raises('finite and positive', ls.TemporalParameters.harmonic, nodes, pi.REFERENCE_EPOCH, periods=(0.0,))
    _raises('finite and positive', ls.TemporalParameters.harmonic, nodes, pi.REFERENCE_EPOCH, time_scale=np.inf)
    _raises('window of 18 fields', ls.TemporalParameters.harmonic, nodes, pi.REFERENCE_EPOCH, periods=tuple(range(1, 9)))
    _raises('reference_epoch must be a datetime', ls.TemporalParameters.harmonic, nodes, 51544.0)


def test_call_errors_come_before_the_device():
    """every check of a from_* or of_* call runs on the host: the errors below are raised with no GPU present"""
    xyz = ti.positions()[:6]
    g = np.zeros((6, 3))
    temporal = ls.TemporalParameters.linear(np.array([0.0, 1.0, 2.0]), np.linspace(0.0, 2.0, 6))
    _raises('5 positions but 6 accelerations', temporal.from_accelerations, xyz[:5], g, 2, 4)
    _raises('5 points but the temporal parameters hold the windows of 6', temporal.from_accelerations, xyz[:5], g[:5], 2, 4)
    _raises('block_points must be positive', temporal.from_accelerations, xyz, g, 2, 4, block_points=0)
    _raises('solution must have shape \\(63,\\)', temporal.of_accelerations, np.zeros(21), xyz, g, 2, 4)
    _raises('vectors must have shape \\(63, S\\)', temporal.of_accelerations, np.zeros(63), xyz, g, 2, 4, vectors=np.zeros((21, 2)))
    _raises('7 points but the temporal parameters', temporal.from_potentials, ti.positions()[:7], np.zeros(7), 2, 4)
    model = wi.synthetic_sequence(ls, 3, 3411)
    jumps = ls.TemporalParameters(np.array([0, 16, 0, 16, 0, 16]), np.ones((6, 1)), 17, model=ls.ColouredNoise(model))
    _raises('point 1 and its history of 1 points span 17 fields', jumps.from_accelerations, xyz, g, 2, 4)
    _raises('arcs must start at 0', ls.TemporalParameters(np.zeros(6, dtype=int), np.ones((6, 1)), 1, model=ls.ColouredNoise(model, [1, 3])).from_accelerations,
            xyz, g, 2, 4)
    design = np.zeros((18, 21))
    _raises('first\\[0\\] is 5', ga.gravityfield.temporal_design_matrix, design, np.full(6, 5), np.ones((6, 2)), 4)
    _raises('design must have shape \\(K M, P\\) with M = 6', ga.gravityfield.temporal_design_matrix, design[:17], np.zeros(6, dtype=int), np.ones((6, 2)), 4)


def test_window_run_tables_are_checked_on_the_host():
    check = ga.engine.check_window_runs
    slot, begin = check([0, 1], [0, 2, 5], 5, 2, 3)
    assert slot.dtype == np.int32 and begin.dtype == np.int32 and list(slot) == [0, 1] and list(begin) == [0, 2, 5]
    _raises('1 <= W <= E <= 16', check, [0], [0, 5], 5, 3, 2)
    _raises('1 <= W <= E <= 16', check, [0], [0, 5], 5, 1, 17)
    _raises('1 <= W <= E <= 16', check, [0], [0, 5], 5, 0, 2)
    _raises('ascend strictly from 0 to the 5 columns', check, [0, 0], [0, 2, 4], 5, 1, 1)
    _raises('ascend strictly', check, [0, 0], [0, 3, 3], 3, 1, 1)
    _raises('ascend strictly', check, [0, 0], [1, 3, 5], 5, 1, 1)
    _raises('ascend strictly', check, np.zeros(0, dtype=int), [0], 5, 1, 1)
    _raises('slot 2, outside 0 .. E - W = 1', check, [0, 2], [0, 2, 5], 5, 2, 3)
    _raises('slot -1', check, [-1], [0, 5], 5, 2, 3)
    _raises('integer arrays', check, [0.0], [0, 5], 5, 1, 1)
    _raises('integer arrays', check, [0, 0], [0, 5], 5, 1, 1)


def test_library_checks_the_run_tables_before_any_hip_call():
    """shg_window_expand itself refuses bad sizes and bad run tables, with no GPU present"""
    import ctypes
    from grates_amd import _lib

    def call(rows, n, slot, begin, W, E, lds=None, slot_stride=None, pointer=0x1000):
        slot, begin = np.asarray(slot, dtype=np.int32), np.asarray(begin, dtype=np.int32)
        lds = n if lds is None else lds
        with pytest.raises(_lib.ShgError) as err:
            _lib.call('shg_window_expand', rows, n, ctypes.c_void_p(pointer), n, ctypes.c_void_p(slot.ctypes.data), ctypes.c_void_p(begin.ctypes.data),
                      len(slot), ctypes.c_void_p(0x100000), W, E, ctypes.c_void_p(0x200000), lds, rows * lds if slot_stride is None else slot_stride, None)
        return str(err.value)
    assert 'window of 17 fields' in call(2, 4, [0], [0, 4], 17, 17)
    assert '1 slots, expected W = 2 .. 16' in call(2, 4, [0], [0, 4], 2, 1)
    assert 'lds 3 below n 4' in call(2, 4, [0], [0, 4], 1, 1, lds=3)
    assert 'slot_stride 7 below the 8 values' in call(2, 4, [0], [0, 4], 1, 2, slot_stride=7)
    assert 'run_begin[0] is 1' in call(2, 4, [0], [1, 4], 1, 1)
    assert 'run_begin must increase strictly' in call(2, 4, [0, 0], [0, 2, 2], 1, 1)
    assert 'run_begin must increase strictly' in call(2, 4, [0, 0], [0, 2, 5], 1, 1)
    assert 'the runs end at column 3' in call(2, 4, [0, 0], [0, 2, 3], 1, 1)
    assert 'starts at slot 2, outside 0 .. E - W = 1' in call(2, 4, [0, 2], [0, 2, 4], 2, 3)
    assert 'starts at slot -1' in call(2, 4, [-1], [0, 4], 1, 1)
    assert 'NULL pointer' in call(2, 4, [0], [0, 4], 1, 1, pointer=0)
    assert 'overlap' in call(2, 4, [0], [0, 4], 1, 1, pointer=0x200008)


# ---- 3: the block and slot planner -----------------------------------------------------------------------------------------------------
def _check_plan(first, W, block_points, stage):
    first = np.asarray(first)
    blocks = ls.temporal_blocks(first, W, block_points, stage)
    expected = ti.enumerate_blocks(first, W, block_points, stage)
    assert [(b.start, b.first, b.last, b.field, b.slots) for b in blocks] == expected
    owned = np.zeros(len(first), dtype=int)
    for block in blocks:
        assert block.slots <= ti.MAX_SLOTS and block.last - block.first <= block_points
        owned[block.first:block.last] += 1
        n = block.last - block.start
        slot = np.repeat(block.run_slot, np.diff(block.run_begin))
        assert block.run_begin[0] == 0 and block.run_begin[-1] == n and np.all(np.diff(block.run_begin) > 0)
        assert np.array_equal(slot + block.field, first[block.start:block.last])          # every (point, field of its window) has its slot
        assert slot.min() == 0 and slot.max() + W == block.slots
        assert np.all(block.run_slot[1:] != block.run_slot[:-1])
        for e in range(block.slots):
            columns = ti.enumerate_support(first, W, stage, block.first, block.last, block.field, e)
            assert block.supports[e] == ((columns[0], columns[-1] + 1) if columns else None), (first, W, block_points, stage, e)
    assert np.all(owned == 1)                                                               # every point in exactly one block
    return blocks


@pytest.mark.parametrize('W', [pytest.param(1, marks=pytest.mark.slow), 2, 3])
def test_planner_against_the_enumeration(W):
    """all sequences of window starts of up to 7 points over 4 fields; the block size and the arcs change from one to the next
    (W = 1: 21 845 sequences, half a minute of host time)"""
    sizes, arcs, index = (1, 2, 3, 7), ([0], [0, 3], [0, 1, 5]), 0
    for length in range(1, 8):
        for first in itertools.product(range(4 - W + 1), repeat=length):
            index += 1
            block_points = sizes[index % 4]
            starts = [a for a in arcs[(index // 4) % 3] if a < length]
            for q in (0, 1, 3):
                _check_plan(first, W, block_points, ti.stages(starts, length, q))
            if all(a <= b for a, b in zip(first[:-1], first[1:])):                        # no noise model: sorted points only
                blocks = _check_plan(first, W, block_points, None)
                assert all(b.slots == W and b.start == b.first and b.supports == [(0, b.last - b.first)] * W for b in blocks)
    assert index == sum((4 - W + 1) ** length for length in range(1, 8))


def test_planner_cuts_at_sixteen_slots():
    first = np.array([0, 3, 6, 9, 12, 14, 15, 30, 30, 31, 20])
    stage = ti.stages([0, 7], len(first), 3)
    blocks = _check_plan(first, 2, 100, stage)
    assert [(b.first, b.last, b.field, b.slots) for b in blocks] == [(0, 6, 0, 16), (6, 7, 9, 8), (7, 11, 20, 13)]
    with pytest.raises(ValueError, match='point 8 and its history of 1 points span 17 fields'):
        ls.temporal_blocks([0, 0, 0, 0, 0, 0, 0, 0, 16], 1, 4, ti.stages([0], 9, 1))
    with pytest.raises(ValueError, match='must not decrease'):
        ls.temporal_blocks([1, 0], 1, 4)
    _check_plan(np.array([0, 16, 32, 32, 64]), 16, 2, None)                                # sorted runs may lie any distance apart


def test_pattern_of_the_plan():
    first = np.array([0, 0, 1, 1, 1, 3, 3])
    white = ls.temporal_pattern(ls.temporal_blocks(first, 2, 2))
    assert white == {(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (3, 3), (3, 4), (4, 4)}
    one_arc = ls.temporal_pattern(ls.temporal_blocks(first, 2, 2, ti.stages([0], 7, 1)))
    assert one_arc == white | {(0, 2), (1, 3), (1, 4), (2, 3), (2, 4)}                   # a point of history couples neighbouring runs
    cut = ls.temporal_pattern(ls.temporal_blocks(first, 2, 2, ti.stages([0, 5], 7, 1)))
    assert cut == white | {(0, 2)}                                                         # nothing crosses the arc that starts at point 5


def test_default_block_points():
    default = ls.TemporalParameters.default_block_points
    assert default(1677, 3, 2) == 3328 and default(1677, 3, 1) == ls.NormalEquations.default_block_points(1677, 3)
    assert default(77, 3, 2) * 8 * 3 * 77 * 2 <= ls.NormalEquations.DESIGN_BLOCK_BYTES < (default(77, 3, 2) + 256) * 8 * 3 * 77 * 2
    assert default(10 ** 6, 3, 16) == 256
