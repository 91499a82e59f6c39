"""
Time-variable gravity fields as sums of constituents (drop-in names of grates/gravityfield.py:784-812, 1054-1140: `Trend`,
`Oscillation`, `TimeVariableGravityField`).  Host-side containers: a constituent is anything with `evaluate_at(epoch)`; the device
work happens where the evaluated fields are used (`gravityfield.gridded_rms`, batched synthesis).

Every constituent here is a weighted sum of fixed fields, V(t) = sum_i w_i(tau) V_i with tau the time since the reference epoch
in the constituent's own unit -- `Trend` has one term with w = tau, `Oscillation` two with w = (cos, sin)(2 pi tau).

The point functionals are linear in the coefficients, so along an orbit, point i at its own epoch t_i, the same weights blend the
values of the fixed fields: the `*_at(xyz, epochs)` methods (gravityfield._FunctionalsAtEpochs) compute the weights of all epochs on
the host and hand them to one shg_*_points_at call per group of fields.
"""

import functools
import math

import numpy as np

from . import utilities
from .gravityfield import PotentialCoefficients, TimeSeries, _AtCall, _FunctionalsAtEpochs, _merge_fixed_calls


def epoch_arguments(epochs, reference_epoch, unit_seconds):
    """tau [M] of the checked `epochs` (a list of datetimes or float64 modified Julian dates): the time since reference_epoch in units
    of unit_seconds, as _WeightedFields.evaluate_at computes it.  The one expression behind the weights of Trend and Oscillation and
    the factors of lstsq.TemporalParameters.harmonic.  Host only."""
    if isinstance(epochs, np.ndarray):
        return (epochs - utilities._mjd(reference_epoch)) * 86400.0 / unit_seconds
    return np.array([(epoch - reference_epoch).total_seconds() / unit_seconds for epoch in epochs], dtype=np.float64)


class _WeightedFields(_FunctionalsAtEpochs):
    """V(t) = sum_i w_i(tau(t)) V_i; the fields are copied on construction (anything with `copy`, `*` by a float and `+`)."""

    def __init__(self, fields, reference_epoch, unit_days):
        self._fields = [f.copy() for f in fields]
        self._t0 = reference_epoch
        self._unit = 86400.0 * unit_days

    def _weights(self, tau):
        raise NotImplementedError

    def evaluate_at(self, epoch):
        tau = (epoch - self._t0).total_seconds() / self._unit
        terms = [field * weight for field, weight in zip(self._fields, self._weights(tau))]
        out = functools.reduce(lambda acc, term: acc + term, terms[1:], terms[0])
        out.epoch = epoch
        return out

    def _weights_at(self, tau):
        """_weights of every tau [M] at once: [M, W], float64"""
        raise NotImplementedError

    def weights_at(self, epochs):
        """The weights [M, W] of the fields at the checked `epochs` (a list of datetimes or float64 modified Julian dates): tau as
        evaluate_at computes it, total_seconds() of the difference over the unit.  Host only."""
        return self._weights_at(epoch_arguments(epochs, self._t0, self._unit))

    def _at_calls(self, epochs):
        fields = self._fields
        if not all(isinstance(f, PotentialCoefficients) for f in fields):
            raise TypeError('the functionals at epochs need PotentialCoefficients, not {0}'.format(
                next(type(f).__name__ for f in fields if not isinstance(f, PotentialCoefficients))))
        GM, R = fields[0].GM, fields[0].R
        if any(f.GM != GM or f.R != R for f in fields):
            raise ValueError('the functionals at epochs need a common GM and R for all fields')
        batch = TimeSeries._stack(fields)
        return [_AtCall(batch, batch.shape[-1] - 1, GM, R, np.zeros(len(epochs), dtype=np.int64), self.weights_at(epochs), True)]


class Trend(_WeightedFields):
    """Linear trend V(t) = V (t - t0) / time_scale, `time_scale` in days (default: a Julian year), grates/gravityfield.py:1054-1094."""

    def __init__(self, gravity_field, reference_epoch, time_scale=365.25):
        super().__init__([gravity_field], reference_epoch, time_scale)

    def _weights(self, tau):
        return (tau,)

    @staticmethod
    def _weights_at(tau):
        return tau[:, np.newaxis]


class Oscillation(_WeightedFields):
    """V(t) = V_c cos(2 pi (t - t0) / T) + V_s sin(2 pi (t - t0) / T), period T in days, grates/gravityfield.py:1097-1140."""

    def __init__(self, gravity_field_cosine, gravity_field_sine, period, reference_epoch):
        super().__init__([gravity_field_cosine, gravity_field_sine], reference_epoch, period)

    def _weights(self, tau):
        phase = 2.0 * math.pi * tau
        return (math.cos(phase), math.sin(phase))

    @staticmethod
    def _weights_at(tau):
        phase = 2.0 * math.pi * tau
        return np.stack((np.cos(phase), np.sin(phase)), axis=1)


class TimeVariableGravityField(_FunctionalsAtEpochs):
    """Sum of constituents (trend, cycles, an interpolated `TimeSeries`, ...), each with `evaluate_at`; `constituents` stays a
    public list like upstream (grates/gravityfield.py:784-812)."""

    def __init__(self, constituents):
        self.constituents = constituents

    def evaluate_at(self, epoch):
        parts = [c.evaluate_at(epoch) for c in self.constituents]
        return functools.reduce(lambda acc, part: acc + part, parts[1:], parts[0])

    def _at_calls(self, epochs):
        """the calls of the constituents in list order, adjacent trends and cycles of one GM and R merged into one"""
        if not self.constituents:
            raise ValueError('a time-variable field without constituents has no functionals')
        calls = []
        for constituent in self.constituents:
            if not hasattr(constituent, '_at_calls'):
                raise TypeError('constituent {0!r} has no functionals at epochs: a TimeSeries, Trend or Oscillation expected'.format(constituent))
            calls.extend(constituent._at_calls(epochs))
        return _merge_fixed_calls(calls)
