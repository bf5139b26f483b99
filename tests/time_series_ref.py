"""NumPy restatement of the time indexing and the interpolation of forcing time series, written from the statement in include/csi.h
(csi_time_series_plan): the oracle of tests/test_time_series_plan.py, tests/test_time_series_frontend.py and
tests/test_gpu_time_series.py.  Plain double arithmetic in the stated order, so the library has to agree BIT FOR BIT."""
import math

import numpy as np

CLAMP, CYCLICAL, LINEAR = 0, 1, 2


class InvalidSeries(ValueError):
    pass


def inferred_period(times):
    return (times[-1] - times[0]) + (times[-1] - times[-2])


def _between(times, t):
    n = int(np.searchsorted(times, t, side="right")) - 1          # the last node at or below t
    if times[n] == t:
        return n, n, 0.0
    return n, n + 1, float((t - times[n]) / (times[n + 1] - times[n]))


def plan(times, indexing, period, t):
    """(n1, n2, weight): 0-based slice indices and the weight of slice n2."""
    times = np.asarray(times, dtype=np.float64)
    nt = times.size
    if nt < 2 or not np.all(np.isfinite(times)) or not np.all(np.diff(times) > 0) or not math.isfinite(t):
        raise InvalidSeries("nt >= 2, strictly increasing finite times and a finite time are needed")
    if indexing not in (CLAMP, CYCLICAL, LINEAR):
        raise InvalidSeries("unknown indexing kind")
    t = np.float64(t)
    first, last = times[0], times[-1]
    if indexing == CYCLICAL:
        span = last - first
        if period > 0:
            if not (period > span and math.isfinite(period)):
                raise InvalidSeries("the period must exceed the span of the times")
            P = np.float64(period)
        else:
            P = inferred_period(times)
        r = np.fmod(t - first, P)
        if r < 0:
            r = r + P
        tp = first + r
        if tp > last:                                              # the gap behind the last node
            return nt - 1, 0, float((tp - last) / (P - span))
        if tp == last:
            return nt - 1, nt - 1, 0.0
        if tp <= first:
            return 0, 0, 0.0
        return _between(times, tp)
    if t <= first or t >= last:
        low = t <= first
        if indexing == CLAMP or t == first or t == last:
            n = 0 if low else nt - 1
            return n, n, 0.0
        n1 = 0 if low else nt - 2                                  # LINEAR: extrapolate from the first / last two slices
        return n1, n1 + 1, float((t - times[n1]) / (times[n1 + 1] - times[n1]))
    return _between(times, t)


def interpolate(data, n1, n2, frac):
    """psi = (n1 == n2) ? psi_1 : psi_2 * frac + psi_1 * (1 - frac): two products and one sum."""
    if n1 == n2:
        return np.array(data[n1], dtype=np.float64, copy=True)
    w2 = np.float64(frac)
    w1 = np.float64(1.0) - w2
    return data[n2] * w2 + data[n1] * w1


def at(times, data, indexing, period, t):
    """The interpolated slice at time t."""
    return interpolate(data, *plan(times, indexing, period, t))


def of_series(fts, t):
    """... of a csi.FieldTimeSeries."""
    return at(fts.times, fts.data, fts.time_indexing.kind, fts.time_indexing.period, t)
