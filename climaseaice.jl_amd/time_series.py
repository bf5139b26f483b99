"""FieldTimeSeries: forcing given at a list of times and interpolated at the model clock on the device.

FieldTimeSeries(grid, location, times, data, time_indexing, backend)   upstream Oceananigans.OutputReaders.FieldTimeSeries as the
                                                                       reference uses it (sea_ice_model.jl:391-408,
                                                                       thermodynamic_time_step.jl:326-329)
Clamp(), Cyclical(period=None), Linear()                               upstream time indexing (RECALLED: include/csi.h states the rules)
InMemory() / InMemory(n)                                               all slices on the device / n of them, the rest in host memory

A series drives one of fourteen arrays of a SeaIceModel: the stress components or external velocities of the top and bottom stresses,
model.forcing u / v, the free-drift fields, the array term of the top / bottom heat flux, snowfall, the coefficient and reference
temperature of a LinearHeatFlux, the bottom salinity (and the mixed layer's four inputs and the flux of a ShortwaveRadiation: nineteen).  The model allocates the array as
for a plain array and registers the series; csi_time_series_update interpolates it in place at the start of every step.
"""
import numpy as np

from . import _lib
from .grids import Center, Face, TileGrid


class Clamp:
    """Outside the times the end slice is used."""
    kind = _lib.TIME_CLAMP
    period = 0.0


class Linear:
    """Outside the times the first / last two slices are extrapolated."""
    kind = _lib.TIME_LINEAR
    period = 0.0


class Cyclical:
    """The series repeats with `period` (None: inferred, the span of the times plus their last interval)."""
    kind = _lib.TIME_CYCLICAL

    def __init__(self, period=None):
        if period is not None and not float(period) > 0.0:
            raise ValueError("Cyclical: the period must be positive (None: inferred from the times)")
        self.period = 0.0 if period is None else float(period)


class InMemory:
    """InMemory(): every slice on the device.  InMemory(n): n >= 2 slices on the device at a time, the series itself in host memory."""

    def __init__(self, chunk_size=None):
        if chunk_size is not None and (isinstance(chunk_size, bool) or int(chunk_size) != chunk_size or int(chunk_size) < 2):
            raise ValueError("InMemory(n): n >= 2 slices are needed to interpolate between two of them")
        self.chunk_size = None if chunk_size is None else int(chunk_size)


_LOCATIONS = {(Face, Center): "(Face, Center)", (Center, Face): "(Center, Face)", (Center, Center): "(Center, Center)"}


class FieldTimeSeries:
    """FieldTimeSeries(grid, location, times, data=None, time_indexing=Linear(), backend=InMemory()).

    location: (Face, Center), (Center, Face) or (Center, Center) -- a third entry, the vertical one, is ignored.  data has the shape
    (Nt, ny, nx) of Nt interiors of a field at that location (a Face field on a Bounded side is one wider); on a TileGrid an array of
    the global grid's shape is cut to the tile.  None: zeros, to be filled through `.data` before the model is built."""

    def __init__(self, grid, location, times, data=None, time_indexing=None, backend=None):
        loc = tuple(location)
        if len(loc) in (2, 3) and all(x is None for x in loc):
            raise NotImplementedError("FieldTimeSeries{Nothing, Nothing, Nothing}: a time series of NUMBERS is not supported on the "
                                      "accelerated path; give a series of fields at (Face, Center), (Center, Face) or (Center, Center)")
        if len(loc) not in (2, 3) or loc[:2] not in _LOCATIONS:
            raise NotImplementedError(f"FieldTimeSeries: location {location!r} is not supported -- a series drives a stress / velocity "
                                      "component at (Face, Center) or (Center, Face) or a cell quantity at (Center, Center)")
        self.grid, self.location = grid, loc[:2]
        self.times = np.ascontiguousarray(times, dtype=np.float64)
        if self.times.ndim != 1 or self.times.size < 2 or not np.all(np.diff(self.times) > 0) or not np.all(np.isfinite(self.times)):
            raise ValueError("FieldTimeSeries: at least two strictly increasing, finite times are needed")
        self.time_indexing = time_indexing if time_indexing is not None else Linear()
        if not isinstance(self.time_indexing, (Clamp, Cyclical, Linear)):
            raise TypeError("time_indexing: Clamp(), Cyclical(period) or Linear()")
        if isinstance(self.time_indexing, Cyclical) and self.time_indexing.period and \
                not self.time_indexing.period > self.times[-1] - self.times[0]:
            raise ValueError("Cyclical: the period must be longer than the span of the times")
        self.backend = backend if backend is not None else InMemory()
        if not isinstance(self.backend, InMemory):
            raise NotImplementedError(f"FieldTimeSeries backend {type(self.backend).__name__}: InMemory() or InMemory(n); reading a "
                                      "series from disk is not supported")
        nx, ny = grid.interior_size(*self.location)
        nt = self.times.size
        if data is None:
            arr = np.zeros((nt, ny, nx))
        else:
            arr = np.asarray(data, dtype=np.float64)
            if isinstance(grid, TileGrid) and arr.ndim == 3 and arr.shape[1:] == tuple(reversed(grid.global_grid.interior_size(*self.location))) \
                    and arr.shape[1:] != (ny, nx):
                arr = arr[:, grid.j_off:grid.j_off + ny, grid.i_off:grid.i_off + nx]
            if arr.shape != (nt, ny, nx):
                raise ValueError(f"FieldTimeSeries at {_LOCATIONS[self.location]}: data of shape (Nt, ny, nx) = {(nt, ny, nx)} is needed, "
                                 f"got {arr.shape}")
        self.data = np.ascontiguousarray(arr)

    def __len__(self):
        return self.times.size

    @property
    def interior_shape(self):
        return self.data.shape[1:]

    def plan(self, t):
        """(n1, n2, weight) at time t: csi_time_series_plan."""
        return _lib.time_series_plan(self.times, self.time_indexing.kind, self.time_indexing.period, t)


def refuse_series(value, what):
    """Raise, by name, where a FieldTimeSeries is given for a quantity that no series can drive."""
    if isinstance(value, FieldTimeSeries):
        raise NotImplementedError(f"{what}: a FieldTimeSeries cannot drive this quantity -- series are accepted for the stress components, "
                                  "SemiImplicitStress(ue=, ve=), free_drift=dict(u=, v=), model.forcing, the array term of "
                                  "top_heat_flux / bottom_heat_flux and snowfall")
