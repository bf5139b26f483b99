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
        self._describe(grid, location, times, time_indexing, backend)
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

    def _describe(self, grid, location, times, time_indexing, backend):
        """Location, times, indexing and backend: what every kind of series has."""
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


# ---- series on a source grid of their own, regridded on the device (include/csi.h, csi_time_series_set_regridded) ---------------------
class SourceGrid:
    """SourceGrid(x, y, periodic_x=False, period=None): a rectilinear source grid given by its 1-D nodes, in the coordinates of the
    model grid's nodes (degrees of longitude / latitude on a LatitudeLongitudeGrid or TripolarGrid).  Nodes are strictly increasing and
    finite, at least two and at most 65536 per axis; periodic_x: x repeats with `period` (None: inferred as the span of the nodes plus
    their last interval, csi_regrid_plan_axis)."""

    def __init__(self, x, y, periodic_x=False, period=None):
        self.x, self.y = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y))
        for name, a in (("x", self.x), ("y", self.y)):
            if a.ndim != 1 or a.size < 2 or not np.all(np.isfinite(a)) or not np.all(np.diff(a) > 0):
                raise ValueError(f"SourceGrid: the {name} nodes must be 1-D, at least two, finite and strictly increasing")
            if a.size > _lib.REGRID_MAX_SOURCE_EXTENT:
                raise ValueError(f"SourceGrid: at most {_lib.REGRID_MAX_SOURCE_EXTENT} {name} nodes (the device map stores indices as uint16)")
        self.periodic_x = bool(periodic_x)
        if period is not None and not self.periodic_x:
            raise ValueError("SourceGrid: a period needs periodic_x=True")
        if period is not None and not (np.isfinite(period) and float(period) > self.x[-1] - self.x[0]):
            raise ValueError("SourceGrid: the period must be longer than the span of the x nodes")
        self.period = 0.0 if period is None else float(period)

    @property
    def shape(self):
        """(len(y), len(x)): the shape of a slice."""
        return self.y.size, self.x.size

    def plan(self, X, Y):
        """(i0, i1, j0, j1, wx, wy) of target points: csi_regrid_plan_axis per axis for 1-D X (nx,) and Y (ny,), per point for 2-D
        X, Y of one shape.  Arrays of the target's (ny, nx) shape."""
        X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        ax = lambda nodes, per, period, v: np.array([_lib.regrid_plan_axis(nodes, per, period, t) for t in v.ravel()]).reshape(v.shape + (3,))  # noqa: E731
        px, py = ax(self.x, self.periodic_x, self.period, X), ax(self.y, False, 0.0, Y)
        if X.ndim == 1 and Y.ndim == 1:
            px, py = np.broadcast_to(px[None, :, :], (Y.size, X.size, 3)), np.broadcast_to(py[:, None, :], (Y.size, X.size, 3))
        elif X.shape != Y.shape or X.ndim != 2:
            raise ValueError("SourceGrid.plan: 1-D x and y nodes, or 2-D nodes of one shape")
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731
        return (i32(px[..., 0]), i32(px[..., 1]), i32(py[..., 0]), i32(py[..., 1]),
                np.ascontiguousarray(px[..., 2]), np.ascontiguousarray(py[..., 2]))


class RegriddedTimeSeries(FieldTimeSeries):
    """RegriddedTimeSeries(grid, location, source, times, data, time_indexing=Linear(), backend=InMemory()): a series given on a
    SourceGrid.  data has the shape (Nt, len(source.y), len(source.x)) and must be finite (fill_missing); it is NOT cut on tiles -- every
    rank holds the whole source.  At every update the library interpolates in time at the four source points around each point of
    `location`, then bilinearly in space (include/csi.h).  Accepted wherever a FieldTimeSeries is."""

    component = None                     # (a member of a RegriddedVectorTimeSeries: 0 / 1)

    def __init__(self, grid, location, source, times, data, time_indexing=None, backend=None):
        self._describe(grid, location, times, time_indexing, backend)
        if not isinstance(source, SourceGrid):
            raise TypeError("RegriddedTimeSeries: source is a SourceGrid")
        self.source = source
        self.data = self._source_data(data, "data")

    def _source_data(self, data, name):
        arr = np.ascontiguousarray(data, dtype=np.float64)
        want = (self.times.size,) + self.source.shape
        if arr.shape != want:
            raise ValueError(f"{type(self).__name__}: {name} of shape (Nt, len(y), len(x)) = {want} is needed, got {arr.shape}")
        if not np.all(np.isfinite(arr)):
            raise ValueError(f"{type(self).__name__}: {name} must be finite -- a weight may be exactly 0, and 0 * NaN is NaN (fill_missing "
                             "replaces the land points of an ocean product)")
        return arr

    @property
    def interior_shape(self):
        """The TARGET shape: the interior of a field at the series' location (the slices themselves have source.shape)."""
        return tuple(reversed(self.grid.interior_size(*self.location)))

    @property
    def parts(self):
        """The source arrays the slot reads: (data,) of a scalar, (east, north) of a component of a pair."""
        return (self.data,)


class _VectorComponent(RegriddedTimeSeries):
    def __init__(self, pair, component):
        self.pair, self.component = pair, component
        self._describe(pair.grid, (Face, Center) if component == 0 else (Center, Face), pair.times, pair.time_indexing, pair.backend)
        self.source = pair.source
        self.data = pair.east if component == 0 else pair.north

    @property
    def parts(self):
        return self.pair.east, self.pair.north


class RegriddedVectorTimeSeries:
    """RegriddedVectorTimeSeries(grid, source, times, east, north, time_indexing=Linear(), backend=InMemory()): the eastward and
    northward components of a vector (a wind, an ocean current) on a SourceGrid.  `.x` drives a (Face, Center) slot with
    E cos + N sin at ITS points, `.y` a (Center, Face) slot with N cos - E sin at its points, (cos, sin) = grid.rotation(location):
    give them where the two components of a stress, SemiImplicitStress(ue=, ve=), free_drift=dict(u=, v=) or model.forcing are
    accepted.  Pairs at (Center, Center) are not rotated: not built."""

    def __init__(self, grid, source, times, east, north, time_indexing=None, backend=None):
        probe = RegriddedTimeSeries(grid, (Center, Center), source, times, east, time_indexing, backend)
        self.grid, self.source, self.times = grid, source, probe.times
        self.time_indexing, self.backend = probe.time_indexing, probe.backend
        self.east, self.north = probe.data, probe._source_data(north, "north")
        self.x, self.y = _VectorComponent(self, 0), _VectorComponent(self, 1)

    def __iter__(self):
        return iter((self.x, self.y))


def fill_missing(data, valid):
    """Replace the invalid points of source data (..., ny, nx) by the value of the nearest valid point along the source grid: breadth
    first from the valid points over the four neighbours (no wrap), so "nearest" counts grid steps.  An invalid point reached in the
    same round from several filled neighbours takes the FIRST in the order south (j - 1), north (j + 1), west (i - 1), east (i + 1).
    valid: a bool (ny, nx) array, one mask for every leading index.  Nothing changes where valid is True; a mask without a valid point
    raises.  Pure NumPy, once, on the small source grid -- the kernel needs finite sources."""
    out = np.array(data, dtype=np.float64, copy=True)
    done = np.array(valid, dtype=bool, copy=True)
    if done.ndim != 2 or out.shape[-2:] != done.shape:
        raise ValueError("fill_missing: valid is a (ny, nx) bool array of the data's last two extents")
    if not done.any():
        raise ValueError("fill_missing: no valid point")
    shifts = ((slice(1, None), slice(None), slice(None, -1), slice(None)),      # from the south: (j, i) <- (j - 1, i)
              (slice(None, -1), slice(None), slice(1, None), slice(None)),      # from the north
              (slice(None), slice(1, None), slice(None), slice(None, -1)),      # from the west
              (slice(None), slice(None, -1), slice(None), slice(1, None)))      # from the east
    while not done.all():
        new, was = done.copy(), out.copy()
        for tj, ti, sj, si in shifts:
            take = np.zeros_like(done)
            take[tj, ti] = done[sj, si]
            take &= ~new
            src = np.zeros_like(out)
            src[..., tj, ti] = was[..., sj, si]
            out[..., take] = src[..., take]
            new |= take
        done = new
    return out
