"""NumPy restatement of the regridding of forcing time series given on a rectilinear source grid, written from the statement in
include/csi.h (csi_regrid_plan_axis, csi_time_series_set_regridded): the oracle of tests/test_regrid_ref.py and
tests/test_gpu_regrid.py.  Plain double arithmetic in the stated order -- time first, then x, then y, every line two products and one
sum --, so the library has to agree BIT FOR BIT."""
import numpy as np

import time_series_ref as tref

InvalidAxis = tref.InvalidSeries


def plan_axis(nodes, periodic, period, x):
    """(i0, i1, w): the time-indexing rule applied to space -- a non-periodic axis is CLAMP, a periodic one CYCLICAL."""
    return tref.plan(nodes, tref.CYCLICAL if periodic else tref.CLAMP, period if periodic else 0.0, x)


def plan_points(xs, ys, periodic_x, period, X, Y):
    """(i0, i1, j0, j1, wx, wy) as (ny, nx) arrays for 1-D target nodes X (nx,), Y (ny,) or 2-D target nodes of one shape."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    px = np.array([plan_axis(xs, periodic_x, period, v) for v in X.ravel()]).reshape(X.shape + (3,))
    py = np.array([plan_axis(ys, False, 0.0, v) for v in Y.ravel()]).reshape(Y.shape + (3,))
    if X.ndim == 1:
        px, py = np.broadcast_to(px[None], (Y.size, X.size, 3)), np.broadcast_to(py[:, None], (Y.size, X.size, 3))
    ints = lambda a: np.array(a, dtype=np.int64)      # noqa: E731
    return ints(px[..., 0]), ints(px[..., 1]), ints(py[..., 0]), ints(py[..., 1]), np.array(px[..., 2]), np.array(py[..., 2])


def bilinear(c00, c10, c01, c11, wx, wy):
    """lo = c10 wx + c00 (1 - wx); hi = c11 wx + c01 (1 - wx); val = hi wy + lo (1 - wy).  c10: the corner at (i1, j0)."""
    ux, uy = np.float64(1.0) - wx, np.float64(1.0) - wy
    lo = c10 * wx + c00 * ux
    hi = c11 * wx + c01 * ux
    return hi * wy + lo * uy


def corners(slice2d, m):
    i0, i1, j0, j1 = m[:4]
    return slice2d[j0, i0], slice2d[j0, i1], slice2d[j1, i0], slice2d[j1, i1]


def regrid_slice(slice2d, m):
    """One source slice on the target points of the map m = (i0, i1, j0, j1, wx, wy)."""
    return bilinear(*corners(slice2d, m), m[4], m[5])


def at(times, data, indexing, period, t, m):
    """The value at time t on the target points: TIME at the four corners first (time_series_ref.interpolate per corner), then space."""
    n1, n2, frac = tref.plan(times, indexing, period, t)
    c = [tref.interpolate([a, b], 0, 0 if n1 == n2 else 1, frac) for a, b in zip(corners(data[n1], m), corners(data[n2], m))]
    return bilinear(*c, m[4], m[5])


def at_space_first(times, data, indexing, period, t, m):
    """The other order, which the library does NOT use: both slices regridded, then interpolated in time."""
    n1, n2, frac = tref.plan(times, indexing, period, t)
    return tref.interpolate([regrid_slice(data[n1], m), regrid_slice(data[n2], m)], 0, 0 if n1 == n2 else 1, frac)


def rotate(val_e, val_n, cos, sin, component):
    """x = E cos + N sin (component 0) / y = N cos - E sin (component 1)."""
    return val_e * cos + val_n * sin if component == 0 else val_n * cos - val_e * sin


def pair_at(times, east, north, indexing, period, t, m, cos, sin, component):
    return rotate(at(times, east, indexing, period, t, m), at(times, north, indexing, period, t, m), cos, sin, component)


def of_series(fts, t, m, rotation=None):
    """... of a csi.RegriddedTimeSeries (a member of a pair: rotation = (cos, sin) at its location)."""
    ind = fts.time_indexing
    if fts.component is None:
        return at(fts.times, fts.data, ind.kind, ind.period, t, m)
    east, north = fts.parts
    return pair_at(fts.times, east, north, ind.kind, ind.period, t, m, rotation[0], rotation[1], fts.component)


def bearing_haversine(lam_m, phi_m, lam_p, phi_p):
    """The initial great-circle bearing against east from (lam-, phi-) to (lam+, phi+), degrees in, radians out, evaluated at the
    midpoint by symmetry: the mean of the forward bearing at the start and the back-bearing-reversed at the end, each from half-angle
    (haversine) differences.  An independent route to TripolarGrid.rotation's angle."""
    def initial(l1, p1, l2, p2):
        l1, p1, l2, p2 = (np.deg2rad(v) for v in (l1, p1, l2, p2))
        dl = l2 - l1
        north = np.cos(p1) * np.sin(p2) - np.sin(p1) * np.cos(p2) * np.cos(dl)
        east = np.sin(dl) * np.cos(p2)
        return np.arctan2(north, east)
    fwd = initial(lam_m, phi_m, lam_p, phi_p)
    back = initial(lam_p, phi_p, lam_m, phi_m)                    # points back along the arc: reverse it
    rev = np.arctan2(-np.sin(back), -np.cos(back))
    d = np.arctan2(np.sin(rev - fwd), np.cos(rev - fwd))
    return fwd + 0.5 * d
