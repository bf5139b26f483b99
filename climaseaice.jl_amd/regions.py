"""Per-region ice integrals and extrema, reduced on the device (include/csi.h, "per-region ice integrals and extrema").

Regions                  an (Ny, Nx) integer map of region ids 0 .. n - 1 (anything else: no region) with a name per region; builders for
                         hemispheres, latitude bands and named masks.  The device parent is built once per model device and tile
regional_diagnostics     model.regional_diagnostics(regions): csi_regions_compute -- the tracer group of model.diagnostics() per region, in
                         the library's summation order, in one call; no field crosses the bus
RegionalSeriesWriter     model.output_writers["regions"] = RegionalSeriesWriter(regions, schedule, dir): growable .npy series
load_regional_series     reads them back

On a tiled model every call here is COLLECTIVE; each rank passes its piece of the map and all ranks get the same bits.

Not built (refused by name where it can be asked for): more than 64 regions per call (call again with another map), overlapping regions,
the velocity group or the non-finite counts per region, time averages in the series writer.
"""
import json
import os
from types import MappingProxyType, SimpleNamespace

import numpy as np
import torch

from . import _lib
from .grids import Center, LatitudeLongitudeGrid, TileGrid, TripolarGrid
from .output import GrowableNpy

REGIONS_MAX = _lib.REGIONS_MAX
SUMS = ("ice_volume", "ice_area", "ice_extent", "snow_volume", "region_area")
EXTREMA = ("min_h", "max_h", "min_aice", "max_aice", "max_hs")
QUANTITIES = SUMS + EXTREMA + ("cells", "ice_mass")      # one vector per name in a RegionalDiagnostics, one file per name in a series
_SNOW = ("snow_volume", "max_hs")


def _global(grid):
    return grid.global_grid if isinstance(grid, TileGrid) else grid


class Regions:
    """Regions(grid, ids, names = None): `ids` is an (Ny, Nx) integer array over the (global) grid; a cell with id r in 0 .. n - 1 belongs
    to region r, any other id to none.  n = len(names), or max(ids) + 1 without names (names "0" .. "n-1")."""

    def __init__(self, grid, ids, names=None):
        G = _global(grid)
        a = np.asarray(ids)
        if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"Regions: ids must be an integer array, got dtype {a.dtype}")
        if a.shape != (G.Ny, G.Nx):
            raise ValueError(f"Regions: ids must have the shape (Ny, Nx) = {(G.Ny, G.Nx)} of the (global) grid, got {a.shape}")
        info = np.iinfo(np.int32)
        if a.size and (a.min() < info.min or a.max() > info.max):
            raise ValueError("Regions: ids must fit int32")
        if names is None:
            n = int(a.max()) + 1 if a.size and a.max() >= 0 else 1
            if n > REGIONS_MAX:
                raise ValueError(f"Regions: ids up to {n - 1} without names; at most {REGIONS_MAX} regions per map (give names to use fewer)")
            names = [str(k) for k in range(n)]
        names = [str(s) for s in names]
        if not 1 <= len(names) <= REGIONS_MAX:
            raise ValueError(f"Regions: between 1 and {REGIONS_MAX} regions per map, got {len(names)} (call again with another map for more)")
        if len(set(names)) != len(names):
            raise ValueError("Regions: names must be distinct")
        self.grid, self.names = G, tuple(names)
        self.ids = np.ascontiguousarray(a, dtype=np.int32)
        self.ids.setflags(write=False)
        self._parents = {}

    @property
    def n(self):
        return len(self.names)

    def index(self, name):
        if isinstance(name, (int, np.integer)):
            if not 0 <= int(name) < self.n:
                raise KeyError(f"region {name} (the map has {self.n} regions)")
            return int(name)
        try:
            return self.names.index(name)
        except ValueError:
            raise KeyError(f"region {name!r} (regions: {', '.join(self.names)})") from None

    # ---- builders
    @classmethod
    def hemispheres(cls, grid):
        """"south" (0) / "north" (1) by the sign of the cell-centre latitude (a centre on the equator: north)."""
        lat = _center_latitude(grid, "Regions.hemispheres")
        return cls(grid, (lat >= 0.0).astype(np.int32), names=("south", "north"))

    @classmethod
    def latitude_bands(cls, grid, edges, names=None):
        """Band k holds the cells whose centre latitude lies in [edges[k], edges[k + 1]); cells outside every band get -1.  edges: at
        least two strictly increasing finite values."""
        e = np.asarray(edges, dtype=np.float64).reshape(-1)
        if e.size < 2 or not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
            raise ValueError("Regions.latitude_bands: edges must be at least two strictly increasing finite latitudes")
        lat = _center_latitude(grid, "Regions.latitude_bands")
        k = np.searchsorted(e, lat, side="right") - 1
        k[(lat < e[0]) | (lat >= e[-1])] = -1
        if names is None:
            names = [f"{e[q]:g}..{e[q + 1]:g}" for q in range(e.size - 1)]
        if len(names) != e.size - 1:
            raise ValueError(f"Regions.latitude_bands: {e.size - 1} bands need {e.size - 1} names, got {len(names)}")
        return cls(grid, k.astype(np.int32), names=names)

    @classmethod
    def from_masks(cls, masks, grid=None):
        """masks: {"name": (Ny, Nx) boolean array, ...}, in region order.  Overlapping masks are refused by name; cells no mask covers
        get -1.  grid: checked against the masks' shape if given."""
        if not masks:
            raise ValueError("Regions.from_masks: no masks")
        if grid is None:
            ny, nx = np.shape(next(iter(masks.values())))
            grid = SimpleNamespace(Nx=nx, Ny=ny)
        G = _global(grid)
        ids = np.full((G.Ny, G.Nx), -1, dtype=np.int32)
        for k, (name, m) in enumerate(masks.items()):
            m = np.asarray(m)
            if m.dtype != bool or m.shape != (G.Ny, G.Nx):
                raise ValueError(f"Regions.from_masks: mask {name!r} must be a boolean array of shape (Ny, Nx) = {(G.Ny, G.Nx)}")
            taken = m & (ids >= 0)
            if taken.any():
                other = list(masks)[int(ids[taken][0])]
                raise ValueError(f"Regions.from_masks: masks {other!r} and {name!r} overlap in {int(taken.sum())} cells (overlapping regions are not built)")
            ids[m] = k
        return cls(grid, ids, names=list(masks))

    # ---- plumbing
    def piece(self, grid):
        """The (Ny, Nx) ids of `grid`: the map itself, or a tile's piece of it."""
        G = _global(grid)
        if (G.Nx, G.Ny) != (self.grid.Nx, self.grid.Ny):
            raise ValueError(f"regions: the map was made for a {self.grid.Nx} x {self.grid.Ny} grid, the model's is {G.Nx} x {G.Ny}")
        if isinstance(grid, TileGrid):
            return self.ids[grid.j_off:grid.j_off + grid.Ny, grid.i_off:grid.i_off + grid.Nx]
        return self.ids

    def device_parent(self, grid, device):
        """The map as an int32 device array laid out like a (c,c) parent of `grid` (halo elements -1; they are never read), built once
        per (device, tile)."""
        key = (str(device), getattr(grid, "i_off", 0), getattr(grid, "j_off", 0), grid.Nx, grid.Ny, grid.Hx, grid.Hy)
        t = self._parents.get(key)
        if t is None:
            full = np.full((grid.Ny + 2 * grid.Hy, grid.Nx + 2 * grid.Hx), -1, dtype=np.int32)
            full[grid.Hy:grid.Hy + grid.Ny, grid.Hx:grid.Hx + grid.Nx] = self.piece(grid)
            t = torch.from_numpy(full).to(device)
            if t.is_cuda:      # torch wrote on ITS stream, the library works on its own
                torch.cuda.current_stream(t.device).synchronize()
            self._parents[key] = t
        return t


def _center_latitude(grid, who):
    """(Ny, Nx) latitudes of the cell centres of the (global) grid; grids without latitudes raise by name."""
    G = _global(grid)
    if isinstance(G, TripolarGrid):
        return np.asarray(G.nodes_2d(Center, Center)[1], dtype=np.float64)
    if isinstance(G, LatitudeLongitudeGrid):
        return np.broadcast_to(np.asarray(G.ynodes(Center), dtype=np.float64)[:, None], (G.Ny, G.Nx)).copy()
    raise NotImplementedError(f"{who}: a LatitudeLongitudeGrid or a TripolarGrid is needed; a {type(G).__name__} has no cell-centre "
                              "latitudes (build the map from your own arrays: Regions(grid, ids) or Regions.from_masks)")


class RegionalDiagnostics:
    """The result of model.regional_diagnostics(): immutable.  One NumPy vector of n_regions entries per quantity (QUANTITIES), float64
    (cells: int64), read-only; snow_volume and max_hs are None without a snow layer.  r["north"] (or r[1]) is one region's values as a
    read-only mapping.  unassigned_cells: the active cells whose id names no region.  Definitions and the summation order: include/csi.h."""
    __slots__ = ("names", "has_snow", "extent_threshold", "unassigned_cells", "_v")

    def __init__(self, names, has_snow, extent_threshold, unassigned_cells, values):
        v = {}
        for k in QUANTITIES:
            a = values.get(k)
            if a is not None:
                a = np.array(a, dtype=np.int64 if k == "cells" else np.float64)
                a.setflags(write=False)
            v[k] = a
        for k, x in (("names", tuple(names)), ("has_snow", bool(has_snow)), ("extent_threshold", float(extent_threshold)),
                     ("unassigned_cells", int(unassigned_cells)), ("_v", MappingProxyType(v))):
            object.__setattr__(self, k, x)

    def __setattr__(self, k, x):
        raise AttributeError("RegionalDiagnostics is immutable")

    def __getattr__(self, k):
        if k in QUANTITIES:
            return self._v[k]
        raise AttributeError(k)

    def __getitem__(self, region):
        if isinstance(region, (int, np.integer)):
            r = int(region)
            if not 0 <= r < len(self.names):
                raise KeyError(f"region {region} (the record has {len(self.names)} regions)")
        else:
            if region not in self.names:
                raise KeyError(f"region {region!r} (regions: {', '.join(self.names)})")
            r = self.names.index(region)
        return MappingProxyType({k: (None if a is None else a[r].item()) for k, a in self._v.items()})

    def __len__(self):
        return len(self.names)

    def __repr__(self):
        return f"RegionalDiagnostics({', '.join(self.names)}; unassigned_cells = {self.unassigned_cells})"


def regional_diagnostics(model, regions, extent_threshold=0.15):
    """csi_regions_compute on the model's context: two launches and one small copy on the library's stream, which it waits for.
    Collective on a tiled model."""
    if not isinstance(regions, Regions):
        raise TypeError("regional_diagnostics: `regions` must be a csi.Regions")
    parent = regions.device_parent(model.grid, model.device)
    rec, stray = model.ctx.regions_compute(parent.data_ptr(), parent.shape[1], regions.n, extent_threshold)
    snow = model.snow_thickness is not None
    values = {k: [getattr(rec[r], k) for r in range(regions.n)] for k in SUMS + EXTREMA + ("cells",)}
    values["ice_mass"] = [model.sea_ice_density * v for v in values["ice_volume"]]
    if not snow:
        for k in _SNOW:
            values[k] = None
    return RegionalDiagnostics(regions.names, snow, extent_threshold, stray, values)


class RegionalSeriesWriter:
    """RegionalSeriesWriter(regions, schedule, dir, extent_threshold = 0.15, overwrite_existing = False): regional series as growable .npy
    files.

    Implements the begin / after_step protocol of model.output_writers; schedule: IterationInterval or TimeInterval (output.py).  Files:
    `dir/<quantity>.npy` of shape (records, n_regions) for every name of QUANTITIES the model has (float64; cells: int64),
    `unassigned_cells.npy`, `time.npy`, `iteration.npy` and `meta.json` with the regions' names; after every record each is a valid NPY
    file.  A record is one regional_diagnostics call (it waits for the model's stream).  On a tiled model every rank makes the call and
    holds the same record: give each rank's writer its own directory.  recorder: a stand-in for the device call in tests, (regions, model, threshold) -> RegionalDiagnostics."""

    def __init__(self, regions, schedule, dir, extent_threshold=0.15, overwrite_existing=False, recorder=None):
        if not isinstance(regions, Regions):
            raise TypeError("RegionalSeriesWriter: `regions` must be a csi.Regions")
        if getattr(schedule, "averaged", False):
            raise NotImplementedError("RegionalSeriesWriter: time averages of regional series are not built; IterationInterval or TimeInterval")
        self.regions, self.schedule, self.dir, self.extent_threshold = regions, schedule, dir, float(extent_threshold)
        self.recorder = recorder
        if os.path.exists(dir):
            if not overwrite_existing:
                raise FileExistsError(f"RegionalSeriesWriter: {dir} exists (overwrite_existing = False)")
            for n in QUANTITIES + ("unassigned_cells", "time", "iteration"):
                if os.path.exists(os.path.join(dir, n + ".npy")):
                    os.remove(os.path.join(dir, n + ".npy"))
        os.makedirs(dir, exist_ok=True)
        self.files = None                       # made at the first record: which quantities exist depends on the model (snow)
        self.records = 0
        self._started = False
        self.closed = False

    def _open(self, rec):
        n = self.regions.n
        self.quantities = [k for k in QUANTITIES if getattr(rec, k) is not None]
        self.files = {k: GrowableNpy(os.path.join(self.dir, k + ".npy"), "<i8" if k == "cells" else "<f8", (n,)) for k in self.quantities}
        self.stray_file = GrowableNpy(os.path.join(self.dir, "unassigned_cells.npy"), "<i8", ())
        self.time_file = GrowableNpy(os.path.join(self.dir, "time.npy"), "<f8", ())
        self.iteration_file = GrowableNpy(os.path.join(self.dir, "iteration.npy"), "<i8", ())
        with open(os.path.join(self.dir, "meta.json"), "w") as fh:
            json.dump({"names": list(self.regions.names), "quantities": self.quantities, "extent_threshold": self.extent_threshold,
                       "schedule": self.schedule.describe(), "grid": {"Nx": self.regions.grid.Nx, "Ny": self.regions.grid.Ny}}, fh, indent=1)

    def begin(self, model):
        if self._started:
            return
        self._started = True
        self.schedule.attach(model.clock)
        if self.schedule.initial(model.clock):
            self._record(model, model.clock.time)

    def after_step(self, model, dt):
        self.begin(model)
        for action, value in self.schedule.after_step(model.clock, dt):
            if action == "write":
                self._record(model, value)

    def next_time(self, model):
        self.begin(model)
        return self.schedule.next_time(model.clock)

    def write(self, model):
        """Force a record of the current state."""
        if not self._started:
            self._started = True
            self.schedule.attach(model.clock)
            self.schedule.initial(model.clock)
        self._record(model, model.clock.time)

    def _record(self, model, time):
        rec = (self.recorder or regional_diagnostics)(*((self.regions, model, self.extent_threshold) if self.recorder
                                                        else (model, self.regions, self.extent_threshold)))
        if self.files is None:
            self._open(rec)
        for k in self.quantities:
            self.files[k].append(getattr(rec, k))
        self.stray_file.append(np.int64(rec.unassigned_cells))
        self.time_file.append(np.float64(time))
        self.iteration_file.append(np.int64(model.clock.iteration))
        self.records += 1

    def flush(self):
        pass                                         # (nothing is in flight: every record is written when it is taken)

    def close(self):
        if self.closed:
            return
        if self.files is not None:
            for f in list(self.files.values()) + [self.stray_file, self.time_file, self.iteration_file]:
                f.close()
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def load_regional_series(dir):
    """The files of a RegionalSeriesWriter's directory as a dict: quantity -> (records, n_regions) array, plus "unassigned_cells",
    "time", "iteration" and "names"."""
    meta = json.load(open(os.path.join(dir, "meta.json")))
    out = {n: np.load(os.path.join(dir, n + ".npy")) for n in meta["quantities"] + ["unassigned_cells", "time", "iteration"]}
    out["names"] = tuple(meta["names"])
    return out
