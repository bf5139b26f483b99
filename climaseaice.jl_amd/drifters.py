"""Lagrangian ice drifters: points that move with the ice, advected and sampled on the device (include/csi.h, "Lagrangian ice drifters").

Stands where users of the reference copy u and v to the host after every step and integrate buoy tracks there (Oceananigans gives its
ocean models LagrangianParticles; SeaIceModel has no counterpart).  The state -- index-space positions xi in [0, Nx], eta in [0, Ny] and
an int32 status per drifter -- lives in torch tensors (device memory plumbing only); the library keeps none of it.

Drifters        the state; advance(model, dt, substeps) and sample(model, *names) are one launch each on the model's stream
DrifterWriter   model.output_writers["tracks"] = DrifterWriter(drifters, schedule, dir, columns = ...): growable .npy tracks

model.drifters = Drifters(...) makes time_step advance them with the step's dt, after the clock has advanced and before the writers run,
with the velocities the step leaves; prognostic_state / restore_prognostic_state then carry drifters.xi, drifters.eta, drifters.status.

Not built (refused by name where it can be asked for): tiled models (a drifter would have to migrate between ranks), RightFolded grids
(crossing the fold re-orients the drifter), sorting or binning the drifters by cell, deformation from drifter triplets, sampling of
derived or momentum term fields, asynchronous staging of the sampled records (DrifterWriter copies each record synchronously).
"""
import json
import os

import numpy as np
import torch

from . import _lib
from .grids import LatitudeLongitudeGrid, RectilinearGrid, RightFolded, TileGrid
from .output import GrowableNpy

CLAMPED_X, CLAMPED_Y, HELD, LOST, INACTIVE = (_lib.DRIFTER_CLAMPED_X, _lib.DRIFTER_CLAMPED_Y, _lib.DRIFTER_HELD, _lib.DRIFTER_LOST,
                                              _lib.DRIFTER_INACTIVE)
STATUS_BITS = (("clamped_x", CLAMPED_X), ("clamped_y", CLAMPED_Y), ("held", HELD), ("lost", LOST), ("inactive", INACTIVE))
COLUMNS = ("xi", "eta", "u", "v", "h", "aice", "hs")      # bit k of csi_drifters_sample's column mask; a record's rows are in this order


def column_mask(names):
    """The column mask of csi_drifters_sample for a set of column names ("ℵ" is "aice"); unknown names raise by name."""
    mask = 0
    for n in names:
        n = "aice" if n in ("ℵ", "א") else n
        if n not in COLUMNS:
            raise ValueError(f"drifters: unknown column {n!r} (columns: {', '.join(COLUMNS)}; derived and momentum term fields are not sampled)")
        mask |= 1 << COLUMNS.index(n)
    if mask == 0:
        raise ValueError("drifters: no columns")
    return mask


def columns_of(mask):
    return [n for k, n in enumerate(COLUMNS) if mask & (1 << k)]


def _refuse_grid(grid, who):
    if isinstance(grid, TileGrid):
        raise NotImplementedError(f"{who}: tiled models are not supported (a drifter would have to migrate between ranks)")
    if grid.topology[1] is RightFolded:
        raise NotImplementedError(f"{who}: RightFolded grids are not supported (crossing the fold re-orients the drifter)")


class Drifters:
    """Drifters(grid, xi, eta, device = None, substeps = 1): n drifters at the index-space positions (xi, eta), 1-D arrays of equal length.

    xi, eta, status   torch tensors (float64, float64, int32) on `device`; advance moves them to the model's device the first time
    substeps          midpoint sub-steps per advance that time_step asks for when the object is a model's `drifters`
    """

    def __init__(self, grid, xi, eta, device=None, substeps=1):
        _refuse_grid(grid, "Drifters")
        x = np.ascontiguousarray(xi, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(eta, dtype=np.float64).reshape(-1)
        if x.shape != y.shape:
            raise ValueError("Drifters: xi and eta must have the same length")
        if int(substeps) < 1:
            raise ValueError("Drifters: substeps >= 1")
        self.grid, self.substeps = grid, int(substeps)
        self.xi = torch.from_numpy(x.copy()).to(device)
        self.eta = torch.from_numpy(y.copy()).to(device)
        self.status = torch.zeros(x.size, dtype=torch.int32, device=device)
        self._settle()

    # ---- seeding
    @classmethod
    def at_cell_centers(cls, grid, stride=1, where=None, **kw):
        """One drifter at the centre of every stride-th cell in each direction (cells 1, 1 + stride, ...), in grid order (x fastest);
        where: an (Ny, Nx) boolean array, only cells in which it holds are seeded."""
        sx, sy = (stride, stride) if np.isscalar(stride) else stride
        if int(sx) < 1 or int(sy) < 1:
            raise ValueError("Drifters.at_cell_centers: stride >= 1")
        i, j = np.arange(0, grid.Nx, int(sx)), np.arange(0, grid.Ny, int(sy))
        I, J = np.meshgrid(i, j)
        if where is not None:
            w = np.asarray(where, dtype=bool)
            if w.shape != (grid.Ny, grid.Nx):
                raise ValueError("Drifters.at_cell_centers: `where` must have the shape (Ny, Nx)")
            keep = w[J, I]
            I, J = I[keep], J[keep]
        return cls(grid, I.ravel() + 0.5, J.ravel() + 0.5, **kw)

    @classmethod
    def from_coordinates(cls, grid, x, y, **kw):
        """Drifters at the coordinates (x, y) of a RectilinearGrid (metres) or a LatitudeLongitudeGrid (degrees): the index-space
        position is (x - x0) / dx, one subtraction and one division per coordinate.  Other grids raise: their nodes are not a
        formula of the index."""
        x0, dx, y0, dy = _regular_axes(grid, "Drifters.from_coordinates")
        return cls(grid, (np.asarray(x, dtype=np.float64) - x0) / dx, (np.asarray(y, dtype=np.float64) - y0) / dy, **kw)

    def coordinates(self):
        """(x, y) of the drifters on the host: x0 + xi * dx, one product and one sum per coordinate (RectilinearGrid,
        LatitudeLongitudeGrid; other grids raise).  Lost drifters give NaN."""
        x0, dx, y0, dy = _regular_axes(self.grid, "Drifters.coordinates")
        xi, eta, _ = self.numpy()
        return x0 + xi * dx, y0 + eta * dy

    # ---- plumbing
    @property
    def n(self):
        return int(self.xi.numel())

    def _settle(self):
        if self.xi.is_cuda:      # torch wrote on ITS stream, the library works on its own
            torch.cuda.current_stream(self.xi.device).synchronize()

    def to(self, device):
        if self.xi.device != torch.device(device):
            self.xi, self.eta, self.status = self.xi.to(device), self.eta.to(device), self.status.to(device)
            self._settle()
        return self

    def _struct(self):
        return _lib.Drifters(self.n, self.xi.data_ptr() if self.n else None, self.eta.data_ptr() if self.n else None,
                             self.status.data_ptr() if self.n else None)

    def _check(self, model, who):
        _refuse_grid(model.grid, who)
        g, mg = self.grid, model.grid
        if (g.Nx, g.Ny) != (mg.Nx, mg.Ny) or tuple(g.topology) != tuple(mg.topology):
            raise ValueError(f"{who}: the drifters were made for another grid than the model's")
        self.to(model.device)

    def numpy(self, model=None):
        """(xi, eta, status) as host arrays; model: wait for its stream first (an advance may be in flight)."""
        if model is not None:
            model.synchronize()
        return self.xi.detach().cpu().numpy(), self.eta.detach().cpu().numpy(), self.status.detach().cpu().numpy()

    # ---- the two device calls
    def advance(self, model, dt, substeps=1):
        """csi_drifters_advance: `substeps` midpoint sub-steps of dt / substeps on the model's current velocities, ONE launch on the
        model's stream; nothing is waited for."""
        self._check(model, "Drifters.advance")
        model.ctx.drifters_advance(self._struct(), dt, substeps)
        return self

    def sample(self, model, *names):
        """csi_drifters_sample: the named columns ("xi", "eta", "u", "v", "h", "aice", "hs") at the current positions as a
        (columns, n) float64 tensor on the device, rows in the order of COLUMNS whatever order they were named in; ONE launch on the
        model's stream, nothing is waited for (call model.synchronize() before reading it)."""
        self._check(model, "Drifters.sample")
        mask = column_mask(names or COLUMNS[:4])
        if mask & (1 << COLUMNS.index("hs")) and model.snow_thickness is None:
            raise ValueError("Drifters.sample: column 'hs' needs a model with a snow layer")
        out = torch.empty((len(columns_of(mask)), self.n), dtype=torch.float64, device=model.device)
        torch.cuda.current_stream(model.device).synchronize()
        model.ctx.drifters_sample(self._struct(), mask, out.data_ptr() if self.n else None, self.n)
        return out

    def status_counts(self, model=None):
        """How many drifters carry each status bit after the last advance: dict(free, clamped_x, clamped_y, held, lost, inactive)."""
        st = self.numpy(model)[2]
        out = {"free": int((st == 0).sum())}
        out.update({name: int(((st & bit) != 0).sum()) for name, bit in STATUS_BITS})
        return out

    # ---- checkpoints (model.prognostic_state / restore_prognostic_state)
    def state(self, model=None):
        xi, eta, st = self.numpy(model)
        return {"drifters.xi": xi.copy(), "drifters.eta": eta.copy(), "drifters.status": st.copy()}

    def restore(self, state, model=None):
        if model is not None:
            model.synchronize()
        for key, t in (("drifters.xi", self.xi), ("drifters.eta", self.eta), ("drifters.status", self.status)):
            a = np.ascontiguousarray(state[key], dtype=np.float64 if t.dtype == torch.float64 else np.int32)
            if a.shape != tuple(t.shape):
                raise ValueError(f"restore_prognostic_state: {key} has {a.size} entries, the model's drifters {t.numel()}")
            t.copy_(torch.from_numpy(a))
        self._settle()


def _regular_axes(grid, who):
    if isinstance(grid, RectilinearGrid):
        return grid.x[0], grid.dx, grid.y[0], grid.dy
    if isinstance(grid, LatitudeLongitudeGrid):
        return grid.longitude[0], grid.dlam, grid.latitude[0], grid.dphi
    raise NotImplementedError(f"{who}: a RectilinearGrid or a LatitudeLongitudeGrid is needed; on a curvilinear grid "
                              f"({type(grid).__name__}) the nodes are not a formula of the index (seed with index-space positions)")


class DrifterWriter:
    """DrifterWriter(drifters, schedule, dir, columns = ("xi", "eta"), overwrite_existing = False): tracks as growable .npy files.

    Implements the begin / after_step protocol of model.output_writers; schedule: IterationInterval or TimeInterval (output.py).  Files:
    `dir/<column>.npy` of shape (records, n) float64, `status.npy` (records, n) int32, `time.npy`, `iteration.npy`, `meta.json`; after
    every record each is a valid NPY file.  A record is sampled by ONE launch and copied to the host SYNCHRONOUSLY (the writer waits
    for the model's stream): asynchronous staging of drifter records is not built.  sampler: a stand-in for the device call in tests,
    (drifters, model, names) -> (columns, n) array."""

    def __init__(self, drifters, schedule, dir, columns=("xi", "eta"), overwrite_existing=False, sampler=None):
        if getattr(schedule, "averaged", False):
            raise NotImplementedError("DrifterWriter: time averages of drifter records are not built; IterationInterval or TimeInterval")
        self.drifters, self.schedule, self.dir = drifters, schedule, dir
        self.names = columns_of(column_mask(columns))
        self.sampler = sampler
        files = self.names + ["status", "time", "iteration"]
        if os.path.exists(dir):
            if not overwrite_existing:
                raise FileExistsError(f"DrifterWriter: {dir} exists (overwrite_existing = False)")
            for n in files:
                if os.path.exists(os.path.join(dir, n + ".npy")):
                    os.remove(os.path.join(dir, n + ".npy"))
        os.makedirs(dir, exist_ok=True)
        n = drifters.n
        self.files = {c: GrowableNpy(os.path.join(dir, c + ".npy"), "<f8", (n,)) for c in self.names}
        self.status_file = GrowableNpy(os.path.join(dir, "status.npy"), "<i4", (n,))
        self.time_file = GrowableNpy(os.path.join(dir, "time.npy"), "<f8", ())
        self.iteration_file = GrowableNpy(os.path.join(dir, "iteration.npy"), "<i8", ())
        with open(os.path.join(dir, "meta.json"), "w") as fh:
            json.dump({"columns": self.names, "drifters": n, "schedule": schedule.describe(),
                       "grid": {"Nx": drifters.grid.Nx, "Ny": drifters.grid.Ny}}, fh, indent=1)
        self.records = 0
        self._started = False
        self.closed = False

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
        """Force a record of the current positions."""
        if not self._started:
            self._started = True
            self.schedule.attach(model.clock)
            self.schedule.initial(model.clock)
        self._record(model, model.clock.time)

    def _record(self, model, time):
        if self.sampler is not None:
            rec = np.asarray(self.sampler(self.drifters, model, self.names), dtype=np.float64)
            status = self.drifters.numpy()[2]
        else:
            dev = self.drifters.sample(model, *self.names)
            model.synchronize()                      # the synchronous copy: the sampled record and the status
            rec, status = dev.cpu().numpy(), self.drifters.status.cpu().numpy()
        for k, c in enumerate(self.names):
            self.files[c].append(rec[k])
        self.status_file.append(status)
        self.time_file.append(np.float64(time))
        self.iteration_file.append(np.int64(model.clock.iteration))
        self.records += 1

    def flush(self):
        pass                                         # (nothing is in flight: every record is written when it is taken)

    def close(self):
        if self.closed:
            return
        for f in list(self.files.values()) + [self.status_file, self.time_file, self.iteration_file]:
            f.close()
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def load_tracks(dir):
    """The files of a DrifterWriter's directory as a dict: column -> (records, n) array, plus "status", "time", "iteration"."""
    meta = json.load(open(os.path.join(dir, "meta.json")))
    return {n: np.load(os.path.join(dir, n + ".npy")) for n in meta["columns"] + ["status", "time", "iteration"]}
