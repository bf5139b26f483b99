"""Output writers of a SeaIceModel: schedules, the device recorder, growable NPY files.

Stands where the reference attaches `JLD2Writer(model, outputs; schedule = IterationInterval(5), ...)` to a Simulation
(examples/ice_advected_by_anticyclone.jl:161-163, test/distributed_tests_utils.jl:159).  A record is packed on the device by ONE launch
and crosses the bus on the library's copy stream while the model steps on (include/csi.h, csi_output_*); time averages are summed on
the device.  The writer only touches a record on the host when it needs the slot again, or at close().

IterationInterval, TimeInterval, AveragedTimeInterval   Oceananigans' schedules (RECALLED: Oceananigans is not vendored; each docstring
                                                        is the definition)
OutputWriter      model.output_writers["name"] = OutputWriter(model, outputs, schedule, dir, ...); time_step drives it
aligned_time_step min(dt, next output time - time): a run that lands on its output times
load_output       the files of a directory (the rank directories of a tiled run reassembled) as arrays

Files: `dir/<name>.npy` per output, shape (records, ny, nx), plus time.npy, iteration.npy (one entry per record) and meta.json.
Each .npy has a fixed 128-byte header whose first extent is a fixed-width number, patched after every record: after every record the
file is a valid NPY file that np.load reads, mmap_mode included.  A tiled model writes `dir/rank_<r>/` per rank, no communication.

Not kept in checkpoints: a restored model's writer starts a fresh averaging window (attach a new writer, or accept the shorter first
window).  File writes happen on the calling thread.
"""
import json
import math
import os
import struct
from collections import deque

import numpy as np

from . import _lib
from .grids import Center, TileGrid

_NPY_HEADER = 128
_RESERVED = ("time", "iteration", "meta")


# ---- schedules ------------------------------------------------------------------------------------------------------------------------
class IterationInterval:
    """IterationInterval(n) (RECALLED; this statement is the definition): a record whenever clock.iteration is a multiple of n,
    iteration 0 included when the writer is first driven at it."""
    averaged = False

    def __init__(self, interval):
        if int(interval) != interval or interval < 1:
            raise ValueError("IterationInterval: a whole number >= 1")
        self.interval = int(interval)

    def attach(self, clock):
        pass

    def initial(self, clock):
        return clock.iteration % self.interval == 0

    def after_step(self, clock, dt):
        return [("write", clock.time)] if clock.iteration % self.interval == 0 else []

    def next_time(self, clock):
        return math.inf

    def describe(self):
        return {"kind": "IterationInterval", "interval": self.interval}


class TimeInterval:
    """TimeInterval(interval) (RECALLED; this statement is the definition): `next` starts at the time the writer is first driven at,
    where it fires (the initial record).  After a step that ends at `time`: if time >= next, ONE record, then
    next += interval while next <= time -- a step that overshoots several intervals gives one record."""
    averaged = False

    def __init__(self, interval):
        if not (interval > 0 and math.isfinite(interval)):
            raise ValueError("TimeInterval: a finite interval > 0")
        self.interval = float(interval)
        self.next = None

    def attach(self, clock):
        self.next = float(clock.time)

    def _advance(self, time):
        while self.next <= time:
            self.next += self.interval

    def initial(self, clock):
        self._advance(clock.time)
        return True

    def after_step(self, clock, dt):
        if clock.time >= self.next:
            self._advance(clock.time)
            return [("write", clock.time)]
        return []

    def next_time(self, clock):
        return self.next

    def describe(self):
        return {"kind": "TimeInterval", "interval": self.interval}


class AveragedTimeInterval:
    """AveragedTimeInterval(interval, window = interval) (RECALLED; this statement is the definition).  t_out starts one interval
    after the time the writer is first driven at.  The state at the END of a step that covers (t - dt, t] enters the average of the
    window (t_out - window, t_out] with weight

        w = min(t, t_out) - max(t - dt, t_out - window)          (the length of the overlap; the step is skipped if w <= 0)

    and the record -- sum(w x) / sum(w) -- is written once t >= t_out; then t_out += interval and the SAME step is weighed against the
    new window (a step that overshoots belongs to both; one that overshoots several intervals gives several records).  There is no
    initial record.  Oceananigans keeps a running mean instead of a weighted sum divided by the sum of the weights: the two differ by
    rounding only."""
    averaged = True

    def __init__(self, interval, window=None):
        window = interval if window is None else window
        if not (interval > 0 and math.isfinite(interval)) or not (0 < window <= interval):
            raise ValueError("AveragedTimeInterval: a finite interval > 0 and 0 < window <= interval")
        self.interval, self.window = float(interval), float(window)
        self.t_out = None
        self._open = False           # something has been accumulated since the last record

    def attach(self, clock):
        self.t_out = float(clock.time) + self.interval

    def initial(self, clock):
        return False

    def after_step(self, clock, dt):
        t, t0 = float(clock.time), float(clock.time) - float(dt)
        actions, pending = [], self._open
        while True:
            w = min(t, self.t_out) - max(t0, self.t_out - self.window)
            if w > 0:
                actions.append(("accumulate", w))
                pending = True
            if t < self.t_out:
                break
            if pending:
                actions.append(("write", self.t_out))
                pending = False
            self.t_out += self.interval
        self._open = pending
        return actions

    def next_time(self, clock):
        return self.t_out

    def describe(self):
        return {"kind": "AveragedTimeInterval", "interval": self.interval, "window": self.window}


def aligned_time_step(model, dt):
    """min(dt, next output time - time) over the model's writers, so that a run lands on its output times (iteration schedules never
    shorten a step)."""
    out = float(dt)
    for w in model.output_writers.values():
        gap = w.next_time(model) - model.clock.time
        if 0 < gap < out:
            out = gap
    return out


# ---- which fields a model has bound ----------------------------------------------------------------------------------------------------
_STATE_SLOTS = {"u": "U", "v": "V", "h": "H", "aice": "A", "hs": "HS",
                "Gn.h": "GH", "Gn.aice": "GA", "Gn.u": "GU", "Gn.v": "GV", "Gn.hs": "GHS",
                "Psi_minus.h": "HM", "Psi_minus.aice": "AM", "Psi_minus.u": "UM", "Psi_minus.v": "VM", "Psi_minus.hs": "HSM",
                "dynamics.s11": "S11", "dynamics.s22": "S22", "dynamics.s12": "S12", "dynamics.un": "UN", "dynamics.vn": "VN",
                "dynamics.P": "P", "dynamics.alpha": "ALPHA", "dynamics.Delta": "DELTA", "dynamics.zeta_f": "ZETA_F",
                "dynamics.zeta_c": "ZETA_C",
                "mass_fluxes.ice": "MASS_FLUX", "mass_fluxes.snow": "MASS_FLUX_SNOW",
                "mass_fluxes.intercepted_snowfall": "SNOWFALL_INTERCEPTED",
                "ice_thermodynamics.top_surface_temperature": "TU", "snow_thermodynamics.top_surface_temperature": "TUS"}
_SHORT = {"sigma11": "dynamics.s11", "sigma22": "dynamics.s22", "sigma12": "dynamics.s12"}


def bound_fields(model):
    """name -> (Field, slot of csi_field_bind) of every field the model has bound to its context: the names of _state_fields(model),
    the stress / external-velocity arrays ("top_u", ...), model.forcing ("forcing_u", "forcing_v"), the prescribed free-drift fields,
    the array terms of the heat fluxes and a per-cell snowfall, the mixed layer's "ocean.temperature", its per-cell inputs and, once
    allocated, "ocean.surface_flux_used"; "sigma11" / "sigma22" / "sigma12" are short for "dynamics.s11" ..."""
    from .fields import Field
    from .model import _state_fields
    out = {}
    for name, f in _state_fields(model).items():
        if name in _STATE_SLOTS:
            out[name] = (f, _STATE_SLOTS[name])
    for short, long in _SHORT.items():
        if long in out:
            out[short] = out[long]
    for slot, f in model._stress_fields.items():
        out[slot.lower()] = (f, slot)
    if getattr(model, "forcing_fields", None) is not None:
        out["forcing_u"], out["forcing_v"] = (model.forcing_fields.u, "FORCING_U"), (model.forcing_fields.v, "FORCING_V")
    for comp, f in model._free_drift_fields.items():
        out[f"free_drift_{comp.lower()}"] = (f, f"FREE_DRIFT_{comp}")
    for side, slot in (("top", "TOP_HEAT_FLUX"), ("bottom", "BOTTOM_HEAT_FLUX")):
        f = getattr(model.external_heat_fluxes, side, None)
        if isinstance(f, Field):
            out[f"{side}_heat_flux"] = (f, slot)
    if isinstance(model.snowfall, Field):
        out["snowfall"] = (model.snowfall, "SNOWFALL")
    if getattr(model, "linear_heat_flux", None) is not None:      # the LinearHeatFlux term's per-cell K and Ta
        out["flux_coefficient"] = (model.linear_heat_flux.coefficient, "FLUX_COEFFICIENT")
        out["flux_reference_temperature"] = (model.linear_heat_flux.reference_temperature, "FLUX_REFERENCE_TEMPERATURE")
    if getattr(model, "bottom_salinity", None) is not None:
        out["bottom_salinity"] = (model.bottom_salinity, "BOTTOM_SALINITY")
    if getattr(model, "_heat_fluxes_used", None) is not None:     # the used-flux outputs, once allocated (model.heat_fluxes_used)
        out["top_heat_flux_used"] = (model._heat_fluxes_used.top, "TOP_HEAT_FLUX_USED")
        out["bottom_heat_flux_used"] = (model._heat_fluxes_used.bottom, "BOTTOM_HEAT_FLUX_USED")
    if getattr(model, "shortwave_flux", None) is not None:        # the ShortwaveRadiation term's per-cell flux
        out["shortwave"] = (model.shortwave_flux, "SHORTWAVE")
    if getattr(model, "_albedo_used", None) is not None:          # the albedo a step used, once allocated (model.albedo_used)
        out["albedo_used"] = (model._albedo_used, "ALBEDO_USED")
    if getattr(model, "ocean", None) is not None:                 # the mixed layer: its temperature, per-cell inputs, Qow once allocated
        out.update(model.ocean.bound_fields())
    from .derived import slot_of
    for name, f in getattr(model, "_derived_fields", {}).items():      # derived fields, once allocated (model.derived_field)
        out[name] = (f, slot_of(name))
    from .momentum_terms import slot_of as term_slot_of
    for name, f in getattr(model, "_momentum_term_fields", {}).items():      # momentum term fields, once allocated (model.momentum_term)
        out[name] = (f, term_slot_of(name))
    for k, (name, f) in enumerate(getattr(model, "tracers", {}).items()):      # advected tracers (tracers.py): CSI_TRACER_FIELD(k), no slot
        out[name] = (f, f"TRACER:{k}")
    return out


class DeviceRecorder:
    """The device part of a writer: one output set of the model's context (include/csi.h).  specs: [(slot, dtype "f32" | "f64", averaged,
    masked, fill_value)].  tests/output_ref.py holds a NumPy stand-in with the same methods."""
    bound_fields = staticmethod(bound_fields)

    def __init__(self, model, specs, slots):
        self.ctx = model.ctx
        self.handle = self.ctx.output_create([(s, _lib.OUT_F32 if d == "f32" else _lib.OUT_F64, a, m, v) for s, d, a, m, v in specs], slots)
        self.layout = [self.ctx.output_layout(self.handle, k) for k in range(len(specs))]

    def accumulate(self, w):
        self.ctx.output_accumulate(self.handle, w)

    def snapshot(self):
        return self.ctx.output_snapshot(self.handle)

    def wait(self, slot):
        return self.ctx.output_wait(self.handle, slot)

    def release(self, slot):
        self.ctx.output_release(self.handle, slot)

    def close(self):
        if self.handle and self.ctx.h:
            self.ctx.output_destroy(self.handle)
        self.handle = 0


# ---- growable NPY files ----------------------------------------------------------------------------------------------------------------
def _npy_header(descr, count, tail):
    """The 128-byte header of a version-1.0 NPY file of shape (count,) + tail, the count as a 20-character number."""
    shape = f"({count:20d}, " + "".join(f"{n}, " for n in tail) + ")"
    text = f"{{'descr': '{descr}', 'fortran_order': False, 'shape': {shape}, }}"
    if len(text) + 11 > _NPY_HEADER:
        raise ValueError("NPY header does not fit into 128 bytes")
    text = text + " " * (_NPY_HEADER - 11 - len(text)) + "\n"
    return b"\x93NUMPY\x01\x00" + struct.pack("<H", _NPY_HEADER - 10) + text.encode("latin1")


class GrowableNpy:
    """An NPY file of shape (records,) + tail that grows by one record at a time and is a valid NPY file after each of them."""

    def __init__(self, path, descr, tail):
        self.descr, self.tail, self.count = descr, tuple(int(n) for n in tail), 0
        self.f = open(path, "w+b")
        self.f.write(_npy_header(descr, 0, self.tail))
        self.f.flush()

    def append(self, record):
        a = np.ascontiguousarray(record, dtype=np.dtype(self.descr)).reshape(np.shape(record))      # (ascontiguousarray makes 0-d 1-d)
        assert a.shape == self.tail, (a.shape, self.tail)
        self.f.seek(0, os.SEEK_END)
        self.f.write(a.tobytes())
        self.count += 1
        self.f.seek(0)
        self.f.write(_npy_header(self.descr, self.count, self.tail))       # the data first, then the extent
        self.f.flush()

    def close(self):
        if self.f:
            self.f.close()
            self.f = None


# ---- the writer -----------------------------------------------------------------------------------------------------------------------
class OutputWriter:
    """OutputWriter(model, outputs, schedule, dir, dtype = "f32", mask = False, fill_value = nan, slots = 2, overwrite_existing = False).

    outputs   a dict name -> Field, or a list of names, of fields the model has bound to its context (bound_fields(model)); anything
              else is refused by name.  The names of the derived fields ("shear", "divergence", ...: derived.py) may appear in a list:
              they are allocated here and computed on the device immediately before every accumulate and snapshot; so are
              the momentum term fields ("top_x", "internal_y", ...: momentum_terms.py)
              "ocean.temperature" and "ocean.surface_flux_used" name the mixed layer's fields (ocean.py); the second is allocated here
              "albedo_used" names the albedo a ShortwaveRadiation term used (model.albedo_used); it is allocated here
    schedule  IterationInterval, TimeInterval (snapshots) or AveragedTimeInterval (every output is a time average)
    dtype     "f32" (round to nearest even on the device) or "f64"
    mask      True: (Center, Center) outputs take fill_value in the inactive cells of the model's mask
    slots     records that may be in flight; the writer waits for the oldest one only when it needs its slot again

    Attach it with model.output_writers[key] = writer.  time_step drives it: before the first step it writes the initial state if
    the schedule fires at that clock (the reference examples' iteration-0 record; averaged schedules have none), after every step --
    clock advanced, tiles validated -- it accumulates and writes what the schedule asks for.  write(model) forces a record;
    close() (or leaving a `with` block) drains every slot and closes the files."""

    def __init__(self, model, outputs, schedule, dir, dtype="f32", mask=False, fill_value=math.nan, slots=2, overwrite_existing=False,
                 recorder=None):
        if dtype not in ("f32", "f64"):
            raise ValueError("OutputWriter: dtype must be 'f32' or 'f64'")
        if int(slots) < 1:
            raise ValueError("OutputWriter: slots >= 1")
        if type(model).__name__ == "EnthalpyMethodSeaIceModel":
            raise NotImplementedError("OutputWriter: an output writer over the column fields of an EnthalpyMethodSeaIceModel is not built; "
                                      "read them with ColumnField.interior_numpy() between time_steps calls")
        recorder = recorder or DeviceRecorder
        from .derived import DERIVED_NAMES, name_of_slot
        if not isinstance(outputs, dict) and hasattr(model, "derived_field"):
            for name in outputs:                     # a derived field named in a list is allocated and bound here
                if name in DERIVED_NAMES:
                    model.derived_field(name)
        from .momentum_terms import TERM_FIELD_NAMES, name_of_slot as term_name_of_slot
        if not isinstance(outputs, dict) and hasattr(model, "momentum_term"):
            for name in outputs:                     # ... and so is a momentum term field
                if name in TERM_FIELD_NAMES:
                    model.momentum_term(name)
        if not isinstance(outputs, dict) and "ocean.surface_flux_used" in outputs and getattr(model, "ocean", None) is not None:
            model.ocean.surface_flux_used        # (allocated and bound the first time it is asked for)
        if not isinstance(outputs, dict) and "albedo_used" in outputs and getattr(model, "shortwave", None) is not None:
            model.albedo_used                    # (likewise)
        bound = recorder.bound_fields(model)
        if isinstance(outputs, dict):
            items = []
            for name, fld in outputs.items():
                slot = next((s for f, s in bound.values() if f is fld), None)
                if slot is None:
                    raise ValueError(f"OutputWriter: output {name!r} is not a field the model has bound to its context")
                items.append((str(name), fld, slot))
        else:
            items = []
            for name in outputs:
                if name not in bound:
                    raise ValueError(f"OutputWriter: {name!r} is not a field the model has bound to its context "
                                     f"(bound: {', '.join(sorted(bound))})")
                items.append((str(name), *bound[name]))
        if not items:
            raise ValueError("OutputWriter: no outputs")
        if len(items) > _lib.OUTPUT_MAX_FIELDS:
            raise ValueError(f"OutputWriter: at most {_lib.OUTPUT_MAX_FIELDS} outputs per writer")
        for name, _, _ in items:
            if name in _RESERVED or os.sep in name:
                raise ValueError(f"OutputWriter: {name!r} cannot name an output")
        g = model.grid
        self.schedule, self.dtype, self.slots = schedule, dtype, int(slots)
        self.names = [n for n, _, _ in items]
        # derived outputs: computed (model.compute_derived, one launch) immediately before every accumulate and snapshot; a writer
        # without them makes no such call
        self.derived = tuple(name_of_slot(slot) for _, _, slot in items if name_of_slot(slot) is not None)
        # momentum term outputs likewise (model.compute_momentum_terms, one launch for all of them)
        self.momentum_terms = tuple(term_name_of_slot(slot) for _, _, slot in items if term_name_of_slot(slot) is not None)
        self.dir = os.path.join(dir, f"rank_{g.rank}") if isinstance(g, TileGrid) else dir
        if os.path.exists(self.dir):
            if not overwrite_existing:
                raise FileExistsError(f"OutputWriter: {self.dir} exists (overwrite_existing = False)")
            for n in self.names + ["time", "iteration"]:
                if os.path.exists(os.path.join(self.dir, n + ".npy")):
                    os.remove(os.path.join(self.dir, n + ".npy"))
        os.makedirs(self.dir, exist_ok=True)
        averaged = bool(schedule.averaged)
        specs = [(slot, dtype, averaged, bool(mask) and f.location == (Center, Center), float(fill_value)) for _, f, slot in items]
        self.recorder = recorder(model, specs, self.slots)
        self.layout = list(self.recorder.layout)
        descr = "<f4" if dtype == "f32" else "<f8"
        self.files = {n: GrowableNpy(os.path.join(self.dir, n + ".npy"), descr, (ny, nx)) for n, (_, ny, nx) in zip(self.names, self.layout)}
        self.time_file = GrowableNpy(os.path.join(self.dir, "time.npy"), "<f8", ())
        self.iteration_file = GrowableNpy(os.path.join(self.dir, "iteration.npy"), "<i8", ())
        tiled = isinstance(g, TileGrid)
        meta = {"outputs": [{"name": n, "location": [f.LX.__name__, f.LY.__name__], "dtype": dtype, "shape": [ny, nx],
                             "fill_value": None if not spec[3] else (None if math.isnan(spec[4]) else spec[4]), "masked": spec[3],
                             "averaged": averaged, "offset": [int(getattr(g, "i_off", 0)), int(getattr(g, "j_off", 0))]}
                            for (n, f, _), spec, (_, ny, nx) in zip(items, specs, self.layout)],
                "schedule": schedule.describe(),
                "grid": {"Nx": g.Nx, "Ny": g.Ny, "Hx": g.Hx, "Hy": g.Hy},
                "tile": ({"rank": g.rank, "partition": [g.Rx, g.Ry], "rank_x": g.rx, "rank_y": g.ry,
                          "global": [g.global_grid.Nx, g.global_grid.Ny]} if tiled else None)}
        with open(os.path.join(self.dir, "meta.json"), "w") as fh:
            json.dump(meta, fh, indent=1)
        self.pending = deque()       # (slot, time, iteration) of the records in flight, oldest first
        self.records = 0
        self._started = False
        self.closed = False

    # ---- driven by time_step
    def begin(self, model):
        """Before a step: the first time, start the schedule at the clock and write the initial state if it fires there."""
        if self._started:
            return
        self._started = True
        self.schedule.attach(model.clock)
        if self.schedule.initial(model.clock):
            self._record(model, model.clock.time)

    def after_step(self, model, dt):
        self.begin(model)
        for action, value in self.schedule.after_step(model.clock, dt):
            if action == "accumulate":
                if self.derived:
                    model.compute_derived(*self.derived)
                if self.momentum_terms:
                    model.compute_momentum_terms(*self.momentum_terms)
                self.recorder.accumulate(value)
            else:
                self._record(model, value)

    def next_time(self, model):
        self.begin(model)
        return self.schedule.next_time(model.clock)

    def write(self, model):
        """Force a record of the current state (an averaged writer: of what has been accumulated so far)."""
        if not self._started:             # (the forced record stands for the initial one)
            self._started = True
            self.schedule.attach(model.clock)
            self.schedule.initial(model.clock)
        self._record(model, model.clock.time)

    # ---- records
    def _record(self, model, time):
        if len(self.pending) >= self.slots:
            self._drain_one()
        if self.derived:
            model.compute_derived(*self.derived)
        if self.momentum_terms:
            model.compute_momentum_terms(*self.momentum_terms)
        slot = self.recorder.snapshot()
        self.pending.append((slot, float(time), int(model.clock.iteration)))

    def _drain_one(self):
        slot, time, iteration = self.pending.popleft()
        rec = self.recorder.wait(slot)
        dt = np.float32 if self.dtype == "f32" else np.float64
        for n, (off, ny, nx) in zip(self.names, self.layout):
            self.files[n].append(rec[off:off + ny * nx * np.dtype(dt).itemsize].view(dt).reshape(ny, nx))
        self.time_file.append(np.float64(time))
        self.iteration_file.append(np.int64(iteration))
        self.recorder.release(slot)
        self.records += 1

    def flush(self):
        """Wait for every record in flight and write it."""
        while self.pending:
            self._drain_one()

    def close(self):
        if self.closed:
            return
        self.flush()
        for f in list(self.files.values()) + [self.time_file, self.iteration_file]:
            f.close()
        self.recorder.close()
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _load_dir(d):
    meta = json.load(open(os.path.join(d, "meta.json")))
    out = {o["name"]: np.load(os.path.join(d, o["name"] + ".npy")) for o in meta["outputs"]}
    out["time"] = np.load(os.path.join(d, "time.npy"))
    out["iteration"] = np.load(os.path.join(d, "iteration.npy"))
    return meta, out


def load_output(dir):
    """The files of a writer's directory as a dict: name -> (records, ny, nx) array, plus "time" and "iteration".  A directory of
    rank_<r> sub-directories (a tiled run) is reassembled from their meta.json: every rank's interior at its (i0, j0) offset -- the
    interiors partition the global field, the last face of a Bounded side belongs to the easternmost / northernmost tile."""
    if os.path.exists(os.path.join(dir, "meta.json")):
        return _load_dir(dir)[1]
    ranks = sorted(n for n in os.listdir(dir) if n.startswith("rank_") and os.path.exists(os.path.join(dir, n, "meta.json")))
    if not ranks:
        raise FileNotFoundError(f"load_output: {dir} holds neither meta.json nor rank_<r> directories")
    parts = [_load_dir(os.path.join(dir, n)) for n in ranks]
    out = {"time": parts[0][1]["time"], "iteration": parts[0][1]["iteration"]}
    for meta, data in parts[1:]:
        if not (np.array_equal(data["time"], out["time"]) and np.array_equal(data["iteration"], out["iteration"])):
            raise ValueError("load_output: the ranks' records were not written at the same times")
    for k, o in enumerate(parts[0][0]["outputs"]):
        name = o["name"]
        pieces = [(m["outputs"][k]["offset"], d[name]) for m, d in parts]
        ny = max(j0 + a.shape[1] for (i0, j0), a in pieces)
        nx = max(i0 + a.shape[2] for (i0, j0), a in pieces)
        full = np.zeros((len(out["time"]), ny, nx), dtype=pieces[0][1].dtype)
        seen = np.zeros((ny, nx), dtype=np.int32)
        for (i0, j0), a in pieces:
            full[:, j0:j0 + a.shape[1], i0:i0 + a.shape[2]] = a
            seen[j0:j0 + a.shape[1], i0:i0 + a.shape[2]] += 1
        if not (seen == 1).all():
            raise ValueError(f"load_output: the tiles of {name!r} do not partition the global field")
        out[name] = full
    return out
