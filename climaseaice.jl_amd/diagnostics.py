"""Device diagnostics of a SeaIceModel: advection timescale, integrals, extrema, finite check, and the time-step wizard built on them.

cell_advection_timescale   the method of the reference's root module (src/ClimaSeaIce.jl:63-69) that a TimeStepWizard calls
diagnostics                what the reference's tests and validation scripts reduce on the host (maximum(u), volume and area series,
                           progress lines), computed on the device by csi_diagnostics_compute (include/csi.h): no field is copied
TimeStepWizard             Oceananigans' wizard rule (RECALLED: Oceananigans is not vendored; new_time_step's docstring is the definition)

On a tiled model every call here is COLLECTIVE: all ranks call it between the same two steps and get the same bits.
"""
import math
from dataclasses import dataclass
from types import MappingProxyType

from . import _lib

_GROUPS = {"velocity": _lib.DIAG_VELOCITY, "tracers": _lib.DIAG_TRACERS, "all": _lib.DIAG_ALL}


@dataclass(frozen=True)
class Diagnostics:
    """The result of model.diagnostics(): immutable.  Members of a group that was not requested (and the snow members of a model
    without a snow layer) are None.  Definitions, the summation order of the five sums and the tile combine: include/csi.h."""
    what: tuple                      # the groups computed: ("velocity",), ("tracers",) or both
    has_snow: bool
    extent_threshold: float
    advection_timescale: float = None     # 1 / inv_timescale_max; +inf at rest, NaN iff a velocity is NaN
    inv_timescale_max: float = None
    max_abs_u: float = None
    max_abs_v: float = None
    ice_volume: float = None         # sum (h aice) Az over active cells, m^3
    ice_area: float = None           # sum aice Az
    ice_extent: float = None         # sum Az where aice >= extent_threshold
    snow_volume: float = None        # sum (hs aice) Az
    active_area: float = None        # sum Az
    ice_mass: float = None           # sea_ice_density * ice_volume
    min_h: float = None
    max_h: float = None
    min_aice: float = None
    max_aice: float = None
    max_hs: float = None
    active_cells: int = None
    nonfinite: MappingProxyType = None    # field name -> elements that are NaN or +-Inf (land and the last Bounded faces included)
    nan: MappingProxyType = None          # "u", "v" -> elements that are NaN

    @property
    def finite(self):
        return not any(self.nonfinite.values())


def _what_mask(what):
    if isinstance(what, str):
        if what not in _GROUPS:
            raise ValueError(f"diagnostics: what must be 'all', 'velocity' or 'tracers' (or a tuple of the last two), got {what!r}")
        return _GROUPS[what]
    if isinstance(what, int):
        return what
    mask = 0
    for w in what:
        mask |= _what_mask(w)
    return mask


def diagnostics(model, what="all", extent_threshold=0.15):
    """csi_diagnostics_compute on the model's context: two launches and a 168-byte copy on the library's stream, which it waits for.
    A group whose fields are not bound raises CsiError naming the field (a context without velocities supports "tracers" only)."""
    mask = _what_mask(what)
    d = model.ctx.diagnostics_compute(mask, extent_threshold)
    vel, trc, snow = bool(mask & _lib.DIAG_VELOCITY), bool(mask & _lib.DIAG_TRACERS), bool(d.has_snow)
    kw, nonfinite, nan = {}, {}, {}
    if vel:
        kw.update(advection_timescale=d.advection_timescale, inv_timescale_max=d.inv_timescale_max, max_abs_u=d.max_abs_u,
                  max_abs_v=d.max_abs_v)
        nonfinite.update(u=d.nonfinite_u, v=d.nonfinite_v)
        nan.update(u=d.nan_u, v=d.nan_v)
    if trc:
        kw.update(ice_volume=d.ice_volume, ice_area=d.ice_area, ice_extent=d.ice_extent, active_area=d.active_area,
                  ice_mass=model.sea_ice_density * d.ice_volume, min_h=d.min_h, max_h=d.max_h, min_aice=d.min_aice,
                  max_aice=d.max_aice, active_cells=d.active_cells)
        nonfinite.update(h=d.nonfinite_h, aice=d.nonfinite_aice)
        if snow:
            kw.update(snow_volume=d.snow_volume, max_hs=d.max_hs)
            nonfinite.update(hs=d.nonfinite_hs)
    return Diagnostics(what=tuple(n for n, on in (("velocity", vel), ("tracers", trc)) if on), has_snow=snow,
                       extent_threshold=float(extent_threshold), nonfinite=MappingProxyType(nonfinite), nan=MappingProxyType(nan), **kw)


def cell_advection_timescale(model):
    """cell_advection_timescale(model::SeaIceModel) (src/ClimaSeaIce.jl:63-69): min over the cells of
    1 / (|u| / dx^fc + |v| / dy^cf).  Reads u and v only (the velocity group)."""
    return diagnostics(model, "velocity").advection_timescale


def assert_finite(model):
    """Raise FloatingPointError naming every field that holds NaN or Inf in its interior (land included), with the counts."""
    bad = {k: n for k, n in diagnostics(model, "all").nonfinite.items() if n}
    if bad:
        raise FloatingPointError("non-finite values in " + ", ".join(f"{k} ({n} element{'s' if n != 1 else ''})" for k, n in bad.items())
                                 + f" at iteration {model.clock.iteration}, time {model.clock.time}")


@dataclass(frozen=True)
class TimeStepWizard:
    """TimeStepWizard(cfl = 0.2, max_change = 1.1, min_change = 0.5, max_dt = inf, min_dt = 0): wizard(model, dt) returns the next step
    (new_time_step on the model's advection timescale; one device reduction over u and v)."""
    cfl: float = 0.2
    max_change: float = 1.1
    min_change: float = 0.5
    max_dt: float = math.inf
    min_dt: float = 0.0

    def __call__(self, model, dt):
        return new_time_step(dt, cell_advection_timescale(model), self)


def new_time_step(old_dt, timescale, wizard):
    """Oceananigans' new_time_step (RECALLED; this is the definition):

        dt = cfl * timescale
        dt = min(max_change * old_dt, dt)
        dt = max(min_change * old_dt, dt)
        dt = clamp(dt, min_dt, max_dt)            # max_dt if dt > max_dt, min_dt if dt < min_dt, else dt

    Pure host arithmetic in double.  timescale = +inf (ice at rest) gives max_change * old_dt (clamped); a NaN timescale gives NaN."""
    dt = wizard.cfl * float(timescale)
    if math.isnan(dt):
        return math.nan
    dt = min(wizard.max_change * old_dt, dt)
    dt = max(wizard.min_change * old_dt, dt)
    return wizard.max_dt if dt > wizard.max_dt else (wizard.min_dt if dt < wizard.min_dt else dt)
