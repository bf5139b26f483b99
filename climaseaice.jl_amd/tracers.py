"""Advected ice tracers and ice age (include/csi.h, "advected ice tracers and ice age": that comment is the definition).

    model = csi.SeaIceModel(grid, advection=csi.WENO(order=7), tracers=("dye", csi.IceAge()))
    csi.set_(model, h=..., aice=..., dye=...)
    csi.time_step(model, dt)
    age = model.tracer("age").interior_numpy()

The reference's SeaIceModel(grid; tracers = ...) makes its tracers prognostic fields and never steps them; here every step advects them
on the device with the velocities, scheme, weight dtype and mode of h: a plain tracer like the snow thickness, a tracer weighted by
concentration as the transported quantity aice * c.  The arrays are the model's CenterFields; the library is given them once
(csi_tracers_set) and keeps the dense c* of a stage and the Psi^- copies of an RK3 step itself.

Not built: tiles and multi-GPU; tracer integrals in diagnostics or regions; per-tracer schemes; time-series or array-valued sources;
volume weighting; tracers in the fused advection-only stage launch; tracers as bound slots."""
import ctypes as C
import math

from . import _lib


def _reserved():
    """names a tracer may not take: the keywords of set_, the keys bound_fields can hold (state fields, stress and forcing arrays,
    derived and momentum term fields, ...) and the attributes of the time stepper's G^n -- a tracer of that name would shadow the field"""
    from .derived import DERIVED_NAMES
    from .momentum_terms import TERM_FIELD_NAMES
    from .output import _SHORT, _STATE_SLOTS
    names = {"h", "aice", "hs", "u", "v", "ice_thickness", "ice_concentration", "snow_thickness", "\u2135", "\u05d0", "snowfall", "shortwave",
             "forcing_u", "forcing_v", "free_drift_u", "free_drift_v", "top_heat_flux", "bottom_heat_flux", "flux_coefficient",
             "flux_reference_temperature", "bottom_salinity", "top_heat_flux_used", "bottom_heat_flux_used", "albedo_used", "clock"}
    names |= set(DERIVED_NAMES) | set(TERM_FIELD_NAMES) | set(_SHORT) | {k for k in _STATE_SLOTS if "." not in k}
    names |= {f"{side}_{comp}" for side in ("top", "bot") for comp in ("u", "v")}
    return names


_WEIGHTINGS = {None: _lib.TRACER_PLAIN, "concentration": _lib.TRACER_BY_CONCENTRATION}


class Tracer:
    """Tracer(name, weighting=None | "concentration", nonnegative=True, source=0.0).

    weighting    None: the tracer itself is transported, G = -div(U c), like the snow thickness (a density: it does not stay uniform
                 in divergent flow).  "concentration": aice * c is transported and c recovered with the concentration the same
                 tendencies give, so a uniform c stays uniform and ridging leaves it unchanged.
    nonnegative  clip at zero after the update, as the snow thickness is
    source       a rate per second, added where there is ice (a number)"""

    def __init__(self, name, weighting=None, nonnegative=True, source=0.0):
        if not isinstance(name, str) or not name.isidentifier():
            raise ValueError(f"Tracer: name must be an identifier, got {name!r}")
        if name in _reserved():
            raise ValueError(f"Tracer: the name {name!r} is taken by a field of the model (h, aice, hs, u, v, the names of the derived, momentum "
                             "term, stress and forcing fields, ...)")
        if weighting not in _WEIGHTINGS:
            raise ValueError(f"Tracer {name}: weighting must be None or 'concentration', got {weighting!r}")
        if not isinstance(nonnegative, (bool, int)) or int(nonnegative) not in (0, 1):
            raise ValueError(f"Tracer {name}: nonnegative must be True or False")
        if isinstance(source, bool) or not isinstance(source, (int, float)):
            raise NotImplementedError(f"Tracer {name}: source must be a number (time-series and array-valued sources are not built)")
        if not math.isfinite(source):
            raise ValueError(f"Tracer {name}: source must be finite")
        self.name, self.weighting, self.nonnegative, self.source = name, weighting, bool(nonnegative), float(source)

    def __repr__(self):
        return f"Tracer({self.name!r}, weighting={self.weighting!r}, nonnegative={self.nonnegative}, source={self.source})"


class IceAge(Tracer):
    """IceAge(name="age", units="s" | "days"): the age of the ice, weighted by concentration, nonnegative, growing by one second (or
    1 / 86400 day) per second where there is ice and restarting from zero where the ice vanishes.  Valid to read after a step (a cell
    that became ice during the step holds the step's dt); growth does not dilute it."""

    def __init__(self, name="age", units="s"):
        if units not in ("s", "days"):
            raise ValueError(f"IceAge: units must be 's' or 'days', got {units!r}")
        super().__init__(name, weighting="concentration", nonnegative=True, source=1.0 if units == "s" else 1.0 / 86400.0)
        self.units = units


def tracer_specs(tracers, grid=None):
    """SeaIceModel's `tracers` argument as a list of Tracer: None or () -> []; a bare string is a plain tracer; every error by name."""
    if tracers is None:
        return []
    if isinstance(tracers, (str, Tracer)):
        tracers = (tracers,)
    specs = []
    for t in tracers:
        if isinstance(t, str):
            t = Tracer(t)
        if not isinstance(t, Tracer):
            raise TypeError(f"tracers: a name, a csi.Tracer or a csi.IceAge, got {type(t).__name__}")
        if any(t.name == o.name for o in specs):
            raise ValueError(f"tracers: the name {t.name!r} appears twice")
        specs.append(t)
    if len(specs) > _lib.TRACERS_MAX:
        raise ValueError(f"tracers: at most {_lib.TRACERS_MAX} tracers (CSI_TRACERS_MAX), got {len(specs)}")
    if specs and type(grid).__name__ == "TileGrid":
        raise NotImplementedError("tracers: tiled models (TileGrid) do not take tracers -- tiles and multi-GPU are not built")
    return specs


def tracers_struct(specs, fields, tendencies):
    """The csi_tracers of a model: device addresses of its tracer fields and of their G^n fields, the flags of the specs."""
    t = _lib.Tracers()
    t.n = len(specs)
    for k, s in enumerate(specs):
        t.c[k] = fields[k].data.data_ptr()
        t.G[k] = tendencies[k].data.data_ptr() if tendencies[k] is not None else None
        t.weighting[k] = _WEIGHTINGS[s.weighting]
        t.nonnegative[k] = int(s.nonnegative)
        t.source[k] = s.source
    return t


def attach(model):
    """csi_tracers_set for the model's tracers (called once, by SeaIceModel, after h and aice are bound)."""
    specs = model.tracer_specs
    fields = [model.tracers[s.name] for s in specs]
    tendencies = [getattr(model.timestepper.Gn, s.name) for s in specs]
    model._tracers_struct = tracers_struct(specs, fields, tendencies)      # (kept: the arrays it names are the model's)
    model.ctx.tracers_set(model._tracers_struct)
