"""SlabOceanMixedLayer -- the ocean under the ice as data: a bucket of water with a temperature of its own, cooled by the atmosphere
over the open-water fraction, whose heat deficit below freezing grows ice (frazil) and whose heat above freezing melts it from below.
The fixed form of the closure of the reference's examples/freezing_of_a_lake.jl:91-120; include/csi.h (csi_mixed_layer_set) is the
definition, csrc/mixed_layer.hip the kernel.  This module only describes the layer and wires it to a model; no arithmetic happens here.
"""
import ctypes as C

import numpy as np

from . import _lib
from .fields import CenterField, Field
from .time_series import FieldTimeSeries

# input name -> (slot of csi_field_bind, the field's name)
INPUT_SLOTS = {"surface_heat_flux": ("ML_SURFACE_HEAT_FLUX", "ocean_surface_heat_flux"),
               "coefficient": ("ML_COEFFICIENT", "ocean_coefficient"),
               "atmosphere_temperature": ("ML_REFERENCE_TEMPERATURE", "ocean_reference_temperature"),
               "deep_heat_flux": ("ML_DEEP_HEAT_FLUX", "ocean_deep_heat_flux")}


def _is_number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


class SlabOceanMixedLayer:
    """SlabOceanMixedLayer(depth, temperature=0.0, density=1026.0, heat_capacity=3991.0, ice_ocean_exchange_velocity=6e-5,
    surface_heat_flux=None, coefficient=None, atmosphere_temperature=None, deep_heat_flux=None)

    Per cell and step (all fluxes positive upward; include/csi.h has the statement the kernel follows):
        Qow = (surface_heat_flux + coefficient * (To - atmosphere_temperature)) * (1 - aice)      absent terms are not added
        Qio = min(ice_ocean_exchange_velocity * density * heat_capacity * (To - Tf) * aice, all the heat above freezing)   where To > Tf
        To' = To + dt * (deep_heat_flux - Qow - Qio) / (density * heat_capacity * depth), not below Tf: the deficit is frazil, Qfr <= 0
        the ice step's bottom heat flux = Qio + Qfr
    Each flux input is a number, an (Ny, Nx) array, a CenterField or a FieldTimeSeries; coefficient and atmosphere_temperature come
    together (bulk_sensible_heat_flux(...) forms K: pass the LinearHeatFlux it returns as `coefficient`, or its .coefficient);
    temperature is a number or an (Ny, Nx) array.  Give it to SeaIceModel(grid, ..., ocean=...); afterwards
        model.ocean.temperature          the CenterField To (state; its Psi^- copy under SplitRungeKutta3: temperature_minus)
        model.ocean.bottom_heat_flux     the CenterField the layer writes and the ice step reads (also heat_fluxes_used.bottom)
        model.ocean.surface_flux_used    Qow of the last step, allocated and bound the first time it is asked for
    Heat offered as Qio beyond what melts the cell's ice is lost, as any bottom flux is."""

    def __init__(self, depth, temperature=0.0, density=1026.0, heat_capacity=3991.0, ice_ocean_exchange_velocity=6e-5,
                 surface_heat_flux=None, coefficient=None, atmosphere_temperature=None, deep_heat_flux=None):
        for name, value in (("depth", depth), ("density", density), ("heat_capacity", heat_capacity),
                            ("ice_ocean_exchange_velocity", ice_ocean_exchange_velocity)):
            if not _is_number(value) or not np.isfinite(value):
                raise ValueError(f"SlabOceanMixedLayer.{name}: a finite number is needed")
        for name, value in (("depth", depth), ("density", density), ("heat_capacity", heat_capacity)):
            if not value > 0:
                raise ValueError(f"SlabOceanMixedLayer.{name} must be > 0")
        if ice_ocean_exchange_velocity < 0:
            raise ValueError("SlabOceanMixedLayer.ice_ocean_exchange_velocity must be >= 0")
        if type(coefficient).__name__ == "LinearHeatFlux":      # what bulk_sensible_heat_flux returns: K, and Ta unless given here
            if atmosphere_temperature is None:
                atmosphere_temperature = coefficient.reference_temperature
            coefficient = coefficient.coefficient
        if (coefficient is None) != (atmosphere_temperature is None):
            raise ValueError("SlabOceanMixedLayer: coefficient and atmosphere_temperature are given together or not at all")
        self.depth, self.density, self.heat_capacity = float(depth), float(density), float(heat_capacity)
        self.ice_ocean_exchange_velocity = float(ice_ocean_exchange_velocity)
        self.inputs = {"surface_heat_flux": surface_heat_flux, "coefficient": coefficient,
                       "atmosphere_temperature": atmosphere_temperature, "deep_heat_flux": deep_heat_flux}
        for name, value in self.inputs.items():
            self._check_input(name, value)
            if _is_number(value):
                if not np.isfinite(value):
                    raise ValueError(f"SlabOceanMixedLayer.{name} is not finite")
                self.inputs[name] = float(value)
        if isinstance(temperature, (FieldTimeSeries, Field)) or callable(temperature):
            raise ValueError("SlabOceanMixedLayer.temperature: a number or an (Ny, Nx) array is needed (the temperature is state)")
        self.initial_temperature = float(temperature) if _is_number(temperature) else np.asarray(temperature, dtype=np.float64)
        self.temperature = self.temperature_minus = self.bottom_heat_flux = None
        self.fields = {}                 # input name -> CenterField of the inputs that are per cell
        self._surface_flux_used = None
        self._model = None

    @staticmethod
    def _check_input(name, value):
        if value is None or _is_number(value) or isinstance(value, (Field, FieldTimeSeries, np.ndarray, list)):
            return
        if callable(value) or type(value).__name__ == "FluxFunction":
            raise NotImplementedError(f"SlabOceanMixedLayer.{name}: {type(value).__name__} is not supported -- FluxFunction and other "
                                      "callables cannot cross the C ABI; give a number, an (Ny, Nx) array, a CenterField or a "
                                      "FieldTimeSeries")
        raise TypeError(f"SlabOceanMixedLayer.{name}: unsupported {type(value).__name__}")

    # ---- what the C ABI is told ---------------------------------------------------------------------------------------------------
    def per_cell(self, name):
        v = self.inputs[name]
        return v is not None and not _is_number(v)

    def flags(self):
        """csi_mixed_layer_params.flags: which terms of Qs exist and which inputs are per cell.  The bulk pair is per cell as soon as
        one of the two is (the number is broadcast into an array)."""
        i = self.inputs
        f = 0
        if i["surface_heat_flux"] is not None:
            f |= _lib.ML_HAS_SURFACE | (_lib.ML_SURFACE_ARRAY if self.per_cell("surface_heat_flux") else 0)
        if i["coefficient"] is not None:
            bulk = self.per_cell("coefficient") or self.per_cell("atmosphere_temperature")
            f |= _lib.ML_HAS_BULK | (_lib.ML_BULK_ARRAYS if bulk else 0)
        if self.per_cell("deep_heat_flux"):
            f |= _lib.ML_DEEP_ARRAY
        return f

    def array_inputs(self):
        """The inputs that travel as arrays, in slot order: [(input name, slot, value)]."""
        f = self.flags()
        names = (["surface_heat_flux"] if f & _lib.ML_SURFACE_ARRAY else []) + \
            (["coefficient", "atmosphere_temperature"] if f & _lib.ML_BULK_ARRAYS else []) + (["deep_heat_flux"] if f & _lib.ML_DEEP_ARRAY else [])
        return [(n, INPUT_SLOTS[n][0], self.inputs[n]) for n in names]

    def series_slots(self):
        """The slots of csi_time_series_set this layer's FieldTimeSeries inputs drive."""
        return [slot for _, slot, v in self.array_inputs() if isinstance(v, FieldTimeSeries)]

    def params(self):
        """csi_mixed_layer_params; inputs that are per cell (or absent) leave 0 in their number."""
        arrays = {n for n, _, _ in self.array_inputs()}
        num = lambda n: self.inputs[n] if _is_number(self.inputs[n]) and n not in arrays else 0.0
        return _lib.MixedLayerParams(self.density, self.heat_capacity, self.depth, self.ice_ocean_exchange_velocity,
                                     num("surface_heat_flux"), num("coefficient"), num("atmosphere_temperature"), num("deep_heat_flux"),
                                     self.flags(), 0)

    def check(self, grid, cell_shape_ok):
        """The checks SeaIceModel makes before it touches a device: shapes of the per-cell inputs and of the temperature."""
        for name, _, value in self.array_inputs():
            if not _is_number(value) and not cell_shape_ok(value, grid):
                raise ValueError(f"SlabOceanMixedLayer.{name}: a number, an array of shape (Ny, Nx) = {(grid.Ny, grid.Nx)}, a CenterField "
                                 "of the grid or a FieldTimeSeries of that shape is needed")
        if not _is_number(self.initial_temperature) and not cell_shape_ok(self.initial_temperature, grid):
            raise ValueError(f"SlabOceanMixedLayer.temperature: a number or an array of shape (Ny, Nx) = {(grid.Ny, grid.Nx)} is needed")

    # ---- wiring (SeaIceModel._configure_ocean) --------------------------------------------------------------------------------------
    def attach(self, model):
        """Allocate and bind To (and its Psi^- copy under RK3), the per-cell inputs, and describe the layer to the context.  The
        bottom heat-flux array is the model's (it has set the one ARRAY bottom term by now)."""
        if self._model is not None and self._model is not model:
            raise ValueError("this SlabOceanMixedLayer belongs to another model (its temperature is that model's state)")
        self._model = model
        g, dev = model.grid, model.device
        self.temperature = model._cell_field(self.initial_temperature, "ocean_temperature")
        model._bind("ML_TEMPERATURE", self.temperature)
        if model.timestepper.Psi_minus is not None:
            self.temperature_minus = CenterField(g, dev, "ocean_temperature-")
            model._bind("ML_TEMPERATURE_M", self.temperature_minus)
        self.bottom_heat_flux = model.external_heat_fluxes.bottom
        for name, slot, value in self.array_inputs():
            fld = model._cell_field(value, INPUT_SLOTS[name][1])
            model._bind(slot, fld)
            self.fields[name] = fld
        self._params = self.params()
        model.ctx.call("csi_mixed_layer_set", C.byref(self._params))

    @property
    def surface_flux_used(self):
        """The CenterField into which every mixed-layer step writes the open-water surface flux Qow it used (W m^-2 per cell area).
        Allocated and bound the first time it is asked for.  Read it after the step (synchronize() first)."""
        if self._model is None:
            raise ValueError("surface_flux_used needs a model: SeaIceModel(grid, ..., ocean=this)")
        self._surface_flux_used = self._model._lazy_slot_field("ML_SURFACE_FLUX_USED", "ocean_surface_flux_used")
        return self._surface_flux_used

    def state_fields(self):
        """What a checkpoint carries: To and its Psi^- copy."""
        out = {"ocean.temperature": self.temperature}
        if self.temperature_minus is not None:
            out["ocean.temperature_minus"] = self.temperature_minus
        return out

    def bound_fields(self):
        """name -> (Field, slot) of what this layer has bound (output.bound_fields)."""
        out = {"ocean.temperature": (self.temperature, "ML_TEMPERATURE")}
        if self.temperature_minus is not None:
            out["ocean.temperature_minus"] = (self.temperature_minus, "ML_TEMPERATURE_M")
        for name, fld in self.fields.items():
            out["ocean." + name] = (fld, INPUT_SLOTS[name][0])
        if self._surface_flux_used is not None:
            out["ocean.surface_flux_used"] = (self._surface_flux_used, "ML_SURFACE_FLUX_USED")
        return out


def check_ocean(grid, ocean, ice_thermodynamics, bottom_heat_flux, cell_shape_ok):
    """Refuse, by name, what SeaIceModel(ocean=...) cannot take -- before a device is touched."""
    if ocean is None:
        return
    if not isinstance(ocean, SlabOceanMixedLayer):
        raise TypeError(f"ocean: a SlabOceanMixedLayer is needed, got {type(ocean).__name__} (closures cannot cross the C ABI)")
    if ice_thermodynamics is None:
        raise ValueError("ocean: a SlabOceanMixedLayer needs ice_thermodynamics (the liquidus and the bottom salinity are the ice's)")
    given = bottom_heat_flux if bottom_heat_flux is not None else ice_thermodynamics.bottom_heat_flux
    if isinstance(given, str) and given == "frazil":
        raise ValueError('bottom_heat_flux = "frazil" beside ocean: the mixed layer is what forms frazil; leave bottom_heat_flux out')
    if given is not None:
        raise ValueError("bottom_heat_flux is given beside ocean: the mixed layer computes the ice's bottom heat flux; a coupler with "
                         "its own ocean keeps bottom_heat_flux and leaves ocean out")
    ocean.check(grid, cell_shape_ok)
