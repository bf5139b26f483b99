"""SeaIceModel / set! / time_step! / update_state! -- host-side mirror of the reference API for the
accelerated path.  All arithmetic happens in libcsi_hip.so through the C ABI (include/csi.h).

SeaIceModel       sea_ice_model.jl:22-51,140-297 (fields allocated as :182-200, timestepper :235)
set!              :301-315
time_step!        sea_ice_fe_step.jl:13-34 (ForwardEuler) / upstream SplitRungeKutta3 loop around
                  rk_substep!, sea_ice_rk_substep.jl:81-94
update_state!     sea_ice_model.jl:379-394
"""
import ctypes as C
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .dynamics import (ElastoViscoPlasticRheology, ExplicitSolver, FPlane, FreeDriftVelocities, IceStrength, SeaIceMomentumEquation,
                       SemiImplicitStress, StressBalanceFreeDrift, ViscousRheology)
from .fields import CenterField, Field, XFaceField, YFaceField
from .ocean import SlabOceanMixedLayer, check_ocean
from .time_series import FieldTimeSeries, RegriddedTimeSeries, refuse_series
from .grids import (METRIC_NAMES, Bounded, Center, Face, FullyConnected, LeftConnected, LeftConnectedRightFolded, Periodic, RightConnected,
                    RightFolded, TileGrid)


_OWN = object()      # SlabThermodynamics.params: use the object's own fluxes

# the name _cell_field gives a per-cell input's field -> its series slot, for the inputs older than the shortwave flux
_SERIES_SLOT_OF = {_lib.SLOTS[_lib.slot_id(n)][1]: n for n in _lib.SERIES_SLOTS[8:] + _lib.THERMO_SERIES_SLOTS + _lib.MIXED_LAYER_SERIES_SLOTS}


def series_slot_of(name):
    """The csi_time_series_set slot that a FieldTimeSeries given for the per-cell input `name` drives (KeyError: none does)."""
    slot = _lib.slot_of_display_name(name)
    if not _lib.SLOTS[_lib.slot_id(slot)][3] & _lib.SLOT_SERIES:
        raise KeyError(name)
    return slot


def _cell_shape_ok(value, grid):
    """An (Ny, Nx) array of the grid (on a TileGrid also of the global grid) or a CenterField of the grid."""
    if isinstance(value, Field):
        return value.location == (Center, Center) and (value.ni, value.nj) == tuple(grid.field_size(Center, Center))
    if isinstance(value, FieldTimeSeries):      # (cut to the tile when it was built)
        return value.location == (Center, Center) and value.interior_shape == (grid.Ny, grid.Nx)
    shape = np.shape(value)
    if isinstance(grid, TileGrid) and shape == (grid.global_grid.Ny, grid.global_grid.Nx):
        return True
    return shape == (grid.Ny, grid.Nx)


def check_heat_flux(spec, side, grid):
    """Refuse, by name, what the C ABI cannot take: closures (FluxFunction, callables), RadiativeEmission, LinearHeatFlux or
    ShortwaveRadiation at the bottom, more than one array, LinearHeatFlux or ShortwaveRadiation per side, arrays of the wrong shape
    (ValueError)."""
    if spec is None or _is_number(spec) or (side == "bottom" and isinstance(spec, str) and spec == "frazil"):
        return
    items = spec if isinstance(spec, tuple) else (spec,)
    if len(items) > _lib.MAX_HEAT_FLUX_TERMS:
        raise NotImplementedError(f"{side}_heat_flux: at most {_lib.MAX_HEAT_FLUX_TERMS} terms")
    arrays = linear = shortwave = 0
    for x in items:
        if _is_number(x):
            continue
        if isinstance(x, RadiativeEmission):
            if side != "top":
                raise NotImplementedError("RadiativeEmission is a top heat flux only")
        elif isinstance(x, LinearHeatFlux):
            if side != "top":
                raise NotImplementedError("LinearHeatFlux is a top heat flux only")
            linear += 1
            if linear > 1:
                raise NotImplementedError("top_heat_flux: at most one LinearHeatFlux term (sum the coefficients into one)")
            for name, value in (("coefficient", x.coefficient), ("reference_temperature", x.reference_temperature)):
                if not _is_number(value) and not _cell_shape_ok(value, grid):
                    raise ValueError(f"LinearHeatFlux.{name}: a number, an array of shape (Ny, Nx) = {(grid.Ny, grid.Nx)} or a "
                                     "CenterField of the grid is needed")
        elif isinstance(x, ShortwaveRadiation):
            if side != "top":
                raise NotImplementedError("ShortwaveRadiation is a top heat flux only")
            shortwave += 1
            if shortwave > 1:
                raise NotImplementedError("top_heat_flux: at most one ShortwaveRadiation term (sum the fluxes into one)")
            if not _is_number(x.flux) and not _cell_shape_ok(x.flux, grid):
                raise ValueError(f"ShortwaveRadiation.flux: a number, an array of shape (Ny, Nx) = {(grid.Ny, grid.Nx)}, a CenterField of "
                                 "the grid or a FieldTimeSeries on it is needed")
        elif isinstance(x, (Field, np.ndarray, list, FieldTimeSeries)):
            arrays += 1
            if arrays > 1:
                raise NotImplementedError(f"{side}_heat_flux: at most one array / CenterField term (sum the arrays into one)")
            if not _cell_shape_ok(x, grid):
                raise ValueError(f"{side}_heat_flux: an array of shape (Ny, Nx) = {(grid.Ny, grid.Nx)} or a CenterField of the grid "
                                 f"is needed, got {np.shape(x) if not isinstance(x, Field) else 'a field of another shape'}")
        elif callable(x) or type(x).__name__ == "FluxFunction":
            raise NotImplementedError(f"{side}_heat_flux: {type(x).__name__} is not supported -- FluxFunction and other callables "
                                      "cannot cross the C ABI; give numbers, (Ny, Nx) arrays, CenterFields, RadiativeEmission "
                                      "or a tuple of them; a bulk flux K (T - Ta) is data: LinearHeatFlux, and so is absorbed shortwave with "
                                      "a temperature-dependent albedo: ShortwaveRadiation")
        else:
            raise TypeError(f"{side}_heat_flux: unsupported term {type(x).__name__}")


def check_heat_fluxes(grid, ice, top_heat_flux, bottom_heat_flux, snowfall=None, snow=None):
    """The checks SeaIceModel makes before it touches a device: fluxes given in one place only, and each one acceptable."""
    if top_heat_flux is not None and ice.top_heat_flux is not None:
        raise ValueError("top_heat_flux is given both to SeaIceModel and to SlabThermodynamics")
    if bottom_heat_flux is not None and ice.bottom_heat_flux is not None:
        raise ValueError("bottom_heat_flux is given both to SeaIceModel and to SlabThermodynamics")
    check_heat_flux(top_heat_flux if top_heat_flux is not None else ice.top_heat_flux, "top", grid)
    check_heat_flux(bottom_heat_flux if bottom_heat_flux is not None else ice.bottom_heat_flux, "bottom", grid)
    top = top_heat_flux if top_heat_flux is not None else ice.top_heat_flux
    for x in (top if isinstance(top, tuple) else (top,)):
        if isinstance(x, ShortwaveRadiation) and x.snow_albedo is not None and snow is None:
            raise ValueError("ShortwaveRadiation.snow_albedo is given, but the model has no snow layer (snow_thermodynamics)")
    refuse_series(ice.prescribed, "PrescribedTemperature (the per-cell temperature is also state)")
    for name, value in (("snowfall", snowfall), ("PrescribedTemperature", ice.prescribed), ("bottom_salinity", ice.bottom_salinity)):
        if value is not None and not _is_number(value) and not _cell_shape_ok(value, grid):
            raise ValueError(f"{name}: an array of shape (Ny, Nx) = {(grid.Ny, grid.Nx)} or a CenterField of the grid is needed")


def _is_number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


class ValueBoundaryCondition:
    """Oceananigans ValueBoundaryCondition(value): on a tangential velocity at a wall, value 0 is no-slip.  A number becomes a float;
    anything else -- an (Ny, Nx) array, a FieldTimeSeries: the boundary temperatures of EnthalpyMethodSeaIceModel -- is kept as it
    is, and the velocity conditions of SeaIceModel refuse it by name."""

    def __init__(self, value=0.0):
        self.value = float(value) if np.isscalar(value) else value


class FieldBoundaryConditions:
    """FieldBoundaryConditions(north =, south =, west =, east =, top =, bottom =): sides left out keep the default (no-flux for the
    tangential velocity, impenetrable for the normal one; no-flux for the column model's temperature).  Used as
    SeaIceModel(boundary_conditions = dict(u =, v =)) and EnthalpyMethodSeaIceModel(boundary_conditions = dict(T =))."""

    def __init__(self, north=None, south=None, west=None, east=None, immersed=None, top=None, bottom=None):
        self.north, self.south, self.west, self.east, self.immersed = north, south, west, east, immersed
        self.top, self.bottom = top, bottom


class FluxBoundaryCondition:
    """Oceananigans FluxBoundaryCondition(number)."""

    def __init__(self, value=0.0):
        self.value = float(value)


class ImmersedBoundaryCondition:
    """ImmersedBoundaryCondition(west =, east =, south =, north =) of FluxBoundaryConditions with number values: the
    stresses the ice feels on immersed faces (ice_stress_divergence.jl:65-123).  Passed as
    SeaIceModel(boundary_conditions = dict(u = FieldBoundaryConditions(immersed = ImmersedBoundaryCondition(...)), ...))."""

    def __init__(self, west=None, east=None, south=None, north=None):
        self.west, self.east, self.south, self.north = west, east, south, north

    def values(self):
        out = []
        for bc in (self.west, self.east, self.south, self.north):
            if bc is None:
                out.append(0.0)
            elif isinstance(bc, FluxBoundaryCondition):
                out.append(bc.value)
            else:
                raise NotImplementedError("immersed boundary conditions: FluxBoundaryCondition(number) or None")
        return out


class PrescribedTemperature:
    """HeatBoundaryConditions.PrescribedTemperature(T): a number, or per cell an (Ny, Nx) array / CenterField
    (slab_sea_ice_thermodynamics.jl:83-100)."""

    def __init__(self, temperature):
        refuse_series(temperature, "PrescribedTemperature (the per-cell temperature is also state)")
        self.per_cell = not _is_number(temperature)
        self.temperature = temperature if self.per_cell else float(temperature)


class RadiativeEmission:
    """HeatBoundaryConditions.RadiativeEmission (boundary_fluxes.jl:98-127): the top heat flux eps sigma (T + T_r)^4 at the
    surface temperature T.  A term of top_heat_flux, alone or in a tuple; with MeltingConstrainedFluxBalance the surface
    temperature is solved per cell by the secant method (include/csi.h, csi_heat_fluxes_set)."""

    def __init__(self, emissivity=1.0, stefan_boltzmann_constant=5.67e-8, reference_temperature=273.15):
        self.emissivity = float(emissivity)
        self.stefan_boltzmann_constant = float(stefan_boltzmann_constant)
        self.reference_temperature = float(reference_temperature)


_WEIGHTINGS = {None: _lib.WEIGHT_NONE, "concentration": _lib.WEIGHT_CONCENTRATION, "ice_present": _lib.WEIGHT_ICE_PRESENT}


class LinearHeatFlux:
    """The bulk form the reference's users write into a FluxFunction closure (examples/melting_in_spring.jl:64-73,
    test/test_energy_conservation.jl:8-13), as data: Q(T) = (K * (T - Ta)) * w at the surface temperature T, in this order.
    coefficient K (W m^-2 K^-1) and reference_temperature Ta: a number, an (Ny, Nx) array, a CenterField or a FieldTimeSeries.
    area_weighting: "concentration" (w = aice at the start of the step), "ice_present" (Q = 0 where aice == 0, no product) or None.
    A term of top_heat_flux, alone or in a tuple, at most one; with MeltingConstrainedFluxBalance the surface temperature is solved
    per cell by the secant method, as with RadiativeEmission (include/csi.h, csi_heat_fluxes_set)."""

    def __init__(self, coefficient, reference_temperature, area_weighting="concentration"):
        if area_weighting not in _WEIGHTINGS:
            raise ValueError('LinearHeatFlux.area_weighting: "concentration", "ice_present" or None')
        self.coefficient = float(coefficient) if _is_number(coefficient) else coefficient
        self.reference_temperature = float(reference_temperature) if _is_number(reference_temperature) else reference_temperature
        self.area_weighting = area_weighting

    @property
    def per_cell(self):
        return not (_is_number(self.coefficient) and _is_number(self.reference_temperature))


class SteppedAlbedo:
    """alpha(T) = cold if T < threshold else warm (strict <): the albedo of examples/arctic_basin_seasonal_cycle.jl:106-110,
    ifelse(Ts < -0.1, 0.75, 0.64), as data.  Both albedos lie in [0, 1]."""

    def __init__(self, cold=0.75, warm=0.64, threshold=-0.1):
        for name, v in (("cold", cold), ("warm", warm), ("threshold", threshold)):
            if not _is_number(v) or not np.isfinite(v):
                raise ValueError(f"SteppedAlbedo.{name}: a finite number is needed")
        for name, v in (("cold", cold), ("warm", warm)):
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"SteppedAlbedo.{name} = {v}: an albedo lies in [0, 1]")
        self.cold, self.warm, self.threshold = float(cold), float(warm), float(threshold)


class ShortwaveRadiation:
    """Absorbed shortwave radiation with a temperature-dependent albedo, the closure of examples/arctic_basin_seasonal_cycle.jl:106-110 as
    data: Q(T) = (F * (1 - alpha(T))) * w at the surface temperature T, in this order (include/csi.h, csi_shortwave_set).
    flux F (W m^-2, positive upward like every heat flux: sunlight reaching the surface is negative): a number, an (Ny, Nx) array, a
    CenterField or a FieldTimeSeries.  albedo: a SteppedAlbedo; snow_albedo: a second one for the cells of a model with a snow layer
    whose hs at the start of the step is > 0 (None: `albedo` serves both).  area_weighting: as LinearHeatFlux's, default None.
    A term of top_heat_flux, alone or in a tuple, at most one; with MeltingConstrainedFluxBalance the surface temperature is solved per
    cell by the secant method, and model.albedo_used holds the albedo every step used.  Give the balance its RadiativeEmission term as
    well, as the example does: beside terms that are linear in T alone the secant can cycle across the albedo's jump until maxiters
    (include/csi.h)."""

    def __init__(self, flux, albedo=None, snow_albedo=None, area_weighting=None):
        if area_weighting not in _WEIGHTINGS:
            raise ValueError('ShortwaveRadiation.area_weighting: "concentration", "ice_present" or None')
        albedo = SteppedAlbedo() if albedo is None else albedo
        for name, a in (("albedo", albedo), ("snow_albedo", snow_albedo)):
            if not isinstance(a, SteppedAlbedo) and not (name == "snow_albedo" and a is None):
                raise TypeError(f"ShortwaveRadiation.{name}: a SteppedAlbedo is needed, got {type(a).__name__} (a closure cannot cross "
                                "the C ABI; a continuous ramp is not offered: include/csi.h)")
        if callable(flux) or type(flux).__name__ == "FluxFunction" or isinstance(flux, (str, bool)) or flux is None:
            raise TypeError(f"ShortwaveRadiation.flux: a number, an (Ny, Nx) array, a CenterField or a FieldTimeSeries is needed, got "
                            f"{type(flux).__name__}")
        if _is_number(flux) and not np.isfinite(flux):
            raise ValueError("ShortwaveRadiation.flux is not finite")
        self.flux = float(flux) if _is_number(flux) else flux
        self.albedo, self.snow_albedo, self.area_weighting = albedo, snow_albedo, area_weighting

    @property
    def per_cell(self):
        return not _is_number(self.flux)

    def params(self):
        """The csi_shortwave this term describes."""
        a, s = self.albedo, self.snow_albedo
        return _lib.Shortwave(0.0 if self.per_cell else self.flux, a.cold, a.warm, a.threshold,
                              s.cold if s else 0.0, s.warm if s else 0.0, s.threshold if s else 0.0,
                              _WEIGHTINGS[self.area_weighting], int(self.per_cell), int(s is not None), 0)


def bulk_sensible_heat_flux(transfer_coefficient, atmosphere_density, atmosphere_heat_capacity, atmosphere_wind_speed,
                            atmosphere_temperature, area_weighting="concentration"):
    """The bulk sensible heat flux Cs rho_a c_a u_a (Tu - Ta) as a LinearHeatFlux: K = ((Cs * rho_a) * c_a) * u_a formed in this order
    in fp64 from numbers or arrays (examples/melting_in_spring.jl:64-73), Ta = atmosphere_temperature."""
    parts = [x if _is_number(x) else np.asarray(x, dtype=np.float64)
             for x in (transfer_coefficient, atmosphere_density, atmosphere_heat_capacity, atmosphere_wind_speed)]
    K = ((np.float64(parts[0]) * parts[1]) * parts[2]) * parts[3]
    return LinearHeatFlux(float(K) if np.ndim(K) == 0 else K, atmosphere_temperature, area_weighting)


class MeltingConstrainedFluxBalance:
    """HeatBoundaryConditions.MeltingConstrainedFluxBalance (top_heat_boundary_conditions.jl:5-52): the top temperature
    balances the external and conductive fluxes, capped at the melting temperature.  On the accelerated path the
    external flux does not depend on the temperature unless it has a RadiativeEmission or LinearHeatFlux term: then the reference's
    secant solve runs per cell, otherwise its closed-form root is used (include/csi.h)."""


class SlabThermodynamics:
    """SlabThermodynamics of the ice layer with a PrescribedTemperature (top_temperature = number) or
    MeltingConstrainedFluxBalance (top_heat_boundary_condition) top boundary condition and IceWaterThermalEquilibrium
    at the bottom (SeaIceThermodynamics/slab_sea_ice_thermodynamics.jl:82-109); PhaseTransitions defaults
    (SeaIceThermodynamics.jl:106-124).  Heat fluxes: a number, an (Ny, Nx) array, a CenterField, RadiativeEmission (top only) or
    a tuple of them (summed as the reference's getflux does), here or in SeaIceModel (not both); bottom_salinity: a number or, per
    cell, an (Ny, Nx) array, a CenterField or a FieldTimeSeries (the ocean's surface salinity: Tb = Tm(S(i, j))); top_heat_flux=None is the
    reference's default: for a prescribed temperature the external flux in equilibrium with the internal conductive flux,
    otherwise 0 (sea_ice_model.jl:243-256); bottom_heat_flux=None is 0 and "frazil" the -(1 - aice) W m^-2 flux of
    examples/freezing_bucket.jl:79-81.  top_surface_temperature: the CenterField the model binds when the step reads or writes
    the surface temperature per cell (None before)."""

    def __init__(self, top_temperature=-10.0, conductivity=2.0, top_heat_flux=None, bottom_heat_flux=None,
                 heat_capacity=2000.0, density=917.0, liquid_density=999.8, liquid_heat_capacity=4186.0,
                 reference_latent_heat=334e3, reference_temperature=0.0, liquidus_slope=0.054,
                 freshwater_melting_temperature=0.0, bottom_salinity=0.0, ice_consolidation_thickness=0.05,
                 top_heat_boundary_condition=None, ice_salinity=0.0):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.prescribed = None            # PrescribedTemperature given per cell
        if isinstance(top_heat_boundary_condition, PrescribedTemperature):
            if top_heat_boundary_condition.per_cell:
                self.prescribed = top_heat_boundary_condition.temperature
                self.top_temperature = 0.0
            else:
                self.top_temperature = top_heat_boundary_condition.temperature
        self.flux_balance = isinstance(top_heat_boundary_condition, MeltingConstrainedFluxBalance)
        self.top_surface_temperature = None

    def params(self, sea_ice_density, snow=False, top_heat_flux=_OWN, bottom_heat_flux=_OWN):
        """csi_slab_params.  top_heat_flux / bottom_heat_flux: the model's resolved fluxes (default: this object's); those that
        are not numbers travel as heat-flux terms (SeaIceModel) and leave 0 here."""
        top = self.top_heat_flux if top_heat_flux is _OWN else top_heat_flux
        bottom = self.bottom_heat_flux if bottom_heat_flux is _OWN else bottom_heat_flux
        frazil = isinstance(bottom, str) and bottom == "frazil"
        equilibrium = top is None and not self.flux_balance and not snow     # sea_ice_model.jl:245-256
        return _lib.SlabParams(self.conductivity, sea_ice_density, self.density, self.liquid_density, self.liquid_heat_capacity,
                               self.heat_capacity, self.reference_latent_heat, self.reference_temperature, self.liquidus_slope,
                               self.freshwater_melting_temperature,
                               float(self.bottom_salinity) if _is_number(self.bottom_salinity) else 0.0, self.ice_consolidation_thickness,
                               self.top_temperature, 1 if equilibrium else 0, 1 if frazil else 0,
                               float(top) if _is_number(top) else 0.0,
                               1.0 if frazil else (float(bottom) if _is_number(bottom) else 0.0),
                               1 if self.flux_balance else 0, 0, float(self.ice_salinity))


class SnowSlabThermodynamics:
    """snow_slab_thermodynamics(grid; conductivity = 0.31) (slab_sea_ice_thermodynamics.jl:42-49): the snow layer of
    the layered step.  Top boundary condition: MeltingConstrainedFluxBalance (the default) or PrescribedTemperature."""

    def __init__(self, conductivity=0.31, top_heat_boundary_condition=None):
        self.conductivity = float(conductivity)
        self.top_heat_boundary_condition = top_heat_boundary_condition or MeltingConstrainedFluxBalance()

        self.top_surface_temperature = None

    @property
    def prescribed(self):
        """The per-cell PrescribedTemperature of the snow surface (None: a number or the flux balance)."""
        bc = self.top_heat_boundary_condition
        return bc.temperature if isinstance(bc, PrescribedTemperature) and bc.per_cell else None

    def params(self, snow_density, snowfall):
        bc = self.top_heat_boundary_condition
        prescribed = isinstance(bc, PrescribedTemperature)
        return _lib.SnowParams(self.conductivity, float(snow_density), float(snowfall) if _is_number(snowfall) else 0.0,
                               bc.temperature if prescribed and not bc.per_cell else 0.0, 0 if prescribed else 1, 0)


def snow_slab_thermodynamics(grid=None, conductivity=0.31, **kw):
    return SnowSlabThermodynamics(conductivity=conductivity, **kw)


class WENO:
    """WENO(order = 3 | 5 | 7), upstream's upwind-biased WENO-Z scheme (called at sea_ice_advection.jl:51-58).
    weight_dtype: "f64" (default) or "f32" -- the precision of the smoothness indicators and nonlinear weights, mirroring the second
    float type parameter FT2 of newer upstream versions (include/csi.h: csi_set_weno_weight_dtype; recalled, unverified)."""

    def __init__(self, order=5, weight_dtype="f64"):
        if order not in (3, 5, 7):
            raise NotImplementedError("WENO order 3, 5 or 7")
        if weight_dtype not in ("f64", "f32"):
            raise ValueError("weight_dtype must be 'f64' or 'f32'")
        self.order = order
        self.scheme = order
        self.weight_dtype = weight_dtype


class UpwindBiased:
    def __init__(self, order=5):
        if order not in (1, 3, 5):
            raise NotImplementedError("UpwindBiased order 1, 3 or 5")
        self.order = order
        self.scheme = 1 if order == 1 else -order


_TOPO = {Periodic: _lib.PERIODIC, Bounded: _lib.BOUNDED, FullyConnected: _lib.FULLY_CONNECTED,
         LeftConnected: _lib.LEFT_CONNECTED, RightConnected: _lib.RIGHT_CONNECTED,
         RightFolded: _lib.RIGHT_FOLDED, LeftConnectedRightFolded: _lib.LEFT_CONNECTED_RIGHT_FOLDED}


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class SeaIceModel:
    def __init__(self, grid, dynamics=None, advection=None, timestepper="SplitRungeKutta3", sea_ice_density=900.0,
                 ice_thermodynamics=None, snow_thermodynamics=None, snow_density=330.0, snowfall=0.0,
                 boundary_conditions=None, forcing=None, device="cuda:0", mode="fast", stream=None, top_heat_flux=None,
                 bottom_heat_flux=None, ocean=None, tracers=None):
        self.grid = grid
        # tracers: names or csi.Tracer / csi.IceAge specs, advected on the device (tracers.py; include/csi.h); refused before anything is allocated
        from .tracers import tracer_specs
        self.tracer_specs = tracer_specs(tracers, grid)
        # dynamics: None (prescribed velocities), a SeaIceMomentumEquation, or StressBalanceFreeDrift(top_momentum_stress = ...,
        # bottom_momentum_stress = ...) as the whole dynamics (stress_balance_free_drift.jl:131-151)
        if isinstance(dynamics, StressBalanceFreeDrift):
            dynamics.check_as_dynamics()
        elif dynamics is not None and not isinstance(dynamics, SeaIceMomentumEquation):
            raise NotImplementedError("dynamics: None, a SeaIceMomentumEquation or a StressBalanceFreeDrift")
        self.dynamics = dynamics
        self.advection = advection
        self.ice_thermodynamics = ice_thermodynamics
        self.boundary_conditions = boundary_conditions or {}
        self.forcing = forcing          # dict(u = array-like, v = array-like): model.forcing given as arrays (m s^-2)
        self.snow_thermodynamics = snow_thermodynamics
        # snowfall: a number or per cell an (Ny, Nx) array / CenterField (thermodynamic_time_step.jl:328-334)
        self.snow_density, self.snowfall = float(snow_density), float(snowfall) if _is_number(snowfall) else snowfall
        # external_heat_fluxes (sea_ice_model.jl:262-264): given here or in SlabThermodynamics; _configure_heat resolves them
        self._heat_flux_args = (top_heat_flux, bottom_heat_flux)
        if ice_thermodynamics is not None:
            check_heat_fluxes(grid, ice_thermodynamics, top_heat_flux, bottom_heat_flux, snowfall if snow_thermodynamics else None,
                              snow=snow_thermodynamics)
        # ocean: None (the bottom heat flux is given) or a SlabOceanMixedLayer, which computes it (ocean.py; include/csi.h)
        check_ocean(grid, ocean, ice_thermodynamics, bottom_heat_flux, _cell_shape_ok)
        self.ocean = ocean
        self.external_heat_fluxes = SimpleNamespace(top=None, bottom=None)
        if snow_thermodynamics is not None and ice_thermodynamics is None:
            raise ValueError("a snow layer needs ice_thermodynamics")
        if timestepper not in ("SplitRungeKutta3", "ForwardEuler"):
            raise ValueError("timestepper must be 'SplitRungeKutta3' or 'ForwardEuler'")
        self.timestepper_kind = timestepper
        self.sea_ice_density = float(sea_ice_density)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SeaIceModel needs a HIP device (torch 'cuda' device); there is no CPU path")
        dev = self.device
        # prognostic fields (sea_ice_model.jl:182-183,199-200)
        self.velocities = SimpleNamespace(u=XFaceField(grid, dev, "u"), v=YFaceField(grid, dev, "v"))
        self.ice_thickness = CenterField(grid, dev, "h")
        self.ice_concentration = CenterField(grid, dev, "aice")
        # TimeStepper(timestepper, grid, prognostic_fields): G^n for both, Psi^- for RK (:235)
        Gn = SimpleNamespace(h=CenterField(grid, dev, "Gh"), aice=CenterField(grid, dev, "Gaice"))
        self.timestepper = SimpleNamespace(Gn=Gn, Psi_minus=None)
        if isinstance(dynamics, SeaIceMomentumEquation) and isinstance(dynamics.solver, ExplicitSolver):
            # the ExplicitSolver's velocity tendencies (explicit_momentum_equations.jl:103-104)
            Gn.u, Gn.v = XFaceField(grid, dev, "Gu"), YFaceField(grid, dev, "Gv")
        if timestepper == "SplitRungeKutta3":
            self.timestepper.Psi_minus = SimpleNamespace(h=CenterField(grid, dev, "h-"), aice=CenterField(grid, dev, "aice-"),
                                                         u=XFaceField(grid, dev, "u-"), v=YFaceField(grid, dev, "v-"))
        # snow layer: hs is a prognostic field with its own tendency and cache (sea_ice_model.jl:201-224)
        self.snow_thickness = None
        self.mass_fluxes = None
        if snow_thermodynamics is not None:
            self.snow_thickness = CenterField(grid, dev, "hs")
            Gn.hs = CenterField(grid, dev, "Ghs")
            if self.timestepper.Psi_minus is not None:
                self.timestepper.Psi_minus.hs = CenterField(grid, dev, "hs-")
            self.mass_fluxes = SimpleNamespace(thermodynamics=SimpleNamespace(ice=CenterField(grid, dev, "mass_flux"),
                                                                              snow=CenterField(grid, dev, "mass_flux_snow")),
                                               intercepted_snowfall=CenterField(grid, dev, "intercepted_snowfall"))
            self.snow_top_temperature = CenterField(grid, dev, "Tu_snow")
            self.ice_top_temperature = CenterField(grid, dev, "Tu")
        # advected tracers: name -> CenterField, in the order given (model.tracer(name)); their tendencies in Gn.<name> and csi_tracers_set
        # in _configure.  Empty: none of the tracer calls is ever made
        self.tracers = OrderedDict((t.name, CenterField(grid, dev, t.name)) for t in self.tracer_specs)
        for t in self.tracer_specs:
            setattr(Gn, t.name, CenterField(grid, dev, "G" + t.name))
        self.clock = SimpleNamespace(time=0.0, iteration=0)
        self.output_writers = OrderedDict()      # key -> output.OutputWriter, driven by time_step (empty: nothing is called)
        self.drifters = None                     # a drifters.Drifters: time_step advances them with the step's dt (None: no call)
        self._keep = []
        self._stress_fields = {}
        self._free_drift_fields = {}
        self._derived_fields = {}           # name -> CenterField of the derived fields asked for so far (derived_field)
        self._momentum_term_fields = {}     # name -> XFaceField / YFaceField of the momentum term fields asked for so far (momentum_term)
        self._series, self._pending_series = {}, []     # slot name -> what csi_time_series_set was given (kept alive)
        self._regrid_maps, self._series_arrays = {}, {}   # (id(source), location) -> (map id, source); id(source data) -> its device copy
        self.linear_heat_flux = None        # the LinearHeatFlux term's per-cell (coefficient, reference_temperature) fields, if any
        self.bottom_salinity = None         # the per-cell bottom salinity's field, if any
        self.shortwave = None               # the ShortwaveRadiation term, if any, and its per-cell flux's field
        self.shortwave_flux = None
        self._albedo_used = None
        self._heat_fluxes_used = None
        self._lazy_fields = {}              # slot -> the output field allocated and bound the first time it was asked for (_lazy_slot_field)
        self.ctx = _lib.Context(dev.index or 0, stream)
        self._configure()
        self._attach_pending_series()
        if self.tracer_specs:
            from .tracers import attach
            attach(self)
        self.set_mode(mode)
        self.ctx.call("csi_set_weno_weight_dtype", 1 if getattr(advection, "weight_dtype", "f64") == "f32" else 0)
        torch.cuda.synchronize(self.device)   # field initialisation ran on torch's stream

    # ---- plumbing: describe the problem to the library -----------------------------------------
    def _bind(self, name, fld):
        self.ctx.call("csi_field_bind", _lib.slot_id(name), C.c_void_p(fld.data.data_ptr()), fld.ni, fld.ni, fld.nj)

    def _slot_field(self, slot, value=None, name=None, bind=True):
        """The device field of a slot, at the slot's location (_lib.SLOTS), bound to it: a Field is used in place (moved to the device if
        needed), a FieldTimeSeries gets a new field it writes into, a number, array or function a new field set to it, None a zero field."""
        if isinstance(value, Field):
            fld = value
            if fld.data.device != self.device:
                fld.data = fld.data.to(self.device)
        else:
            fld = Field(_lib.slot_location(slot), self.grid, self.device, slot.lower() if name is None else name)
            if isinstance(value, FieldTimeSeries):
                self._pending_series.append((slot, value, fld))
            elif value is not None:
                fld.set(value)
        if bind:
            self._bind(slot, fld)
        return fld

    def _lazy_slot_field(self, slot, name):
        """An output field the library fills once its slot is bound: allocated, bound and kept the first time it is asked for."""
        if slot not in self._lazy_fields:
            fld = Field(_lib.slot_location(slot), self.grid, self.device, name)
            torch.cuda.synchronize(self.device)      # (the zero fill ran on torch's stream)
            self._bind(slot, fld)
            self._lazy_fields[slot] = fld
        return self._lazy_fields[slot]

    def _configure(self):
        g = self.grid
        m = g.metrics()
        met = _lib.Metrics()
        if m["kind"] == "uniform":
            kind = _lib.METRIC_UNIFORM
            met.dx, met.dy = m["dx"], m["dy"]
        elif m["kind"] == "full":
            kind = _lib.METRIC_FULL
            met.full_ld = g.Nx + 2 * g.Hx + 1
            for k, name in enumerate(METRIC_NAMES):
                a = np.ascontiguousarray(m[name], dtype=np.float64)
                assert a.shape == (g.Ny + 2 * g.Hy + 1, g.Nx + 2 * g.Hx + 1), (name, a.shape)
                self._keep.append(a)
                met.full[k] = _dptr(a)
        else:
            kind = _lib.METRIC_PER_J
            met.dy = m["dy"]
            for k in ("dxc", "dxf", "azc", "azf"):
                a = np.ascontiguousarray(m[k], dtype=np.float64)
                self._keep.append(a)
                setattr(met, k, _dptr(a))
        self.ctx.call("csi_grid_set", g.Nx, g.Ny, g.Hx, g.Hy, _TOPO[g.topology[0]], _TOPO[g.topology[1]], kind, C.byref(met))
        if isinstance(g, TileGrid):
            self._init_tiles(g)
        self._bind("H", self.ice_thickness)
        self._bind("A", self.ice_concentration)
        self._bind("U", self.velocities.u)
        self._bind("V", self.velocities.v)
        self._bind("GH", self.timestepper.Gn.h)
        self._bind("GA", self.timestepper.Gn.aice)
        if hasattr(self.timestepper.Gn, "u"):
            self._bind("GU", self.timestepper.Gn.u)
            self._bind("GV", self.timestepper.Gn.v)
        if self.timestepper.Psi_minus is not None:
            pm = self.timestepper.Psi_minus
            self._bind("HM", pm.h); self._bind("AM", pm.aice); self._bind("UM", pm.u); self._bind("VM", pm.v)
        if self.snow_thermodynamics is not None:
            self._bind("HS", self.snow_thickness)
            self._bind("GHS", self.timestepper.Gn.hs)
            if self.timestepper.Psi_minus is not None:
                self._bind("HSM", self.timestepper.Psi_minus.hs)
            self._bind("MASS_FLUX", self.mass_fluxes.thermodynamics.ice)
            self._bind("MASS_FLUX_SNOW", self.mass_fluxes.thermodynamics.snow)
            self._bind("SNOWFALL_INTERCEPTED", self.mass_fluxes.intercepted_snowfall)
            self._bind("TU", self.ice_top_temperature)
            self._bind("TUS", self.snow_top_temperature)
            wp = self.snow_thermodynamics.params(self.snow_density, self.snowfall)
            self.ctx.call("csi_snow_params_set", C.byref(wp))
            self._snow_params = wp
        if self.ice_thermodynamics is not None:
            self._configure_heat()
        # boundary_conditions = (u = FieldBoundaryConditions(north = ValueBoundaryCondition(0), ...), v = ...)
        for name, sides in (("U", ("south", "north")), ("V", ("west", "east"))):
            bcs = self.boundary_conditions.get(name.lower())
            for k, side in enumerate(sides):
                bc = getattr(bcs, side, None) if bcs is not None else None
                if bc is not None and not isinstance(bc, ValueBoundaryCondition):
                    raise NotImplementedError("velocity boundary conditions: ValueBoundaryCondition or the default")
                if bc is not None and not isinstance(bc.value, float):
                    raise NotImplementedError("velocity boundary conditions: ValueBoundaryCondition(number); an array or a FieldTimeSeries "
                                              "is accepted by the enthalpy-method column model's temperature only")
                self.ctx.call("csi_velocity_bc_set", _lib.F[name], k, 0 if bc is None else 1, 0.0 if bc is None else bc.value)
            imm = getattr(bcs, "immersed", None) if bcs is not None else None
            self.ctx.call("csi_immersed_flux_bc_set", _lib.F[name], *(imm.values() if imm is not None else (0.0, 0.0, 0.0, 0.0)))
        # model.forcing = (u = array, v = array): user forcing of the velocity tendencies (sum_of_forcing_u / _v)
        if self.forcing is not None:
            self.forcing_fields = SimpleNamespace(u=self._slot_field("FORCING_U", self.forcing["u"]), v=self._slot_field("FORCING_V", self.forcing["v"]))
            torch.cuda.synchronize(self.device)
            self.ctx.call("csi_fill_halo_local", _lib.F["FORCING_U"])
            self.ctx.call("csi_fill_halo_local", _lib.F["FORCING_V"])
        d = self.dynamics
        if d is None:
            return
        if isinstance(d, StressBalanceFreeDrift):
            # the free-drift velocity as the whole dynamics: the two stresses and the dynamics kind; nothing of a momentum equation
            self._set_stress(_lib.STRESS_TOP, d.top_momentum_stress, "TOP")
            self._set_stress(_lib.STRESS_BOTTOM, d.bottom_momentum_stress, "BOT")
            self.ctx.call("csi_dynamics_set", _lib.DYNAMICS_FREE_DRIFT)
            return
        if d.grid is not g:
            raise ValueError("dynamics was built on a different grid")
        f = d.auxiliaries.fields
        for fld in vars(f).values():
            if fld.data.device != self.device:
                fld.data = fld.data.to(self.device)
        viscous = isinstance(d.rheology, ViscousRheology)
        if not viscous:                            # ViscousRheology: no auxiliary fields (Rheologies.jl:33)
            for name, fld in (("S11", f.s11), ("S22", f.s22), ("S12", f.s12), ("UN", f.un), ("VN", f.vn), ("P", f.P),
                              ("ALPHA", f.alpha), ("DELTA", f.Delta), ("ZETA_F", f.zeta_f), ("ZETA_C", f.zeta_c)):
                self._bind(name, fld)
        # (the scalars every rheology shares travel in csi_evp_params; a viscous model leaves the EVP ones at their defaults)
        r = ElastoViscoPlasticRheology() if viscous else d.rheology
        p = _lib.EvpParams(r.ice_compressive_strength, r.ice_compaction_hardening, r.yield_curve_eccentricity,
                           r.minimum_plastic_stress, r.min_relaxation_parameter, r.max_relaxation_parameter,
                           r.relaxation_strength,
                           _lib.PRESSURE_ICE_STRENGTH if isinstance(r.pressure_formulation, IceStrength) else _lib.PRESSURE_REPLACEMENT,
                           0 if d.coriolis is None else 1, float(getattr(d.coriolis, "f", 0.0)),
                           d.minimum_concentration, d.minimum_mass, self.sea_ice_density)
        self.ctx.call("csi_evp_params_set", C.byref(p))
        self.ctx.call("csi_rheology_set", _lib.RHEOLOGY_VISCOUS if viscous else _lib.RHEOLOGY_EVP, d.rheology.nu if viscous else 0.0)
        self.ctx.call("csi_momentum_solver_set", _lib.SOLVER_EXPLICIT if isinstance(d.solver, ExplicitSolver) else _lib.SOLVER_SPLIT_EXPLICIT)
        if hasattr(d.coriolis, "points"):          # per-point f (curvilinear grids)
            fu, fv = d.coriolis.points(g)
            self._keep += [fu, fv]
            self.ctx.call("csi_coriolis_rows_set", None, None, 0)
            self.ctx.call("csi_coriolis_points_set", _dptr(fu), _dptr(fv), fu.shape[1])
        elif hasattr(d.coriolis, "rows"):          # BetaPlane: f per row, evaluated here like the metric vectors
            fu, fv = (np.ascontiguousarray(a, dtype=np.float64) for a in d.coriolis.rows(g))
            self.ctx.call("csi_coriolis_rows_set", _dptr(fu), _dptr(fv), fu.size)
        else:
            self.ctx.call("csi_coriolis_rows_set", None, None, 0)
        self._set_stress(_lib.STRESS_TOP, d.external_momentum_stresses.top, "TOP")
        self._set_stress(_lib.STRESS_BOTTOM, d.external_momentum_stresses.bottom, "BOT")
        if isinstance(d.free_drift, FreeDriftVelocities):      # free_drift = (u, v): the kernels read the two fields in place
            for comp, value in (("U", d.free_drift.u), ("V", d.free_drift.v)):
                self._free_drift_field(comp, value)
            self.ctx.call("csi_free_drift_set", _lib.FREE_DRIFT_FIELDS)
            torch.cuda.synchronize(self.device)
            for comp in ("U", "V"):                    # (csi_time_step_momentum fills them again at every step)
                self.ctx.call("csi_fill_halo_local", _lib.F[f"FREE_DRIFT_{comp}"])
        else:
            self.ctx.call("csi_free_drift_set", _lib.FREE_DRIFT_STRESS_BALANCE if d.free_drift is not None else _lib.FREE_DRIFT_NONE)

    def _cell_field(self, value, name):
        """A (Center, Center) field on the model grid from a CenterField (used as it is: writes into it reach the next step) or an
        (Ny, Nx) array -- on a TileGrid also one of the global grid's shape, of which the tile's part is taken."""
        g = self.grid
        if isinstance(value, Field) and (value.location != (Center, Center) or (value.ni, value.nj) != tuple(g.field_size(Center, Center))):
            raise ValueError(f"{name}: a CenterField on the model's grid is needed")
        slot = series_slot_of(name) if isinstance(value, FieldTimeSeries) else _lib.slot_of_display_name(name)
        if isinstance(value, (Field, FieldTimeSeries)):      # (a series writes into a new field; every field is bound by the caller)
            return self._slot_field(slot, value, name, bind=False)
        arr = np.asarray(value, dtype=np.float64)
        if arr.ndim == 0:                           # a number beside a per-cell partner (LinearHeatFlux): broadcast
            arr = np.full((g.Ny, g.Nx), float(arr))
        if isinstance(g, TileGrid) and arr.shape == (g.global_grid.Ny, g.global_grid.Nx):
            arr = arr[g.j_off:g.j_off + g.Ny, g.i_off:g.i_off + g.Nx]
        if arr.shape != (g.Ny, g.Nx):
            raise ValueError(f"{name}: an array of shape (Ny, Nx) = {(g.Ny, g.Nx)} is needed, got {arr.shape}")
        return self._slot_field(slot, arr, name, bind=False)

    def _heat_terms(self, spec, side):
        """getflux's forms (boundary_fluxes.jl:8-22, 98-127) as csi_heat_flux_term entries: None for the numeric path (None, a
        number, "frazil"), else (terms, the ARRAY term's field or None).  check_heat_flux has vetted spec."""
        if spec is None or _is_number(spec) or isinstance(spec, str):
            return None
        items = spec if isinstance(spec, tuple) else (spec,)
        terms, field = [], None
        for x in items or (0.0,):            # getflux(()) = zero(grid)
            t = _lib.HeatFluxTerm()
            if _is_number(x):
                t.kind, t.value = _lib.FLUX_CONSTANT, float(x)
            elif isinstance(x, RadiativeEmission):
                t.kind = _lib.FLUX_RADIATIVE_EMISSION
                t.emissivity, t.stefan_boltzmann_constant, t.reference_temperature = (x.emissivity, x.stefan_boltzmann_constant,
                                                                                       x.reference_temperature)
            elif isinstance(x, LinearHeatFlux):
                t.kind, t.reserved = _lib.FLUX_LINEAR, _WEIGHTINGS[x.area_weighting]
                if x.per_cell:          # both per cell: a number beside an array is broadcast into one
                    t.reserved |= _lib.LINEAR_COEFFICIENT_ARRAY | _lib.LINEAR_REFERENCE_ARRAY
                    k = self._cell_field(x.coefficient, "flux_coefficient")
                    ta = self._cell_field(x.reference_temperature, "flux_reference_temperature")
                    self._bind("FLUX_COEFFICIENT", k)
                    self._bind("FLUX_REFERENCE_TEMPERATURE", ta)
                    self.linear_heat_flux = SimpleNamespace(coefficient=k, reference_temperature=ta)
                else:
                    t.value, t.reference_temperature = x.coefficient, x.reference_temperature
            elif isinstance(x, ShortwaveRadiation):
                t.kind = _lib.FLUX_SHORTWAVE          # (marks the position in the sum; csi_shortwave_set carries the rest, first)
                if x.per_cell:
                    self.shortwave_flux = self._cell_field(x.flux, "shortwave")
                    self._bind("SHORTWAVE", self.shortwave_flux)
                self.shortwave = x
                self._shortwave_params = x.params()
                self.ctx.call("csi_shortwave_set", C.byref(self._shortwave_params))
            else:
                field = self._cell_field(x, f"{side}_heat_flux")
                t.kind = _lib.FLUX_ARRAY
            terms.append(t)
        return terms, field

    def _configure_heat(self):
        """External heat fluxes, per-cell prescribed temperature and snowfall (include/csi.h, csi_heat_fluxes_set)."""
        ice, snow = self.ice_thermodynamics, self.snow_thermodynamics
        top_arg, bottom_arg = self._heat_flux_args
        top = top_arg if top_arg is not None else ice.top_heat_flux
        bottom = bottom_arg if bottom_arg is not None else ice.bottom_heat_flux
        if self.ocean is not None:       # the mixed layer writes the one ARRAY bottom term's array before every thermodynamic step
            bottom = np.zeros((self.grid.Ny, self.grid.Nx))
        sp = ice.params(self.sea_ice_density, snow=snow is not None, top_heat_flux=top, bottom_heat_flux=bottom)
        self.ctx.call("csi_slab_params_set", C.byref(sp))
        self._slab_params = sp
        fields = {}
        for side, spec, slot, k in (("top", top, "TOP_HEAT_FLUX", _lib.HEAT_TOP), ("bottom", bottom, "BOTTOM_HEAT_FLUX", _lib.HEAT_BOTTOM)):
            got = self._heat_terms(spec, side)
            if got is None:
                self.ctx.call("csi_heat_fluxes_set", k, None, 0)
                setattr(self.external_heat_fluxes, side, spec)
                continue
            terms, fld = got
            arr = (_lib.HeatFluxTerm * len(terms))(*terms)
            self._keep.append(arr)
            if fld is not None:
                self._bind(slot, fld)
            self.ctx.call("csi_heat_fluxes_set", k, arr, len(terms))
            setattr(self.external_heat_fluxes, side, fld if fld is not None else spec)
            fields[side] = got
        prescribed = snow.prescribed if snow is not None else ice.prescribed
        snowfall_array = snow is not None and not _is_number(self.snowfall)
        if snowfall_array:
            self.snowfall = self._cell_field(self.snowfall, "snowfall")
            self._bind("SNOWFALL", self.snowfall)
        # IceWaterThermalEquilibrium.salinity per cell (bottom_heat_boundary_conditions.jl:36-39)
        salinity_array = not _is_number(ice.bottom_salinity)
        if salinity_array:
            self.bottom_salinity = self._cell_field(ice.bottom_salinity, "bottom_salinity")
            self._bind("BOTTOM_SALINITY", self.bottom_salinity)
        ss = _lib.SurfaceSolve(1e-3, 1000, int(prescribed is not None), int(snowfall_array),
                               _lib.SOLVE_BOTTOM_SALINITY_ARRAY if salinity_array else 0)
        self.ctx.call("csi_surface_solve_set", C.byref(ss))
        # top_surface_temperature (top_heat_boundary_conditions.jl:82-100): state that starts at 0 wherever the step reads or writes it
        if snow is not None:
            if prescribed is not None:
                if isinstance(prescribed, Field):
                    self.snow_top_temperature = self._cell_field(prescribed, "Tu_snow")
                    self._bind("TUS", self.snow_top_temperature)
                else:
                    self.snow_top_temperature.set(self._cell_field(prescribed, "Tu_snow").interior_numpy())
            ice.top_surface_temperature, snow.top_surface_temperature = self.ice_top_temperature, self.snow_top_temperature
        elif prescribed is not None or (ice.flux_balance and fields):
            tu = self._cell_field(prescribed, "Tu") if prescribed is not None else CenterField(self.grid, self.device, "Tu")
            self.ice_top_temperature = ice.top_surface_temperature = tu
            self._bind("TU", tu)
        if self.ocean is not None:
            self.ocean.attach(self)

    def _init_tiles(self, g):
        """csi_tile_set + RCCL communicator: rank 0 makes the unique id, the host broadcasts it
        (torch.distributed when there is more than one process; plumbing only)."""
        self.ctx.call("csi_tile_set", g.rx, g.ry, g.Rx, g.Ry, int(g.periodic[0]), int(g.periodic[1]))
        world = g.Rx * g.Ry
        if getattr(g, "local_group", None) is not None:      # several tiles in this process (one thread each): no RCCL
            if g.local_group.world_size != world:
                raise RuntimeError("the local group's size does not match the partition")
            self._keep.append(g.local_group)
            self.ctx.call("csi_comm_init_local", g.local_group.h, g.rank)
            return
        if getattr(g, "host_group", None) is not None:       # one process per tile, no RCCL: shared memory + HIP IPC
            self.ctx.call("csi_comm_init_host", str(g.host_group).encode(), world, g.rank)
            return
        idbuf = (C.c_uint8 * 128)()
        if world > 1:
            import torch.distributed as dist
            if not dist.is_initialized():
                raise RuntimeError("a tiled model with more than one tile needs torch.distributed to be initialised")
            if dist.get_world_size() != world or dist.get_rank() != g.rank:
                raise RuntimeError("tile rank / partition do not match torch.distributed")
            payload = [None]
            if g.rank == 0:
                rc = self.ctx.L.csi_comm_unique_id(idbuf)
                if rc != _lib.OK:
                    raise _lib.CsiError(rc, self.ctx.L.csi_last_error(None).decode())
                payload = [bytes(idbuf)]
            dist.broadcast_object_list(payload, src=0)
            idbuf = (C.c_uint8 * 128).from_buffer_copy(payload[0])
        else:
            rc = self.ctx.L.csi_comm_unique_id(idbuf)
            if rc != _lib.OK:
                raise _lib.CsiError(rc, self.ctx.L.csi_last_error(None).decode())
        self.ctx.call("csi_comm_init", world, g.rank, idbuf)

    def _stress_field(self, slot, comp, value):
        """materialize_stress (sea_ice_external_stress.jl:63-69,132-137): a device copy on the model grid."""
        fld = self._stress_fields[f"{slot}_{comp}"] = self._slot_field(f"{slot}_{comp}", value)
        return fld

    def _set_stress(self, side, stress, slot):
        s = _lib.Stress()
        if stress is None:
            s.kind = _lib.STRESS_NONE
        elif isinstance(stress, SemiImplicitStress):
            s.kind = _lib.STRESS_SEMI_IMPLICIT
            s.rho_e, s.Cd = stress.rho_e, stress.Cd
            for comp, val in (("u", stress.ue), ("v", stress.ve)):
                if val is None:
                    setattr(s, comp + "e_kind", _lib.VEL_ZERO)
                elif np.isscalar(val):
                    setattr(s, comp + "e_kind", _lib.VEL_CONST)
                    setattr(s, comp + "e", float(val))
                else:
                    setattr(s, comp + "e_kind", _lib.VEL_FIELD)
                    self._stress_field(slot, comp.upper(), val)
        else:
            tu, tv = (stress["u"], stress["v"]) if isinstance(stress, dict) else (stress[0], stress[1])
            if np.isscalar(tu) and np.isscalar(tv):
                s.kind = _lib.STRESS_CONST
                s.tau_u, s.tau_v = float(tu), float(tv)
            else:
                s.kind = _lib.STRESS_FIELD
                self._stress_field(slot, "U", tu)
                self._stress_field(slot, "V", tv)
        self.ctx.call("csi_stress_set", side, C.byref(s))

    @property
    def heat_fluxes_used(self):
        """(top, bottom): the CenterFields into which every thermodynamic step writes the external heat fluxes it used (W m^-2) --
        the bare-ice step its Qu (the internal flux with the equilibrium default) and Qb, the layered step Qui per cell, before the
        snow-melt partition, and Qbi.  Allocated and bound the first time they are asked for; from then on the flux kernels run also
        for a numeric configuration, with the number path's bits.  Read them after the step (synchronize() first)."""
        if self.ice_thermodynamics is None:
            raise ValueError("heat_fluxes_used needs ice_thermodynamics")
        if self._heat_fluxes_used is None:
            self._heat_fluxes_used = SimpleNamespace(top=self._lazy_slot_field("TOP_HEAT_FLUX_USED", "top_heat_flux_used"),
                                                     bottom=self._lazy_slot_field("BOTTOM_HEAT_FLUX_USED", "bottom_heat_flux_used"))
        return self._heat_fluxes_used

    @property
    def albedo_used(self):
        """The CenterField into which every thermodynamic step writes the albedo its ShortwaveRadiation term used, at the surface
        temperature the step solved or was given.  Allocated and bound the first time it is asked for.  Read it after the step
        (synchronize() first); in an RK3 step it holds the last stage's values."""
        if self.shortwave is None:
            raise ValueError("albedo_used needs a ShortwaveRadiation term in top_heat_flux")
        self._albedo_used = self._lazy_slot_field("ALBEDO_USED", "albedo_used")
        return self._albedo_used

    def external_stress_field(self, slot, comp):
        return self._stress_fields[f"{slot}_{comp}"]

    def _free_drift_field(self, comp, value):
        """One component of `free_drift = (u, v)` on the device, like _stress_field: a field of the grid is used as it is, a number or
        an interior-shaped array fills a new one.  The library fills the halos at every momentum step."""
        fld = self._free_drift_fields[comp] = self._slot_field(f"FREE_DRIFT_{comp}", value)
        return fld

    def free_drift_field(self, comp):
        """The device field of a prescribed free-drift velocity component ("u" / "v"): write into its interior between steps (then
        torch.cuda.synchronize) to update it in place."""
        return self._free_drift_fields[comp.upper()]

    # ---- forcing time series (include/csi.h, csi_time_series_set) -----------------------------------------------------------------
    def _set_series(self, slot):
        s = self._series[slot]
        if s.map is None:
            self.ctx.call("csi_time_series_set", _lib.slot_id(slot), C.byref(s.struct))
        else:
            self.ctx.call("csi_time_series_set_regridded", _lib.slot_id(slot), C.byref(s.struct), s.map,
                          C.byref(s.other) if s.other is not None else None, s.series.component or 0)

    def _regrid_map(self, source, location):
        """The library's map from `source` to the points of `location` on this model's grid or tile: one per (source, location),
        shared by the slots; computed with csi_regrid_plan_axis (SourceGrid.plan) from grid.target_nodes, with grid.rotation."""
        key = (id(source), location)
        if key not in self._regrid_maps:
            i0, i1, j0, j1, wx, wy = source.plan(*self.grid.target_nodes(*location))
            cos, sin = self.grid.rotation(*location)
            kind = {(Face, Center): _lib.REGRID_FACE_CENTER, (Center, Face): _lib.REGRID_CENTER_FACE,
                    (Center, Center): _lib.REGRID_CENTER_CENTER}[location]
            self._regrid_maps[key] = (self.ctx.regrid_map_create(kind, i0, i1, j0, j1, wx, wy, source.shape, cos, sin), source)
        return self._regrid_maps[key][0]

    def _attach_pending_series(self):
        """Register the series met while the model was described (their fields are bound by now), interpolate them at the clock and
        fill the halos the library fills for plain arrays at construction."""
        for slot, fts, fld in self._pending_series:
            if isinstance(fts, RegriddedTimeSeries) and fts.component is not None and fts.location != fld.location:
                raise ValueError(f"{slot.lower()}: the {'xy'[fts.component]} component of a RegriddedVectorTimeSeries (.{'xy'[fts.component]}) "
                                 f"drives an array at ({fts.location[0].__name__}, {fts.location[1].__name__}); this one lies at "
                                 f"({fld.LX.__name__}, {fld.LY.__name__}) and takes .{'yx'[fts.component]}")
            if fts.location != fld.location or fts.interior_shape != tuple(reversed(self.grid.interior_size(*fld.location))):
                raise ValueError(f"{slot.lower()}: a FieldTimeSeries at ({fld.LX.__name__}, {fld.LY.__name__}) with slices of the "
                                 f"interior shape {tuple(reversed(self.grid.interior_size(*fld.location)))} is needed, got one at "
                                 f"({fts.location[0].__name__}, {fts.location[1].__name__}) with {fts.interior_shape}")
            if slot in self._series:
                raise ValueError(f"{slot.lower()}: two time series for one array")
            nt = len(fts)
            host = fts.backend.chunk_size is not None
            regridded = isinstance(fts, RegriddedTimeSeries)
            keep, structs = [], []
            for data in (fts.parts if regridded else (fts.data,)):      # (slices of the source shape for a regridded series)
                ny, nx = data.shape[1:]
                held = data if host else (self._series_arrays.get(id(data)) if regridded else None)
                if held is None:                                        # (the two members of a pair share their two device arrays)
                    held = self._series_arrays[id(data)] = torch.from_numpy(data).to(self.device)
                ptr = held.ctypes.data if host else held.data_ptr()    # (the caller's array: the library reads it)
                keep.append((held, data))
                structs.append(_lib.TimeSeries(nt, fts.time_indexing.kind, _lib.SERIES_HOST if host else _lib.SERIES_DEVICE,
                                               fts.backend.chunk_size or 0, fts.time_indexing.period, _dptr(fts.times), C.c_void_p(ptr), nx, nx * ny))
            self._series[slot] = SimpleNamespace(series=fts, field=fld, struct=structs[0], other=structs[1] if len(structs) > 1 else None, keep=keep,
                                                 map=self._regrid_map(fts.source, fld.location) if regridded else None,
                                                 window=fts.backend.chunk_size or 0)
        self._pending_series = []
        if not self._series:
            return
        torch.cuda.synchronize(self.device)
        for slot in self._series:
            self._set_series(slot)
        self.update_time_series()
        for slot in self._series:
            if self._series[slot].field.location != (Center, Center):
                self.ctx.call("csi_fill_halo_local", _lib.F[slot])

    def update_time_series(self):
        """csi_time_series_update at the model clock (time_step, time_step_momentum, compute_momentum_tendencies and update_state call
        it first); nothing is called for a model without series."""
        if self._series:
            self.ctx.time_series_update(self.clock.time)

    def time_series_status(self, slot):
        """(slices resident in the device window of a host-resident series, -1: none; slice uploads so far) of the series on `slot`,
        e.g. "TOP_U", "SNOWFALL"."""
        return self.ctx.time_series_status(slot, self._series[slot].window)

    def set_mode(self, mode):
        self.mode = mode
        self.ctx.call("csi_set_mode", _lib.MODE_FAST if mode == "fast" else _lib.MODE_STRICT)

    def set_fusion(self, level):
        """FAST mode: 0 / False = three-kernel path, 1 = one fused launch per sub-step, 2 / True (default) = two
        sub-steps per launch where the configuration allows it, 3 = three per launch on fully periodic grids with halo >= 6
        (two elsewhere); bit-identical results."""
        level = 2 if level is True else int(level)
        self.ctx.call("csi_set_fusion", level)

    def set_tile_skipping(self, on):
        """Untiled grids on the two-sub-steps kernel: skip the tiles with no ice mass in or around them (exact: include/csi.h,
        csi_set_tile_skipping; default on)."""
        self.ctx.call("csi_set_tile_skipping", 1 if on else 0)

    def tile_activity(self):
        """(tiles, live, used): the newest counts that have arrived from the device (synchronize() first for the last sub-cycle's)."""
        import ctypes as C
        t, l, u = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self.ctx.call("csi_tile_activity", C.byref(t), C.byref(l), C.byref(u))
        return t.value, l.value, u.value

    def set_row_constant(self, on=True, rtol=0.0):
        """CSI_METRIC_FULL grids: rows whose twelve metric planes hold one value per row are read from per-row vectors (bitwise-equal
        columns only unless rtol > 0: include/csi.h, csi_set_row_constant)."""
        self.ctx.call("csi_set_row_constant", 1 if on else 0, float(rtol))

    def row_constant_rows(self):
        import ctypes as C
        n = C.c_int32(0)
        self.ctx.call("csi_row_constant_rows", C.byref(n))
        return n.value

    def set_exchange_interval(self, k):
        """Tiles: exchange u, v halos of width 2k every k sub-steps (0 = automatic from the halo size)."""
        self.ctx.call("csi_set_exchange_interval", int(k))

    def set_halo_transport(self, kind):
        """Tiles: "peer" (default) = peer-direct halo writes over xGMI with flags, one RCCL exchange per sub-cycle; "rccl" = the
        k-batched ncclSend / ncclRecv exchange (include/csi.h, csi_set_halo_transport)."""
        self.ctx.call("csi_set_halo_transport", {"rccl": 0, "peer": 1}[kind])

    def set_peer_tier(self, tier):
        """Tiles on the peer transport: the memory-ordering tier of its flag protocol, the SAME on every rank (-1 automatic, the
        default: 1 across processes / devices, 0 for a tile connected to itself; 0 no fence, 1 + acquire fence behind the flags,
        2 + release fence before them; include/csi.h, csi_set_peer_tier)."""
        self.ctx.call("csi_set_peer_tier", int(tier))

    def set_mask(self, active):
        """ImmersedBoundaryGrid stand-in: `active` is a (Ny, Nx) boolean array of wet cells of the WHOLE domain (for a
        tile: of the global grid; the tile's mask, halo included, is sliced from it -- the mask is static, so no
        exchange is needed)."""
        g = self.grid
        G = g.global_grid if isinstance(g, TileGrid) else g
        act = np.ascontiguousarray(active).astype(np.uint8)
        if act.shape != (G.Ny, G.Nx):
            raise ValueError("mask must have the shape (Ny, Nx) of the (global) grid")
        # global mask with halos: periodic wrap; cells beyond a wall are inactive by definition
        full = np.zeros((G.Ny + 2 * G.Hy, G.Nx + 2 * G.Hx), dtype=np.uint8)
        full[G.Hy:G.Hy + G.Ny, G.Hx:G.Hx + G.Nx] = act
        if G.topology[0] is Periodic:
            full[:, :G.Hx] = full[:, G.Nx:G.Nx + G.Hx]
            full[:, G.Nx + G.Hx:] = full[:, G.Hx:2 * G.Hx]
        if G.topology[1] is Periodic:
            full[:G.Hy, :] = full[G.Ny:G.Ny + G.Hy, :]
            full[G.Ny + G.Hy:, :] = full[G.Hy:2 * G.Hy, :]
        if G.topology[1] is RightFolded:              # cells beyond the north fold are images of real cells
            from .grids import fold_north
            full = fold_north(full, G.Nx, G.Ny, G.Hx, G.Hy, False, False, 1).astype(np.uint8)
        if isinstance(g, TileGrid):
            full = np.ascontiguousarray(full[g.j_off:g.j_off + g.Ny + 2 * g.Hy, g.i_off:g.i_off + g.Nx + 2 * g.Hx])
        self.mask = torch.from_numpy(full).to(self.device)
        self.ctx.call("csi_mask_set", C.c_void_p(self.mask.data_ptr()), self.mask.shape[1])

    # ---- convenience ----------------------------------------------------------------------------
    @property
    def substeps(self):
        # (ExplicitSolver, StressBalanceFreeDrift as the dynamics: none)
        return 0 if self.dynamics is None else getattr(getattr(self.dynamics, "solver", None), "substeps", 0)

    @property
    def scheme(self):
        return 0 if self.advection is None else self.advection.scheme

    def diagnostics(self, what="all", extent_threshold=0.15):
        """Advection timescale, max|u|, max|v|, area-weighted volume / area / extent sums, extrema and non-finite counts computed on
        the device (diagnostics.py, include/csi.h csi_diagnostics_compute): what = "all", "velocity" or "tracers".  Waits for the
        library's stream; collective on a tiled model.  Returns an immutable Diagnostics record."""
        from .diagnostics import diagnostics
        return diagnostics(self, what, extent_threshold)

    def regional_diagnostics(self, regions, extent_threshold=0.15):
        """The tracer group of diagnostics() per region of a csi.Regions map -- volume, area, extent, snow volume, region area, extrema
        and cell counts as one vector per quantity --, reduced on the device in the diagnostics' summation order (regions.py,
        include/csi.h csi_regions_compute).  Waits for the library's stream; collective on a tiled model."""
        from .regions import regional_diagnostics
        return regional_diagnostics(self, regions, extent_threshold)

    # ---- derived fields and energy budget integrals (derived.py; include/csi.h csi_derived_compute / csi_budget_compute) ----------
    def derived_field(self, name):
        """The (Center, Center) field of a derived quantity -- "divergence", "shear", "deformation", "speed", "sigma_I", "sigma_II",
        "stress_power" --, allocated and bound to its slot the first time it is asked for.  compute_derived fills its interior."""
        from .derived import slot_of
        fld = self._derived_fields[name] = self._lazy_slot_field(slot_of(name), name)
        return fld

    def compute_derived(self, *names):
        """Fill the named derived fields from the current state, all in ONE launch on the library's stream (no copy, no wait: an
        output writer's pack launch, queued next, reads them; synchronize() before reading them with torch / numpy).  Returns the
        fields in the order of the names.  The stress group needs an ElastoViscoPlasticRheology (CsiError naming sigma11 otherwise)."""
        from .derived import mask_of
        mask = mask_of(names)
        fields = [self.derived_field(n) for n in names]
        self.ctx.derived_compute(mask)
        return fields

    def energy_budget(self, what="all"):
        """Work of the stress divergence, stress power, their relative imbalance and the kinetic energy, summed on the device in the
        diagnostics' order (derived.py): what = "all", "stress" or "kinetic".  Waits for the library's stream; collective on a tiled
        model.  Returns an immutable EnergyBudget record."""
        from .derived import energy_budget
        return energy_budget(self, what)

    # ---- momentum balance terms, interface stresses and their power (momentum_terms.py; include/csi.h) -----------------------------
    def momentum_term(self, name):
        """The field of one component of a momentum balance term -- "coriolis_x", "top_y", "bottom_x", "internal_y", "forcing_x", ...: a
        force per unit area at the u (_x) or v (_y) points --, allocated and bound to its slot the first time it is asked for.
        compute_momentum_terms fills its interior."""
        from .momentum_terms import slot_of
        fld = self._momentum_term_fields[name] = self._lazy_slot_field(slot_of(name), name)
        return fld

    def compute_momentum_terms(self, *names):
        """Fill the named term fields from the current state, all in ONE launch on the library's stream (no copy, no wait;
        synchronize() before reading them with torch / numpy).  A term's name without a component ("top") stands for both.  Returns
        the fields in the order of the names, x before y."""
        from .momentum_terms import expand, mask_of, terms_of
        mask = mask_of(names)
        fields = [self.momentum_term(n) for n in expand(names)]
        for n in expand(terms_of(mask)):              # a bit selects both components: both slots are bound
            self.momentum_term(n)
        self.ctx.momentum_terms_compute(mask)
        return fields

    def interface_stress(self, side):
        """(tau_x, tau_y) of side = "top" (air-ice) or "bottom" (ocean-ice): the reference's x_momentum_stress / y_momentum_stress
        (explicit - implicit * u) at the u / v points, in N m^-2.  The device computes them as the TOP / BOTTOM term slots without
        the interpolated-concentration factor and the sign, by a flag of the same launch: the fields returned ARE model.momentum_term
        (side + "_x" / "_y") and hold the stresses until the next compute_momentum_terms of that term.  The ocean receives
        -compute_momentum_terms("bottom"), the area-weighted force, not this bare stress."""
        from .momentum_terms import interface_stress
        return interface_stress(self, side)

    def momentum_budget(self, what="all"):
        """The power of each term of the momentum balance, sum u F_x Az + v F_y Az, summed on the device in the diagnostics' order
        (momentum_terms.py): what = "all", "external", "body", "internal" or a tuple.  Waits for the library's stream; collective on a
        tiled model.  Returns an immutable MomentumBudget record."""
        from .momentum_terms import momentum_budget
        return momentum_budget(self, what)

    def tracer(self, name):
        """The CenterField of an advected tracer by name (SeaIceModel(..., tracers = ...); tracers.py)."""
        if name not in self.tracers:
            raise KeyError(f"tracer: the model has no tracer named {name!r} (it has: {', '.join(self.tracers) or 'none'})")
        return self.tracers[name]

    def synchronize(self):
        """Wait for the library's stream (call before reading fields with torch / numpy)."""
        self.ctx.call("csi_sync")

    def copy_to_field(self, fld, array):
        """Overwrite a field's parent array from a host array of the same shape (ordered with the library)."""
        self.synchronize()
        fld.data.copy_(torch.from_numpy(np.ascontiguousarray(array, dtype=np.float64)))
        torch.cuda.synchronize(self.device)


def set_(model, **kw):
    """set!(model; h, aice (or ℵ), u, v) then update_state! (sea_ice_model.jl:301-315)."""
    # Python NFKC-normalises identifiers, so the keyword `ℵ` (U+2135) arrives as U+05D0
    names = {"h": model.ice_thickness, "aice": model.ice_concentration, "\u2135": model.ice_concentration,
             "\u05d0": model.ice_concentration, "u": model.velocities.u, "v": model.velocities.v}
    if model.snow_thickness is not None:
        names["hs"] = model.snow_thickness
    names.update(getattr(model, "tracers", {}))
    for k, val in kw.items():
        if k not in names:
            raise KeyError(f"set!: unknown field {k}")
        names[k].set(val)
    torch.cuda.synchronize(model.device)   # torch wrote on its stream; the library uses its own
    update_state(model)
    model.synchronize()                    # ... and whoever reads the fields next (torch / numpy) sees the filled halos


def update_state(model):
    model.update_time_series()
    model.ctx.call("csi_update_state")


def _state_fields(model):
    """name -> Field of what Oceananigans.prognostic_state(model) saves (sea_ice_model.jl:414-426): velocities, ice
    thickness / concentration, snow thickness, the time stepper's G^n and Psi^-, the dynamics' auxiliary fields, the mass fluxes,
    the thermodynamics' top surface temperatures, and "tracers.<name>" for the advected tracers of a model that has them (tracers.py;
    their tendencies travel with G^n, and the library's Psi^- copies are rebuilt by every RK3 step).  Not mirrored: the clock's fields
    beyond (time, iteration)."""
    out = {"u": model.velocities.u, "v": model.velocities.v, "h": model.ice_thickness, "aice": model.ice_concentration}
    if model.snow_thickness is not None:
        out["hs"] = model.snow_thickness
    for name, f in getattr(model, "tracers", {}).items():
        out["tracers." + name] = f
    for k, f in vars(model.timestepper.Gn).items():
        out["Gn." + k] = f
    if model.timestepper.Psi_minus is not None:
        for k, f in vars(model.timestepper.Psi_minus).items():
            out["Psi_minus." + k] = f
    if isinstance(model.dynamics, SeaIceMomentumEquation):      # (StressBalanceFreeDrift as the dynamics: no fields, :46)
        for k, f in vars(model.dynamics.auxiliaries.fields).items():
            out["dynamics." + k] = f
    if model.mass_fluxes is not None:
        mf = model.mass_fluxes
        out.update({"mass_fluxes.ice": mf.thermodynamics.ice, "mass_fluxes.snow": mf.thermodynamics.snow,
                    "mass_fluxes.intercepted_snowfall": mf.intercepted_snowfall})
    # ice_thermodynamics / snow_thermodynamics (sea_ice_model.jl:422-423): their top_surface_temperature fields (the layered
    # step's outputs, bound as TU / TUS) where the model has them
    for key, name in (("ice_thermodynamics.top_surface_temperature", "ice_top_temperature"),
                      ("snow_thermodynamics.top_surface_temperature", "snow_top_temperature")):
        f = getattr(model, name, None)
        if f is not None:
            out[key] = f
    if getattr(model, "ocean", None) is not None:      # the mixed-layer temperature and its Psi^- copy
        out.update(model.ocean.state_fields())
    return {k: f for k, f in out.items() if isinstance(f, Field)}


def prognostic_state(model):
    """Oceananigans.prognostic_state(model) (sea_ice_model.jl:414-426): host copies of the whole parent arrays (halos included)
    plus the clock.  The library keeps no state of its own between calls -- pointers, scratch that every sub-cycle rebuilds --
    so this is all a checkpoint needs (tests/test_gpu_steps.py::test_checkpoint_round_trip_bitwise)."""
    # (a tiled model: the collective check -- csi_sync on every rank + the halo transport's status reduced over ALL ranks -- so that a
    #  checkpoint is never written from an aborted sub-cycle's fields; every rank of the decomposition saves at the same step)
    if isinstance(model.grid, TileGrid):
        model.ctx.validate_all()
    else:
        model.synchronize()
    state = {k: f.numpy().copy() for k, f in _state_fields(model).items()}
    state["clock"] = (model.clock.time, model.clock.iteration)
    if getattr(model, "drifters", None) is not None:      # drifters.xi, drifters.eta, drifters.status: only when drifters are set
        state.update(model.drifters.state())
    return state


def restore_prognostic_state(model, state):
    """Oceananigans.restore_prognostic_state!(model, state) (sea_ice_model.jl:428-445): writes the saved parents back into the
    fields the library is bound to (same arrays: nothing to re-attach)."""
    for k, f in _state_fields(model).items():
        if k in state:
            model.copy_to_field(f, state[k])
    model.clock.time, model.clock.iteration = state["clock"]
    if getattr(model, "drifters", None) is not None and "drifters.xi" in state:
        model.drifters.restore(state, model)
    return model


def time_step_momentum(model, dt, rk_reset=False):
    """time_step_momentum!(model, model.dynamics, dt): split_explicit_momentum_equations.jl:103-195 (EVP or viscous sub-cycle;
    rk_reset: reset_velocities! from Psi^-) or explicit_momentum_equations.jl:8-38 (ExplicitSolver: u^- = Psi^-.u when rk_reset,
    the current velocities otherwise; G^n from compute_momentum_tendencies) or, with StressBalanceFreeDrift as the dynamics,
    stress_balance_free_drift.jl:132-143: u, v = the free-drift velocity at every point (dt and rk_reset are not read; model.substeps
    is 0 and the fusion / tile-skipping switches are accepted and ignored: there is no sub-cycle)."""
    model.update_time_series()
    model.ctx.call("csi_time_step_momentum", float(dt), model.substeps, int(rk_reset))


def compute_momentum_tendencies(model, dt):
    """compute_momentum_tendencies!(model, model.dynamics, dt): G^n.u / G^n.v of the ExplicitSolver (explicit_momentum_equations.jl:
    85-113); nothing for the split-explicit solver."""
    model.update_time_series()
    model.ctx.call("csi_compute_momentum_tendencies", float(dt))


def time_step(model, dt):
    """time_step!(model, dt).  Forcing time series are interpolated at the time the step starts from: every stage reads the same
    forcing, as in the reference, whose tick! follows the stages.  Output writers (model.output_writers) write their initial record
    before the first step and are driven at the end of every step, once the clock has advanced and a tiled model has been validated."""
    for writer in model.output_writers.values():
        writer.begin(model)
    model.update_time_series()
    if model.dynamics is None and model.scheme in (0, None):
        # dynamics = nothing, advection = nothing: the step is the thermodynamic update alone
        # (sea_ice_fe_step.jl:13-34 with time_step_momentum!, compute_tendencies! and dynamic_time_step! no-ops)
        if model.ice_thermodynamics is None:
            raise NotImplementedError("a model without dynamics, advection and thermodynamics has nothing to step")
        if model.ocean is not None:      # the ocean under the ice first: it writes the bottom heat flux the ice step reads
            model.ctx.mixed_layer_step(dt, False)
        if model.snow_thermodynamics is None:
            model.ctx.call("csi_slab_thermo_step", C.byref(model._slab_params), float(dt))
        else:
            model.ctx.call("csi_layered_thermo_step", C.byref(model._slab_params), C.byref(model._snow_params), float(dt))
        model.ctx.call("csi_update_state")
    elif model.timestepper_kind == "ForwardEuler":
        model.ctx.call("csi_time_step_fe", float(dt), model.substeps, model.scheme, int(model.clock.iteration == 0))
    else:
        model.ctx.call("csi_time_step_rk3", float(dt), model.substeps, model.scheme)
    model.clock.time += float(dt)
    model.clock.iteration += 1
    # tiles: once per step, the state is checked on EVERY rank before anything between two steps (output, checkpoints, callbacks) reads
    # it -- what the Julia stub does in the update_state! that ends time_step! (julia/ClimaSeaIceHIP.jl)
    if isinstance(model.grid, TileGrid):
        model.ctx.validate_all()
    # Lagrangian drifters move with the velocities the step leaves, one launch, before the writers sample them (drifters.py)
    if getattr(model, "drifters", None) is not None:
        model.drifters.advance(model, float(dt), model.drifters.substeps)
    for writer in model.output_writers.values():
        writer.after_step(model, float(dt))
