"""ctypes binding of libcsi_hip.so (include/csi.h).

The HIP library is the product; there is no CPU fallback.  Importing this module never touches
the GPU; `load()` raises loudly when the shared library is missing, and every compute entry
point raises `CsiError` when there is no HIP device.
"""
import ctypes as C
import os

import numpy as np

from .grids import Center, Face

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CSI_HIP_LIBRARY", os.path.join(_HERE, "libcsi_hip.so"))   # override: A/B runs of two builds

# ---- enums (include/csi.h) ---------------------------------------------------------------------
OK = 0
PERIODIC, BOUNDED, FULLY_CONNECTED, LEFT_CONNECTED, RIGHT_CONNECTED, RIGHT_FOLDED, LEFT_CONNECTED_RIGHT_FOLDED = 0, 1, 2, 3, 4, 5, 6
METRIC_UNIFORM, METRIC_PER_J, METRIC_FULL = 0, 1, 2
# ---- the field slots of csi_field_bind: include/csi.h's eight chained enums; csrc/csi_slots.h states the same table for the library ----
# One row per slot, in id order: (NAME, the name the library's messages print, (LX, LY), roles).  A new slot is one row here.
SLOT_HALO, SLOT_PEER, SLOT_FORCING, SLOT_SERIES = 1, 2, 4, 8      # csrc/csi_slots.h: what each role means
_H, _HP, _HFS, _S = SLOT_HALO, SLOT_HALO | SLOT_PEER, SLOT_HALO | SLOT_FORCING | SLOT_SERIES, SLOT_SERIES
_cc, _fc, _cf, _ff = (Center, Center), (Face, Center), (Center, Face), (Face, Face)
SLOTS = [
    ("U", "u", _fc, _HP), ("V", "v", _cf, _HP), ("H", "h", _cc, _H), ("A", "aice", _cc, _H), ("S11", "sigma11", _cc, _HP),
    ("S22", "sigma22", _cc, _HP), ("S12", "sigma12", _ff, _HP), ("UN", "un", _fc, _H), ("VN", "vn", _cf, _H), ("P", "P", _cc, _H),
    ("ALPHA", "alpha", _cc, _HP), ("DELTA", "Delta", _cc, _HP), ("ZETA_F", "zeta_f", _ff, _HP), ("ZETA_C", "zeta_c", _cc, _HP),
    ("GH", "Gh", _cc, _H), ("GA", "Gaice", _cc, _H), ("HM", "h-", _cc, _H), ("AM", "aice-", _cc, _H), ("UM", "u-", _fc, _H), ("VM", "v-", _cf, _H),
    ("TOP_U", "top_u", _fc, _HFS), ("TOP_V", "top_v", _cf, _HFS), ("BOT_U", "bottom_u", _fc, _HFS), ("BOT_V", "bottom_v", _cf, _HFS),
    ("MASS_FLUX", "mass_flux", _cc, _H), ("HS", "hs", _cc, _H), ("GHS", "Ghs", _cc, _H), ("HSM", "hs-", _cc, _H),
    ("MASS_FLUX_SNOW", "mass_flux_snow", _cc, _H), ("SNOWFALL_INTERCEPTED", "intercepted_snowfall", _cc, _H), ("TU", "Tu", _cc, _H),
    ("TUS", "Tu_snow", _cc, _H), ("FORCING_U", "forcing_u", _fc, _HFS), ("FORCING_V", "forcing_v", _cf, _HFS), ("GU", "Gu", _fc, _H),
    ("GV", "Gv", _cf, _H), ("TOP_HEAT_FLUX", "top_heat_flux", _cc, _S), ("BOTTOM_HEAT_FLUX", "bottom_heat_flux", _cc, _S),
    ("SNOWFALL", "snowfall", _cc, _S), ("FREE_DRIFT_U", "free_drift_u", _fc, _HFS), ("FREE_DRIFT_V", "free_drift_v", _cf, _HFS),
    ("D_DIVERGENCE", "divergence", _cc, 0), ("D_SHEAR", "shear", _cc, 0), ("D_DEFORMATION", "deformation", _cc, 0), ("D_SPEED", "speed", _cc, 0),
    ("D_SIGMA_I", "sigma_I", _cc, 0), ("D_SIGMA_II", "sigma_II", _cc, 0), ("D_STRESS_POWER", "stress_power", _cc, 0),
    ("M_CORIOLIS_X", "coriolis_x", _fc, 0), ("M_CORIOLIS_Y", "coriolis_y", _cf, 0), ("M_TOP_X", "top_x", _fc, 0), ("M_TOP_Y", "top_y", _cf, 0),
    ("M_BOTTOM_X", "bottom_x", _fc, 0), ("M_BOTTOM_Y", "bottom_y", _cf, 0), ("M_INTERNAL_X", "internal_x", _fc, 0),
    ("M_INTERNAL_Y", "internal_y", _cf, 0), ("M_FORCING_X", "forcing_x", _fc, 0), ("M_FORCING_Y", "forcing_y", _cf, 0),
    ("FLUX_COEFFICIENT", "flux_coefficient", _cc, _S), ("FLUX_REFERENCE_TEMPERATURE", "flux_reference_temperature", _cc, _S),
    ("BOTTOM_SALINITY", "bottom_salinity", _cc, _S), ("TOP_HEAT_FLUX_USED", "top_heat_flux_used", _cc, 0),
    ("BOTTOM_HEAT_FLUX_USED", "bottom_heat_flux_used", _cc, 0), ("ML_TEMPERATURE", "ocean_temperature", _cc, 0),
    ("ML_TEMPERATURE_M", "ocean_temperature-", _cc, 0), ("ML_SURFACE_HEAT_FLUX", "ocean_surface_heat_flux", _cc, _S),
    ("ML_COEFFICIENT", "ocean_coefficient", _cc, _S), ("ML_REFERENCE_TEMPERATURE", "ocean_reference_temperature", _cc, _S),
    ("ML_DEEP_HEAT_FLUX", "ocean_deep_heat_flux", _cc, _S), ("ML_SURFACE_FLUX_USED", "ocean_surface_flux_used", _cc, 0),
    ("SHORTWAVE", "shortwave", _cc, _S), ("ALBEDO_USED", "albedo_used", _cc, 0)]
_NAMES = [row[0] for row in SLOTS]
_ID = {n: k for k, n in enumerate(_NAMES)}
_DISPLAY = {row[1]: row[0] for row in SLOTS}
# the eight enums, each from its first enumerator to the next one's; the last four cuts are the counts from CSI_F_COUNT_BINDABLE on
_cut = [_ID[n] for n in ("U", "TOP_HEAT_FLUX", "FREE_DRIFT_U", "D_DIVERGENCE", "M_CORIOLIS_X", "FLUX_COEFFICIENT", "ML_TEMPERATURE", "SHORTWAVE")] + [len(SLOTS)]
(FIELD_IDS, THERMO_FIELD_IDS, FREE_DRIFT_FIELD_IDS, DERIVED_FIELD_IDS, MOMENTUM_TERM_FIELD_IDS, THERMO_LINEAR_FIELD_IDS,
 MIXED_LAYER_FIELD_IDS, SHORTWAVE_FIELD_IDS) = (_NAMES[a:b] for a, b in zip(_cut, _cut[1:]))
F, F_DERIVED, F_MOMENTUM_TERMS, F_THERMO_LINEAR, F_MIXED_LAYER, F_SHORTWAVE = ({n: _ID[n] for n in _NAMES[a:b]} for a, b in zip([0] + _cut[3:], _cut[3:]))
F_COUNT_BINDABLE, F_COUNT_THERMO, F_COUNT_MIXED_LAYER, F_COUNT_SHORTWAVE = _cut[5:]
# the slots a time series may drive (csi_time_series_set): of F the forcing slots first, then the others; the younger enums' in their own lists
_series = [row[0] for row in SLOTS if row[3] & SLOT_SERIES]
SERIES_SLOTS = sorted((n for n in _series if n in F), key=lambda n: not SLOTS[_ID[n]][3] & SLOT_FORCING)
THERMO_SERIES_SLOTS, MIXED_LAYER_SERIES_SLOTS, SHORTWAVE_SERIES_SLOTS = ([n for n in _series if n in t] for t in (F_THERMO_LINEAR, F_MIXED_LAYER, F_SHORTWAVE))


def slot_id(name):
    """The number of a csi_field_bind slot by name; "TRACER:k" is tracer k as an output field, CSI_TRACER_FIELD(k) (no slot)."""
    if name.startswith("TRACER:"):
        return 4096 + int(name[7:])
    return _ID[name]


def slot_location(name):
    """(LX, LY) of a slot by name: grids.Center / grids.Face."""
    if name.startswith("TRACER:"):
        return SLOTS[_ID["H"]][2]
    return SLOTS[_ID[name]][2]


def slot_of_display_name(display):
    """The slot's name ("ML_COEFFICIENT") for the name the library's messages print ("ocean_coefficient")."""
    return _DISPLAY[display]


STRESS_NONE, STRESS_CONST, STRESS_FIELD, STRESS_SEMI_IMPLICIT = 0, 1, 2, 3
VEL_ZERO, VEL_CONST, VEL_FIELD = 0, 1, 2
STRESS_TOP, STRESS_BOTTOM = 0, 1
MODE_STRICT, MODE_FAST = 0, 1
PRESSURE_REPLACEMENT, PRESSURE_ICE_STRENGTH = 0, 1
RHEOLOGY_EVP, RHEOLOGY_VISCOUS = 0, 1
SOLVER_SPLIT_EXPLICIT, SOLVER_EXPLICIT = 0, 1
FREE_DRIFT_NONE, FREE_DRIFT_STRESS_BALANCE, FREE_DRIFT_FIELDS = 0, 1, 2
DYNAMICS_MOMENTUM_EQUATION, DYNAMICS_FREE_DRIFT = 0, 1
FLUX_CONSTANT, FLUX_ARRAY, FLUX_RADIATIVE_EMISSION, FLUX_LINEAR, FLUX_SHORTWAVE = 0, 1, 2, 3, 4
WEIGHT_NONE, WEIGHT_CONCENTRATION, WEIGHT_ICE_PRESENT = 0, 1, 2
LINEAR_WEIGHT_MASK, LINEAR_COEFFICIENT_ARRAY, LINEAR_REFERENCE_ARRAY = 3, 4, 8      # csi_heat_flux_term.reserved of a LINEAR term
SOLVE_BOTTOM_SALINITY_ARRAY = 1                                                     # csi_surface_solve.reserved
HEAT_TOP, HEAT_BOTTOM = 0, 1
MAX_HEAT_FLUX_TERMS = 8
TIME_CLAMP, TIME_CYCLICAL, TIME_LINEAR = 0, 1, 2
SERIES_DEVICE, SERIES_HOST = 0, 1
REGRID_FACE_CENTER, REGRID_CENTER_FACE, REGRID_CENTER_CENTER = 0, 1, 2      # csi_regrid_location
REGRID_MAX_MAPS, REGRID_MAX_SOURCE_EXTENT = 16, 65536
ML_SURFACE_ARRAY, ML_BULK_ARRAYS, ML_DEEP_ARRAY, ML_HAS_SURFACE, ML_HAS_BULK = 1, 2, 4, 8, 16      # csi_mixed_layer_params.flags

# every symbol include/csi.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = ["csi_version", "csi_context_create", "csi_context_destroy", "csi_last_error", "csi_sync", "csi_set_mode",
           "csi_grid_set", "csi_mask_set", "csi_field_bind", "csi_evp_params_set", "csi_stress_set",
           "csi_evp_initialize", "csi_evp_subcycle", "csi_evp_finalize", "csi_time_step_momentum",
           "csi_compute_tracer_tendencies", "csi_dynamic_step_tracers", "csi_cache_current_fields",
           "csi_update_state", "csi_fill_halo_local", "csi_time_step_fe", "csi_time_step_rk3",
           "csi_slab_thermo_step", "csi_slab_params_set", "csi_layered_thermo_step", "csi_snow_params_set", "csi_tile_set", "csi_comm_unique_id", "csi_comm_init", "csi_comm_count", "csi_local_group_create", "csi_local_group_destroy", "csi_comm_init_local", "csi_comm_init_host", "csi_halo_exchange",
           "csi_plan_exchange", "csi_set_fusion", "csi_set_exchange_interval", "csi_set_halo_transport", "csi_halo_transport", "csi_set_peer_tier", "csi_peer_tier", "csi_plan_ranges", "csi_profile_substeps", "csi_last_path", "csi_last_advection", "csi_last_subcycle_ms", "csi_launches_per_substep", "csi_last_launches", "csi_plan_pair", "csi_plan_peer_chunks", "csi_free_drift_set", "csi_coriolis_rows_set", "csi_velocity_bc_set",
           "csi_immersed_flux_bc_set", "csi_coriolis_points_set", "csi_validate_all", "csi_debug_peer_abort", "csi_set_weno_weight_dtype", "csi_weno_weight_dtype", "csi_subcycle_stats_begin", "csi_subcycle_stats_end",
           "csi_set_tile_skipping", "csi_tile_activity", "csi_set_row_constant", "csi_row_constant_rows",
           "csi_rheology_set", "csi_momentum_solver_set", "csi_compute_momentum_tendencies",
           "csi_heat_fluxes_set", "csi_surface_solve_set", "csi_dynamics_set",
           "csi_time_series_plan", "csi_time_series_set", "csi_time_series_update", "csi_time_series_status",
           "csi_regrid_plan_axis", "csi_regrid_map_create", "csi_regrid_map_destroy", "csi_time_series_set_regridded", "csi_regrid_stats",
           "csi_diagnostics_compute",
           "csi_output_plan_layout", "csi_output_create", "csi_output_layout", "csi_output_record_bytes", "csi_output_accumulate",
           "csi_output_snapshot", "csi_output_test", "csi_output_wait", "csi_output_release", "csi_output_destroy",
           "csi_derived_compute", "csi_budget_compute", "csi_derived_stats",
           "csi_momentum_terms_compute", "csi_momentum_budget_compute", "csi_momentum_terms_stats",
           "csi_mixed_layer_set", "csi_mixed_layer_step", "csi_mixed_layer_stats", "csi_shortwave_set", "csi_last_thermo",
           "csi_enthalpy_plan", "csi_enthalpy_create", "csi_enthalpy_destroy", "csi_enthalpy_bind", "csi_enthalpy_boundary_set",
           "csi_enthalpy_set", "csi_enthalpy_update_state", "csi_enthalpy_time_step", "csi_enthalpy_last_launch",
           "csi_enthalpy_ice_thickness",
           "csi_drifters_locate", "csi_drifters_advance", "csi_drifters_sample", "csi_drifters_stats",
           "csi_regions_layout", "csi_regions_compute", "csi_regions_stats",
           "csi_tracers_set", "csi_tracers_tendencies", "csi_tracers_update", "csi_tracers_stats", "csi_tracers_last"]
# per-region ice integrals and extrema (include/csi.h): the most regions one call takes
REGIONS_MAX = 64
# Lagrangian ice drifters (include/csi.h): the status bits of csi_drifters_advance, the column bits of csi_drifters_sample
DRIFTER_CLAMPED_X, DRIFTER_CLAMPED_Y, DRIFTER_HELD, DRIFTER_LOST, DRIFTER_INACTIVE = 1, 2, 4, 8, 16
DRIFTER_COL_XI, DRIFTER_COL_ETA, DRIFTER_COL_U, DRIFTER_COL_V, DRIFTER_COL_H, DRIFTER_COL_A, DRIFTER_COL_HS, DRIFTER_COL_ALL = 1, 2, 4, 8, 16, 32, 64, 127
# the enthalpy-method column model (include/csi.h): csi_enthalpy_array, csi_enthalpy_side, csi_enthalpy_bc_kind, the two forms, the rule's constants
ENTH_H, ENTH_T, ENTH_PHI, ENTH_KAPPA = 0, 1, 2, 3
ENTH_T_BOTTOM, ENTH_T_TOP, ENTH_H_BOTTOM, ENTH_H_TOP = 0, 1, 2, 3
ENTH_BC_NONE, ENTH_BC_NUMBER, ENTH_BC_ARRAY, ENTH_BC_SERIES_SCALAR, ENTH_BC_SERIES_PLANE, ENTH_BC_FLUX, ENTH_BC_GRADIENT = range(7)
ENTH_PER_STEP, ENTH_ON_CHIP = 1, 2
ENTH_MAX_SUBSTEPS, ENTH_MIN_WAVES_PER_CU, ENTH_LDS_PER_CU = 64, 2, 163840
DIAG_VELOCITY, DIAG_TRACERS, DIAG_ALL = 1, 2, 3
OUT_F64, OUT_F32 = 0, 1
DERIVED_ALL = 127
BUDGET_STRESS, BUDGET_KINETIC, BUDGET_ALL = 1, 2, 3
MTERM_CORIOLIS, MTERM_TOP, MTERM_BOTTOM, MTERM_INTERNAL, MTERM_FORCING, MTERM_ALL, MTERM_RAW_STRESS = 1, 2, 4, 8, 16, 31, 32
MBUDGET_EXTERNAL, MBUDGET_BODY, MBUDGET_INTERNAL, MBUDGET_ALL = 1, 2, 4, 7
OUTPUT_MAX_FIELDS, OUTPUT_MAX_SETS, OUTPUT_MAX_SLOTS = 16, 4, 64


class Metrics(C.Structure):
    _fields_ = [("dx", C.c_double), ("dy", C.c_double),
                ("dxc", C.POINTER(C.c_double)), ("dxf", C.POINTER(C.c_double)),
                ("azc", C.POINTER(C.c_double)), ("azf", C.POINTER(C.c_double)),
                ("full", C.POINTER(C.c_double) * 12), ("full_ld", C.c_int64)]


class EvpParams(C.Structure):
    _fields_ = [("ice_compressive_strength", C.c_double), ("ice_compaction_hardening", C.c_double),
                ("yield_curve_eccentricity", C.c_double), ("minimum_plastic_stress", C.c_double),
                ("min_relaxation_parameter", C.c_double), ("max_relaxation_parameter", C.c_double),
                ("relaxation_strength", C.c_double), ("pressure_formulation", C.c_int32), ("has_coriolis", C.c_int32),
                ("coriolis_f", C.c_double), ("minimum_concentration", C.c_double), ("minimum_mass", C.c_double),
                ("sea_ice_density", C.c_double)]


class Stress(C.Structure):
    _fields_ = [("kind", C.c_int32), ("ue_kind", C.c_int32), ("ve_kind", C.c_int32), ("reserved", C.c_int32),
                ("tau_u", C.c_double), ("tau_v", C.c_double), ("ue", C.c_double), ("ve", C.c_double),
                ("rho_e", C.c_double), ("Cd", C.c_double)]


class SlabParams(C.Structure):
    _fields_ = [("conductivity", C.c_double), ("sea_ice_density", C.c_double), ("density", C.c_double),
                ("liquid_density", C.c_double), ("liquid_heat_capacity", C.c_double), ("heat_capacity", C.c_double),
                ("reference_latent_heat", C.c_double), ("reference_temperature", C.c_double),
                ("liquidus_slope", C.c_double), ("freshwater_melting_temperature", C.c_double),
                ("bottom_salinity", C.c_double), ("ice_consolidation_thickness", C.c_double),
                ("top_temperature", C.c_double), ("top_flux_kind", C.c_int32), ("bottom_flux_kind", C.c_int32),
                ("top_heat_flux", C.c_double), ("bottom_heat_flux", C.c_double),
                ("top_bc_kind", C.c_int32), ("pad_", C.c_int32), ("ice_salinity", C.c_double)]


class SnowParams(C.Structure):
    _fields_ = [("conductivity", C.c_double), ("snow_density", C.c_double), ("snowfall", C.c_double),
                ("top_temperature", C.c_double), ("top_bc_kind", C.c_int32), ("pad_", C.c_int32)]


class HeatFluxTerm(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("value", C.c_double), ("emissivity", C.c_double),
                ("stefan_boltzmann_constant", C.c_double), ("reference_temperature", C.c_double)]


class SurfaceSolve(C.Structure):
    _fields_ = [("tol", C.c_double), ("maxiters", C.c_int32), ("prescribed_array", C.c_int32), ("snowfall_array", C.c_int32),
                ("reserved", C.c_int32)]


class MixedLayerParams(C.Structure):
    """csi_mixed_layer_params (include/csi.h): the slab-ocean mixed layer."""
    _fields_ = [("density", C.c_double), ("heat_capacity", C.c_double), ("depth", C.c_double), ("exchange_velocity", C.c_double),
                ("surface_heat_flux", C.c_double), ("coefficient", C.c_double), ("reference_temperature", C.c_double),
                ("deep_heat_flux", C.c_double), ("flags", C.c_int32), ("reserved", C.c_int32)]


class Shortwave(C.Structure):
    """csi_shortwave (include/csi.h): the SHORTWAVE top term's flux, its stepped albedo for ice and for snow, weighting and flags."""
    _fields_ = [("flux", C.c_double), ("cold", C.c_double), ("warm", C.c_double), ("threshold", C.c_double),
                ("snow_cold", C.c_double), ("snow_warm", C.c_double), ("snow_threshold", C.c_double),
                ("weighting", C.c_int32), ("per_cell", C.c_int32), ("has_snow_pair", C.c_int32), ("reserved", C.c_int32)]


class TimeSeries(C.Structure):
    _fields_ = [("nt", C.c_int32), ("indexing", C.c_int32), ("backend", C.c_int32), ("window", C.c_int32), ("period", C.c_double),
                ("times", C.POINTER(C.c_double)), ("data", C.c_void_p), ("ld", C.c_int64), ("slice_stride", C.c_int64)]


class RegridMap(C.Structure):
    """csi_regrid_map (include/csi.h): one location's target points on a source grid -- indices, weights and optionally the rotation."""
    _fields_ = [("location", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("src_nx", C.c_int32), ("src_ny", C.c_int32),
                ("reserved", C.c_int32), ("i0", C.POINTER(C.c_int32)), ("i1", C.POINTER(C.c_int32)), ("j0", C.POINTER(C.c_int32)),
                ("j1", C.POINTER(C.c_int32)), ("wx", C.POINTER(C.c_double)), ("wy", C.POINTER(C.c_double)),
                ("cos", C.POINTER(C.c_double)), ("sin", C.POINTER(C.c_double))]


class Diagnostics(C.Structure):
    """csi_diagnostics (include/csi.h): "not computed" members hold NaN (doubles) / -1 (counts)."""
    _fields_ = ([("what", C.c_int32), ("has_snow", C.c_int32)] +
                [(n, C.c_double) for n in ("advection_timescale", "inv_timescale_max", "max_abs_u", "max_abs_v")] +
                [(n, C.c_int64) for n in ("nonfinite_u", "nonfinite_v", "nan_u", "nan_v")] +
                [(n, C.c_double) for n in ("ice_volume", "ice_area", "ice_extent", "snow_volume", "active_area",
                                           "min_h", "max_h", "min_aice", "max_aice", "max_hs")] +
                [(n, C.c_int64) for n in ("nonfinite_h", "nonfinite_aice", "nonfinite_hs", "active_cells")] +
                [("extent_threshold", C.c_double)])


class Budget(C.Structure):
    """csi_budget (include/csi.h): members of a group that was not requested hold NaN."""
    _fields_ = [("what", C.c_int32), ("reserved", C.c_int32), ("internal_work", C.c_double), ("stress_power", C.c_double),
                ("kinetic_energy", C.c_double)]


class MomentumBudget(C.Structure):
    """csi_momentum_budget (include/csi.h): members of a group that was not requested hold NaN."""
    _fields_ = [("what", C.c_int32), ("reserved", C.c_int32), ("coriolis", C.c_double), ("top", C.c_double), ("bottom", C.c_double),
                ("internal", C.c_double), ("forcing", C.c_double)]


class OutputField(C.Structure):
    """csi_output_field (include/csi.h): one field of an output set."""
    _fields_ = [("field_id", C.c_int32), ("dtype", C.c_int32), ("averaged", C.c_int32), ("masked", C.c_int32),
                ("fill_value", C.c_double)]


class EnthalpyParams(C.Structure):
    """csi_enthalpy_params (include/csi.h): the enthalpy-method column model's extents, faces and parameters."""
    _fields_ = [("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32), ("reserved", C.c_int32), ("z_faces", C.POINTER(C.c_double)),
                ("ice_heat_capacity", C.c_double), ("water_heat_capacity", C.c_double), ("fusion_enthalpy", C.c_double),
                ("kappa_ice", C.c_double), ("kappa_water", C.c_double)]


class EnthalpyLaunch(C.Structure):
    """csi_enthalpy_launch (include/csi.h): what the last csi_enthalpy_time_step launched."""
    _fields_ = [("form", C.c_int32), ("launches", C.c_int32), ("substeps_per_launch", C.c_int32), ("lds_bytes", C.c_int32)]


class Drifters(C.Structure):
    """csi_drifters (include/csi.h): the caller's device arrays of n drifters."""
    _fields_ = [("n", C.c_int64), ("xi", C.c_void_p), ("eta", C.c_void_p), ("status", C.c_void_p)]


class Regions(C.Structure):
    """csi_regions (include/csi.h): the caller's device id map, laid out like a (c,c) parent."""
    _fields_ = [("ids", C.c_void_p), ("ld", C.c_int64), ("n_regions", C.c_int32), ("reserved", C.c_int32)]


class RegionRecord(C.Structure):
    """csi_region_record (include/csi.h): the tracer group of one region; snow members hold NaN without a snow layer."""
    _fields_ = ([(n, C.c_double) for n in ("ice_volume", "ice_area", "ice_extent", "snow_volume", "region_area",
                                           "min_h", "max_h", "min_aice", "max_aice", "max_hs")] + [("cells", C.c_int64)])


TRACERS_MAX = 8
TRACER_PLAIN, TRACER_BY_CONCENTRATION = 0, 1


def tracer_field(k):
    """CSI_TRACER_FIELD(k) (include/csi.h): tracer k as an output field id."""
    return 4096 + int(k)


class Tracers(C.Structure):
    """csi_tracers (include/csi.h): the caller's tracer arrays (parent shape of h), optional tendency arrays and per-tracer flags."""
    _fields_ = [("n", C.c_int32), ("c", C.c_void_p * TRACERS_MAX), ("G", C.c_void_p * TRACERS_MAX),
                ("weighting", C.c_int32 * TRACERS_MAX), ("nonnegative", C.c_int32 * TRACERS_MAX), ("source", C.c_double * TRACERS_MAX)]


class CsiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libcsi_hip error {code}: {msg}")
        self.code = code


_lib = None


def load():
    """Load libcsi_hip.so; fail loudly if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(make -C climaseaice.jl_amd/csrc).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.csi_version.restype = i32
    L.csi_last_error.restype = C.c_char_p
    L.csi_last_error.argtypes = [vp]
    sig = {
        "csi_context_create": [i32, vp, C.POINTER(vp)],
        "csi_context_destroy": [vp], "csi_sync": [vp], "csi_set_mode": [vp, i32],
        "csi_grid_set": [vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(Metrics)],
        "csi_mask_set": [vp, vp, i64],
        "csi_field_bind": [vp, i32, vp, i64, i32, i32],
        "csi_evp_params_set": [vp, C.POINTER(EvpParams)],
        "csi_stress_set": [vp, i32, C.POINTER(Stress)],
        "csi_evp_initialize": [vp], "csi_evp_subcycle": [vp, dbl, i32, i32], "csi_evp_finalize": [vp],
        "csi_time_step_momentum": [vp, dbl, i32, i32],
        "csi_compute_tracer_tendencies": [vp, i32], "csi_dynamic_step_tracers": [vp, dbl, i32],
        "csi_cache_current_fields": [vp], "csi_update_state": [vp], "csi_fill_halo_local": [vp, i32],
        "csi_time_step_fe": [vp, dbl, i32, i32, i32], "csi_time_step_rk3": [vp, dbl, i32, i32],
        "csi_slab_thermo_step": [vp, C.POINTER(SlabParams), dbl],
        "csi_slab_params_set": [vp, C.POINTER(SlabParams)],
        "csi_layered_thermo_step": [vp, C.POINTER(SlabParams), C.POINTER(SnowParams), dbl],
        "csi_snow_params_set": [vp, C.POINTER(SnowParams)],
        "csi_tile_set": [vp, i32, i32, i32, i32, i32, i32],
        "csi_comm_unique_id": [C.POINTER(C.c_uint8)],
        "csi_comm_init": [vp, i32, i32, C.POINTER(C.c_uint8)],
        "csi_comm_count": [vp, C.POINTER(i32)],
        "csi_local_group_create": [i32, C.POINTER(vp)], "csi_comm_init_local": [vp, vp, i32],
        "csi_comm_init_host": [vp, C.c_char_p, i32, i32],
        "csi_halo_exchange": [vp, C.POINTER(i32), i32, i32],
        "csi_plan_ranges": [i32, i32, i32, i32, i32, i32, i32, C.POINTER(i32)],
        "csi_plan_pair": [i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(i32)],
        "csi_plan_peer_chunks": [i32, i32, i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), i32],
        "csi_set_exchange_interval": [vp, i32],
        "csi_set_halo_transport": [vp, i32], "csi_halo_transport": [vp, C.POINTER(i32)],
        "csi_set_peer_tier": [vp, i32], "csi_peer_tier": [vp, C.POINTER(i32)],
        "csi_set_fusion": [vp, i32], "csi_free_drift_set": [vp, i32],
        "csi_set_tile_skipping": [vp, i32], "csi_tile_activity": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
        "csi_set_row_constant": [vp, i32, dbl], "csi_row_constant_rows": [vp, C.POINTER(i32)],
        "csi_coriolis_rows_set": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), i32],
        "csi_velocity_bc_set": [vp, i32, i32, i32, dbl],
        "csi_coriolis_points_set": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), i64],
        "csi_immersed_flux_bc_set": [vp, i32, dbl, dbl, dbl, dbl],
        "csi_plan_exchange": [i32] * 14 + [C.POINTER(i32)],
        "csi_profile_substeps": [vp, dbl, i32, C.POINTER(dbl)],
        "csi_last_path": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
        "csi_last_advection": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
        "csi_last_subcycle_ms": [vp, C.POINTER(dbl)], "csi_launches_per_substep": [vp, C.POINTER(i32)],
        "csi_last_launches": [vp, C.POINTER(i32), C.POINTER(i32)],
        "csi_validate_all": [vp], "csi_debug_peer_abort": [vp], "csi_set_weno_weight_dtype": [vp, i32], "csi_weno_weight_dtype": [vp, C.POINTER(i32)], "csi_subcycle_stats_begin": [vp],
        "csi_subcycle_stats_end": [vp, C.POINTER(dbl), C.POINTER(i32), C.POINTER(i32)],
        "csi_rheology_set": [vp, i32, dbl], "csi_momentum_solver_set": [vp, i32], "csi_compute_momentum_tendencies": [vp, dbl],
        "csi_heat_fluxes_set": [vp, i32, C.POINTER(HeatFluxTerm), i32], "csi_surface_solve_set": [vp, C.POINTER(SurfaceSolve)],
        "csi_dynamics_set": [vp, i32],
        "csi_time_series_plan": [C.POINTER(dbl), i32, i32, dbl, dbl, C.POINTER(i32), C.POINTER(i32), C.POINTER(dbl)],
        "csi_time_series_set": [vp, i32, C.POINTER(TimeSeries)], "csi_time_series_update": [vp, dbl],
        "csi_time_series_status": [vp, i32, C.POINTER(i32), C.POINTER(i64)],
        "csi_regrid_plan_axis": [C.POINTER(dbl), i32, i32, dbl, dbl, C.POINTER(i32), C.POINTER(i32), C.POINTER(dbl)],
        "csi_regrid_map_create": [vp, C.POINTER(RegridMap), C.POINTER(i32)], "csi_regrid_map_destroy": [vp, i32],
        "csi_time_series_set_regridded": [vp, i32, C.POINTER(TimeSeries), i32, C.POINTER(TimeSeries), i32],
        "csi_regrid_stats": [vp, C.POINTER(i64), C.POINTER(i32)],
        "csi_diagnostics_compute": [vp, i32, dbl, C.POINTER(Diagnostics)],
        "csi_output_plan_layout": [C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(i64), C.POINTER(i64)],
        "csi_output_create": [vp, C.POINTER(OutputField), i32, i32, C.POINTER(i32)],
        "csi_output_layout": [vp, i32, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)],
        "csi_output_record_bytes": [vp, i32, C.POINTER(i64)],
        "csi_output_accumulate": [vp, i32, dbl], "csi_output_snapshot": [vp, i32, C.POINTER(i32)],
        "csi_output_test": [vp, i32, i32, C.POINTER(i32)], "csi_output_wait": [vp, i32, i32, C.POINTER(vp)],
        "csi_output_release": [vp, i32, i32], "csi_output_destroy": [vp, i32],
        "csi_derived_compute": [vp, i32], "csi_budget_compute": [vp, i32, C.POINTER(Budget)],
        "csi_derived_stats": [vp, C.POINTER(i64), C.POINTER(i64)],
        "csi_momentum_terms_compute": [vp, i32], "csi_momentum_budget_compute": [vp, i32, C.POINTER(MomentumBudget)],
        "csi_momentum_terms_stats": [vp, C.POINTER(i64), C.POINTER(i64)],
        "csi_mixed_layer_set": [vp, C.POINTER(MixedLayerParams)], "csi_mixed_layer_step": [vp, dbl, i32],
        "csi_mixed_layer_stats": [vp, C.POINTER(i64)],
        "csi_shortwave_set": [vp, C.POINTER(Shortwave)],
        "csi_last_thermo": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
        "csi_enthalpy_plan": [i32, i32, C.POINTER(i32), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)],
        "csi_enthalpy_create": [vp, C.POINTER(EnthalpyParams), C.POINTER(vp)], "csi_enthalpy_destroy": [vp],
        "csi_enthalpy_bind": [vp, i32, vp],
        "csi_enthalpy_boundary_set": [vp, i32, i32, dbl, vp, C.POINTER(TimeSeries)],
        "csi_enthalpy_set": [vp, i32, dbl], "csi_enthalpy_update_state": [vp, dbl],
        "csi_enthalpy_time_step": [vp, dbl, i32, dbl, C.POINTER(dbl)],
        "csi_enthalpy_last_launch": [vp, C.POINTER(EnthalpyLaunch)], "csi_enthalpy_ice_thickness": [vp, dbl, vp],
        "csi_drifters_locate": [i32, i32, dbl, dbl, C.POINTER(i32), C.POINTER(dbl)],
        "csi_drifters_advance": [vp, C.POINTER(Drifters), dbl, i32], "csi_drifters_sample": [vp, C.POINTER(Drifters), i32, vp, i64],
        "csi_drifters_stats": [vp, C.POINTER(i64)],
        "csi_regions_layout": [i32, i32, i32, C.POINTER(i64), C.POINTER(i64)],
        "csi_regions_compute": [vp, C.POINTER(Regions), dbl, C.POINTER(RegionRecord), C.POINTER(i64)],
        "csi_regions_stats": [vp, C.POINTER(i64)],
        "csi_tracers_set": [vp, C.POINTER(Tracers)], "csi_tracers_tendencies": [vp, i32, dbl, i32], "csi_tracers_update": [vp, dbl],
        "csi_tracers_stats": [vp, C.POINTER(i64), C.POINTER(i64)],
        "csi_tracers_last": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
    }
    for name, args in sig.items():
        fn = getattr(L, name, None)
        if fn is None and "CSI_HIP_LIBRARY" in os.environ:
            continue                      # an older build in an A/B run (scripts/ab_libs.sh): entry points added since are absent
        if fn is None:
            raise AttributeError(f"libcsi_hip.so does not export {name}: rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
        fn.restype = i32
        fn.argtypes = args
    L.csi_local_group_destroy.restype = None
    L.csi_local_group_destroy.argtypes = [vp]
    _lib = L
    return L


def plan_ranges(Nx, Ny, Hx, Hy, topo_x, topo_y, valid_width=2):
    """(stress, u-first, v-first, second-velocity) index ranges of the launch loop (pure host function)."""
    out = (C.c_int32 * 16)()
    rc = load().csi_plan_ranges(Nx, Ny, Hx, Hy, topo_x, topo_y, valid_width, out)
    if rc != OK:
        raise CsiError(rc, "csi_plan_ranges")
    v = list(out)
    return tuple(tuple(v[4 * k:4 * k + 4]) for k in range(4))


def plan_pair(Nx, Ny, Hx, Hy, topo_x, topo_y, k=1, m=0):
    """csi_plan_pair as a dict (None when the two-sub-steps-per-launch kernel does not apply)."""
    L = load()
    out = (C.c_int32 * 32)()
    rc = L.csi_plan_pair(Nx, Ny, Hx, Hy, topo_x, topo_y, k, m, out)
    if rc != OK:
        raise CsiError(rc, "csi_plan_pair")
    if not out[0]:
        return None
    r = lambda q: tuple(out[4 + 4 * q: 8 + 4 * q])
    return dict(nstrips=out[1], nchunks=out[2], rows=out[3], first_compute=r(0), second_compute=r(1), store_sigma=r(2),
                store_first_u=r(3), store_first_v=r(4), store_second=r(5), walls=bool(out[28]))


def time_series_plan(times, indexing, period, t):
    """csi_time_series_plan: (n1, n2, weight) of a time series at time t (pure host function; CsiError on invalid input)."""
    a = np.ascontiguousarray(times, dtype=np.float64)
    n1, n2, frac = C.c_int32(), C.c_int32(), C.c_double()
    rc = load().csi_time_series_plan(a.ctypes.data_as(C.POINTER(C.c_double)), a.size, int(indexing), float(period), float(t),
                                     C.byref(n1), C.byref(n2), C.byref(frac))
    if rc != OK:
        raise CsiError(rc, "csi_time_series_plan: invalid input")
    return n1.value, n2.value, frac.value


def enthalpy_plan(Nz, forced_path=0):
    """csi_enthalpy_plan as a dict: the form of the enthalpy-method column model's step kernel for columns of Nz levels (pure host
    function; CsiError on invalid input and for a forced on-chip form that does not fit)."""
    form, lds, waves, cap = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32()
    rc = load().csi_enthalpy_plan(int(Nz), int(forced_path), C.byref(form), C.byref(lds), C.byref(waves), C.byref(cap))
    if rc != OK:
        raise CsiError(rc, "csi_enthalpy_plan: invalid input, or the forced on-chip form does not fit")
    return dict(form=form.value, lds_bytes=lds.value, waves_per_cu=waves.value, max_substeps=cap.value)


def drifters_locate(Nx, Ny, xi, eta):
    """csi_drifters_locate as a dict: the stencils and weights of one index-space position (pure host function; any xi, eta is accepted,
    CsiError for extents < 1)."""
    idx, w = (C.c_int32 * 6)(), (C.c_double * 4)()
    rc = load().csi_drifters_locate(int(Nx), int(Ny), float(xi), float(eta), idx, w)
    if rc != OK:
        raise CsiError(rc, "csi_drifters_locate: Nx >= 1 and Ny >= 1 are needed")
    return dict(ia=idx[0], ja=idx[1], ib=idx[2], jb=idx[3], ic=idx[4], jc=idx[5], sx=w[0], sy=w[1], rx=w[2], ry=w[3])


def regions_layout(Nx, Ny, n_regions):
    """csi_regions_layout: (records, bytes) of the partial buffer of csi_regions_compute (pure host function; CsiError for extents < 1
    and for n_regions outside 1 .. REGIONS_MAX)."""
    rec, nb = C.c_int64(), C.c_int64()
    rc = load().csi_regions_layout(int(Nx), int(Ny), int(n_regions), C.byref(rec), C.byref(nb))
    if rc != OK:
        raise CsiError(rc, "csi_regions_layout: Nx >= 1, Ny >= 1 and 1 <= n_regions <= 64 are needed")
    return rec.value, nb.value


def regrid_plan_axis(nodes, periodic, period, x):
    """csi_regrid_plan_axis: (i0, i1, weight of i1) of coordinate x on a source axis (pure host function; CsiError on invalid input)."""
    a = np.ascontiguousarray(nodes, dtype=np.float64)
    i0, i1, w = C.c_int32(), C.c_int32(), C.c_double()
    rc = load().csi_regrid_plan_axis(a.ctypes.data_as(C.POINTER(C.c_double)), a.size, int(bool(periodic)), float(period or 0.0), float(x),
                                     C.byref(i0), C.byref(i1), C.byref(w))
    if rc != OK:
        raise CsiError(rc, "csi_regrid_plan_axis: invalid input")
    return i0.value, i1.value, w.value


def output_plan_layout(shapes, dtypes):
    """csi_output_plan_layout: (byte offsets, record bytes) of a record whose field k is a dense (ny, nx) = shapes[k] array of
    dtypes[k] (OUT_F64 / OUT_F32).  Pure host function; CsiError on invalid input."""
    n = len(shapes)
    nx = (C.c_int32 * max(n, 1))(*[int(s[1]) for s in shapes])
    ny = (C.c_int32 * max(n, 1))(*[int(s[0]) for s in shapes])
    dt = (C.c_int32 * max(n, 1))(*[int(d) for d in dtypes])
    off, total = (C.c_int64 * max(n, 1))(), C.c_int64()
    rc = load().csi_output_plan_layout(nx, ny, dt, n, off, C.byref(total))
    if rc != OK:
        raise CsiError(rc, "csi_output_plan_layout: invalid input")
    return list(off)[:n], total.value


def plan_peer_chunks(Nx, Ny, Hx, Hy, peer_south=True, peer_north=True):
    """csi_plan_peer_chunks as a dict: the chunk layout of a pair launch on the peer transport (None: the pair kernel does not apply)."""
    out = (C.c_int32 * 8)()
    rows = (C.c_int32 * 4096)()
    rc = load().csi_plan_peer_chunks(Nx, Ny, Hx, Hy, int(peer_south), int(peer_north), 256, out, rows, 2048)
    if rc != OK:
        raise CsiError(rc, "csi_plan_peer_chunks")
    if not out[0]:
        return None
    n = out[2]
    return dict(nstrips=out[1], nchunks=n, rows=out[3], elo=out[4], ehi=out[5], nS=out[6], nN=out[7],
                chunks=[(rows[2 * q], rows[2 * q + 1]) for q in range(min(n, 2048))])


def plan_exchange(Nx, Ny, Hx, Hy, topo_x, topo_y, rx, ry, Rx, Ry, periodic_x, periodic_y, width, halo):
    """Eight (peer, i0, j0, ni, nj) entries of the library's exchange plan (pure host function)."""
    out = (C.c_int32 * 40)()
    rc = load().csi_plan_exchange(Nx, Ny, Hx, Hy, topo_x, topo_y, rx, ry, Rx, Ry, int(periodic_x), int(periodic_y), width, int(halo), out)
    if rc != OK:
        raise CsiError(rc, "csi_plan_exchange")
    v = list(out)
    return [tuple(v[5 * k:5 * k + 5]) for k in range(8)]


class LocalGroup:
    """csi_local_group: the tiles of one process (one thread each) exchange halos through device copies instead of RCCL
    (include/csi.h).  Pass it to TileGrid(..., local_group=...); keep it alive as long as its models."""

    def __init__(self, world_size):
        self.L = load()
        self.h = C.c_void_p()
        rc = self.L.csi_local_group_create(int(world_size), C.byref(self.h))
        if rc != OK:
            raise CsiError(rc, "csi_local_group_create")
        self.world_size = int(world_size)

    def close(self):
        if self.h:
            self.L.csi_local_group_destroy(self.h)
            self.h = C.c_void_p()


class Context:
    """One csi_context (one GPU).  Thin: every method is one ABI call that raises on failure."""

    def __init__(self, device_id=0, stream=None):
        self.L = load()
        self.h = C.c_void_p()
        rc = self.L.csi_context_create(device_id, C.c_void_p(stream) if stream else None, C.byref(self.h))
        if rc != OK:
            raise CsiError(rc, self.L.csi_last_error(None).decode())

    def _ck(self, rc):
        if rc != OK:
            raise CsiError(rc, self.L.csi_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.L.csi_context_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def call(self, name, *args):
        self._ck(getattr(self.L, name)(self.h, *args))

    def last_subcycle_ms(self):
        v = C.c_double()
        self.call("csi_last_subcycle_ms", C.byref(v))
        return v.value

    def subcycle_stats_begin(self):
        self.call("csi_subcycle_stats_begin")

    def subcycle_stats_end(self):
        """(total device ms, sub-cycles, kernel launches) of every sub-cycle since subcycle_stats_begin (synchronises)."""
        t, n, l = C.c_double(), C.c_int32(), C.c_int32()
        self.call("csi_subcycle_stats_end", C.byref(t), C.byref(n), C.byref(l))
        return t.value, n.value, l.value

    def validate_all(self):
        """csi_sync + the halo transport's status over ALL ranks (collective)."""
        self.call("csi_validate_all")

    def profile_substeps(self, dt, substeps=16):
        out = (C.c_double * 4)()
        self.call("csi_profile_substeps", float(dt), int(substeps), out)
        return dict(stress=out[0], ustep=out[1], vstep=out[2], exchange=out[3])

    def last_path(self):
        f, k, n = C.c_int32(), C.c_int32(), C.c_int32()
        self.call("csi_last_path", C.byref(f), C.byref(k), C.byref(n))
        return dict(fused=bool(f.value), level=f.value, exchange_interval=k.value, exchanges=n.value)

    def last_advection(self):
        """csi_last_advection: the layout of the last advection launch (all zero before the first one)."""
        nt, tx, ty, st = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self.call("csi_last_advection", C.byref(nt), C.byref(tx), C.byref(ty), C.byref(st))
        return dict(tracers_per_thread=nt.value, tile_x=tx.value, tile_y=ty.value, stage_fused=st.value)

    def last_thermo(self):
        """csi_last_thermo: the kernel of the last thermodynamic launch -- step 0 none yet, 1 k_slab, 2 k_layered, 3 k_slab_flux,
        4 k_layered_flux; shortwave 0 / 1 / 2 (no term / the flux a number / per cell); index within the family (-1: numeric kernels)."""
        st, sw, b = C.c_int32(), C.c_int32(), C.c_int32()
        self.call("csi_last_thermo", C.byref(st), C.byref(sw), C.byref(b))
        return dict(step=st.value, shortwave=sw.value, index=b.value)

    def comm_count(self):
        """ranks of the RCCL communicator (ncclCommCount); 0 without one"""
        v = C.c_int32()
        self.call("csi_comm_count", C.byref(v))
        return v.value

    def halo_transport(self):
        """"peer" / "rccl": what the last sub-cycle moved its halos with (csi_halo_transport)"""
        v = C.c_int32()
        self.call("csi_halo_transport", C.byref(v))
        return "peer" if v.value == 1 else "rccl"

    def peer_tier(self):
        """protocol tier of the peer halo transport (csi_peer_tier): 0 write-through + flags, 1 + acquire fence, 2 + release fence"""
        v = C.c_int32()
        self.call("csi_peer_tier", C.byref(v))
        return v.value

    def last_launches(self):
        """(kernel launches, sub-steps) of the last fused sub-cycle."""
        a, b = C.c_int32(), C.c_int32()
        self.call("csi_last_launches", C.byref(a), C.byref(b))
        return a.value, b.value

    def launches_per_substep(self):
        v = C.c_int32()
        self.call("csi_launches_per_substep", C.byref(v))
        return v.value

    def diagnostics_compute(self, what, extent_threshold):
        """csi_diagnostics_compute: the filled csi_diagnostics (two launches and one small copy; waits for the context's stream;
        collective on a tiled context)."""
        d = Diagnostics()
        self.call("csi_diagnostics_compute", int(what), float(extent_threshold), C.byref(d))
        return d

    def time_series_update(self, time):
        """csi_time_series_update: every series-driven slot interpolated at `time`, one launch (none without series)."""
        self.call("csi_time_series_update", float(time))

    def time_series_status(self, slot, window):
        """(slices the ring slots of a HOST series hold, -1: none; slice uploads since csi_time_series_set)."""
        res, up = (C.c_int32 * max(int(window), 1))(*([-1] * max(int(window), 1))), C.c_int64()
        self.call("csi_time_series_status", slot_id(slot), res, C.byref(up))
        return list(res)[:int(window)], up.value

    # ---- series on a source grid of their own (include/csi.h, csi_regrid_map_create) -----------------------------------------------
    def regrid_map_create(self, location, i0, i1, j0, j1, wx, wy, source_shape, cos=None, sin=None):
        """csi_regrid_map_create: the map's id.  location: REGRID_*; i0 .. wy (and cos, sin): (ny, nx) arrays; source_shape: (src_ny, src_nx).
        The library copies everything."""
        ny, nx = np.shape(wx)
        idx = [np.ascontiguousarray(a, dtype=np.int32) for a in (i0, i1, j0, j1)]
        w = [np.ascontiguousarray(a, dtype=np.float64) for a in (wx, wy)]
        rot = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (cos, sin)]
        if any(a.shape != (ny, nx) for a in idx + w + [a for a in rot if a is not None]):
            raise ValueError("regrid map: every array has the (ny, nx) shape of the target interior")
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        d = RegridMap(int(location), nx, ny, int(source_shape[1]), int(source_shape[0]), 0, *[a.ctypes.data_as(ip) for a in idx],
                      *[a.ctypes.data_as(dp) for a in w], *[None if a is None else a.ctypes.data_as(dp) for a in rot])
        out = C.c_int32(-1)
        self.call("csi_regrid_map_create", C.byref(d), C.byref(out))
        return out.value

    def regrid_stats(self):
        """(launches of the regridding kernel so far, maps alive) of this context."""
        n, m = C.c_int64(), C.c_int32()
        self.call("csi_regrid_stats", C.byref(n), C.byref(m))
        return n.value, m.value

    # ---- derived fields and energy budget integrals (include/csi.h) ---------------------------------------------------------------
    def derived_compute(self, mask):
        """csi_derived_compute: every requested derived field in ONE launch on the context's stream (nothing is waited for)."""
        self.call("csi_derived_compute", int(mask))

    def budget_compute(self, what):
        """csi_budget_compute: the filled csi_budget (two launches and one small copy; waits for the context's stream; collective on a
        tiled context)."""
        b = Budget()
        self.call("csi_budget_compute", int(what), C.byref(b))
        return b

    def derived_stats(self):
        """(launches of the derived-field kernel, budget calls) made on this context so far."""
        a, b = C.c_int64(), C.c_int64()
        self.call("csi_derived_stats", C.byref(a), C.byref(b))
        return a.value, b.value

    # ---- Lagrangian ice drifters (include/csi.h, csi_drifters_*) --------------------------------------------------------------------
    def drifters_advance(self, d, dt, substeps=1):
        """csi_drifters_advance: `substeps` midpoint sub-steps of dt / substeps in ONE launch on the context's stream (nothing is waited for)."""
        self.call("csi_drifters_advance", C.byref(d), float(dt), int(substeps))

    def drifters_sample(self, d, columns, dev_out, ld):
        """csi_drifters_sample: the columns of the mask at dev_out[k * ld + q], ONE launch (nothing is waited for)."""
        self.call("csi_drifters_sample", C.byref(d), int(columns), C.c_void_p(dev_out) if dev_out else None, int(ld))

    def drifters_stats(self):
        """Launches of the two drifter kernels made on this context so far."""
        n = C.c_int64()
        self.call("csi_drifters_stats", C.byref(n))
        return n.value

    # ---- per-region ice integrals and extrema (include/csi.h, csi_regions_*) ---------------------------------------------------------
    def regions_compute(self, ids_ptr, ld, n_regions, extent_threshold, reserved=0):
        """csi_regions_compute: (the n_regions filled csi_region_record, unassigned_cells); two launches and one small copy, waits for
        the context's stream; collective on a tiled context.  ids_ptr: the device address of the map's parent."""
        r = Regions(C.c_void_p(ids_ptr) if ids_ptr else None, int(ld), int(n_regions), int(reserved))
        out = (RegionRecord * max(1, min(int(n_regions), REGIONS_MAX)))()
        stray = C.c_int64(-1)
        self.call("csi_regions_compute", C.byref(r), float(extent_threshold), out, C.byref(stray))
        return out, stray.value

    def regions_stats(self):
        """Launches made by csi_regions_compute on this context so far (two per call)."""
        n = C.c_int64()
        self.call("csi_regions_stats", C.byref(n))
        return n.value

    # ---- advected ice tracers (include/csi.h, csi_tracers_*) --------------------------------------------------------------------------
    def tracers_set(self, t):
        """csi_tracers_set: the library copies the Tracers struct (None removes the tracers)."""
        self.call("csi_tracers_set", None if t is None else C.byref(t))

    def tracers_tendencies(self, scheme, dt, from_cache=False):
        """csi_tracers_tendencies: the first half of a stage for every tracer, one launch (nothing is waited for)."""
        self.call("csi_tracers_tendencies", int(scheme), float(dt), int(bool(from_cache)))

    def tracers_update(self, dt):
        """csi_tracers_update: the second half of a stage for every tracer, one launch (nothing is waited for)."""
        self.call("csi_tracers_update", float(dt))

    def tracers_stats(self):
        """(launches of the tracer stencil kernel, launches of the point-wise tracer kernels) made on this context so far."""
        a, b = C.c_int64(), C.c_int64()
        self.call("csi_tracers_stats", C.byref(a), C.byref(b))
        return a.value, b.value

    def tracers_last(self):
        """csi_tracers_last: the layout of the last tracer stencil launch (all zero before the first one)."""
        v = [C.c_int32() for _ in range(4)]
        self.call("csi_tracers_last", *[C.byref(x) for x in v])
        return dict(tracers_per_thread=v[0].value, tile_x=v[1].value, tile_y=v[2].value, groups=v[3].value)

    # ---- momentum balance terms, interface stresses and their power (include/csi.h) ------------------------------------------------
    def momentum_terms_compute(self, mask):
        """csi_momentum_terms_compute: every requested term field in ONE launch on the context's stream (nothing is waited for)."""
        self.call("csi_momentum_terms_compute", int(mask))

    def momentum_budget_compute(self, what):
        """csi_momentum_budget_compute: the filled csi_momentum_budget (two launches and one small copy; waits for the context's stream;
        collective on a tiled context)."""
        b = MomentumBudget()
        self.call("csi_momentum_budget_compute", int(what), C.byref(b))
        return b

    def momentum_terms_stats(self):
        """(launches of the term kernel, power calls) made on this context so far."""
        a, b = C.c_int64(), C.c_int64()
        self.call("csi_momentum_terms_stats", C.byref(a), C.byref(b))
        return a.value, b.value

    # ---- the slab-ocean mixed layer (include/csi.h, csi_mixed_layer_set) -----------------------------------------------------------
    def mixed_layer_step(self, dt, from_cache=False):
        """csi_mixed_layer_step: one launch that writes To' and the bottom heat-flux array (nothing is waited for)."""
        self.call("csi_mixed_layer_step", float(dt), int(bool(from_cache)))

    def mixed_layer_stats(self):
        """Launches of the mixed-layer kernel made on this context so far."""
        n = C.c_int64()
        self.call("csi_mixed_layer_stats", C.byref(n))
        return n.value

    # ---- device-side output (include/csi.h, csi_output_*) -------------------------------------------------------------------------
    def output_create(self, fields, slots):
        """csi_output_create: fields = [(slot name, OUT_F64 | OUT_F32, averaged, masked, fill_value), ...]; returns the handle."""
        arr = (OutputField * max(len(fields), 1))(*[OutputField(slot_id(n), int(d), int(a), int(m), float(v)) for n, d, a, m, v in fields])
        h = C.c_int32()
        self.call("csi_output_create", arr, len(fields), int(slots), C.byref(h))
        return h.value

    def output_layout(self, handle, k):
        """(byte offset, ny, nx) of field k in a record of the set"""
        off, nx, ny = C.c_int64(), C.c_int32(), C.c_int32()
        self.call("csi_output_layout", int(handle), int(k), C.byref(off), C.byref(nx), C.byref(ny))
        return off.value, ny.value, nx.value

    def output_record_bytes(self, handle):
        v = C.c_int64()
        self.call("csi_output_record_bytes", int(handle), C.byref(v))
        return v.value

    def output_accumulate(self, handle, w):
        self.call("csi_output_accumulate", int(handle), float(w))

    def output_snapshot(self, handle):
        """csi_output_snapshot: queues the pack launch and the copy, returns the slot without waiting for the device."""
        v = C.c_int32()
        self.call("csi_output_snapshot", int(handle), C.byref(v))
        return v.value

    def output_test(self, handle, slot):
        v = C.c_int32()
        self.call("csi_output_test", int(handle), int(slot), C.byref(v))
        return bool(v.value)

    def output_wait(self, handle, slot):
        """csi_output_wait: waits for that slot's copy only; the record as a uint8 view of the page-locked slot (valid until
        output_release)."""
        p = C.c_void_p()
        self.call("csi_output_wait", int(handle), int(slot), C.byref(p))
        n = self.output_record_bytes(handle)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,))

    def output_release(self, handle, slot):
        self.call("csi_output_release", int(handle), int(slot))

    def output_destroy(self, handle):
        self.call("csi_output_destroy", int(handle))
