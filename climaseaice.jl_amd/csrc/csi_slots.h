// csi_slots.h -- every field slot of csi_field_bind stated once: id, the name messages print, (x, y) location, roles.  Depends on
// include/csi.h alone and compiles as plain C++ (tests/slots_host.cpp prints the table, tests/test_slot_table.py compares it with
// _lib.SLOTS, the header's enumerators and the Julia stub).  A new slot: its enumerator in include/csi.h and its row here.
#pragma once
#include "../../include/csi.h"
#include <vector>
namespace csi {
#ifndef CSI_LOC_DEFINED      // (csi_dev.h states the same two for the kernels)
#define CSI_LOC_DEFINED
enum : int { LOC_C = 0, LOC_F = 1 };
#endif
}  // namespace csi
namespace csi_host {
using csi::LOC_C; using csi::LOC_F;
enum : unsigned {
    SLOT_HALO = 1,       // csi_fill_halo_local and csi_halo_exchange take it
    SLOT_PEER = 2,       // the neighbouring tiles map its array: re-binding it while the peer transport is set up tears the transport down
    SLOT_FORCING = 4,    // update_external_stress fills (and, on tiles, exchanges) its halos before a momentum step, in table order
    SLOT_SERIES = 8      // a time series may drive it (csi_time_series_set, csi_time_series_set_regridded)
};
struct Slot { int id; const char* name; int lx, ly; unsigned roles; };
constexpr int kSlotCount = CSI_F_COUNT_SHORTWAVE;      // the last count of include/csi.h: named here and nowhere else in csrc/
namespace slot_rows {      // (shorthand for the rows only)
constexpr int C = LOC_C, F = LOC_F;
constexpr unsigned H = SLOT_HALO, P = SLOT_PEER, S = SLOT_SERIES, HFS = SLOT_HALO | SLOT_FORCING | SLOT_SERIES;
constexpr Slot kSlots[] = {
    {CSI_F_U, "u", F, C, H | P}, {CSI_F_V, "v", C, F, H | P}, {CSI_F_H, "h", C, C, H}, {CSI_F_A, "aice", C, C, H},
    {CSI_F_S11, "sigma11", C, C, H | P}, {CSI_F_S22, "sigma22", C, C, H | P}, {CSI_F_S12, "sigma12", F, F, H | P}, {CSI_F_UN, "un", F, C, H},
    {CSI_F_VN, "vn", C, F, H}, {CSI_F_P, "P", C, C, H}, {CSI_F_ALPHA, "alpha", C, C, H | P}, {CSI_F_DELTA, "Delta", C, C, H | P},
    {CSI_F_ZETA_F, "zeta_f", F, F, H | P}, {CSI_F_ZETA_C, "zeta_c", C, C, H | P}, {CSI_F_GH, "Gh", C, C, H}, {CSI_F_GA, "Gaice", C, C, H},
    {CSI_F_HM, "h-", C, C, H}, {CSI_F_AM, "aice-", C, C, H}, {CSI_F_UM, "u-", F, C, H}, {CSI_F_VM, "v-", C, F, H}, {CSI_F_TOP_U, "top_u", F, C, HFS},
    {CSI_F_TOP_V, "top_v", C, F, HFS}, {CSI_F_BOT_U, "bottom_u", F, C, HFS}, {CSI_F_BOT_V, "bottom_v", C, F, HFS},
    {CSI_F_MASS_FLUX, "mass_flux", C, C, H}, {CSI_F_HS, "hs", C, C, H}, {CSI_F_GHS, "Ghs", C, C, H}, {CSI_F_HSM, "hs-", C, C, H},
    {CSI_F_MASS_FLUX_SNOW, "mass_flux_snow", C, C, H}, {CSI_F_SNOWFALL_INTERCEPTED, "intercepted_snowfall", C, C, H}, {CSI_F_TU, "Tu", C, C, H},
    {CSI_F_TUS, "Tu_snow", C, C, H}, {CSI_F_FORCING_U, "forcing_u", F, C, HFS}, {CSI_F_FORCING_V, "forcing_v", C, F, HFS}, {CSI_F_GU, "Gu", F, C, H},
    {CSI_F_GV, "Gv", C, F, H}, {CSI_F_TOP_HEAT_FLUX, "top_heat_flux", C, C, S}, {CSI_F_BOTTOM_HEAT_FLUX, "bottom_heat_flux", C, C, S},
    {CSI_F_SNOWFALL, "snowfall", C, C, S}, {CSI_F_FREE_DRIFT_U, "free_drift_u", F, C, HFS}, {CSI_F_FREE_DRIFT_V, "free_drift_v", C, F, HFS},
    {CSI_F_D_DIVERGENCE, "divergence", C, C, 0}, {CSI_F_D_SHEAR, "shear", C, C, 0}, {CSI_F_D_DEFORMATION, "deformation", C, C, 0},
    {CSI_F_D_SPEED, "speed", C, C, 0}, {CSI_F_D_SIGMA_I, "sigma_I", C, C, 0}, {CSI_F_D_SIGMA_II, "sigma_II", C, C, 0},
    {CSI_F_D_STRESS_POWER, "stress_power", C, C, 0}, {CSI_F_M_CORIOLIS_X, "coriolis_x", F, C, 0}, {CSI_F_M_CORIOLIS_Y, "coriolis_y", C, F, 0},
    {CSI_F_M_TOP_X, "top_x", F, C, 0}, {CSI_F_M_TOP_Y, "top_y", C, F, 0}, {CSI_F_M_BOTTOM_X, "bottom_x", F, C, 0},
    {CSI_F_M_BOTTOM_Y, "bottom_y", C, F, 0}, {CSI_F_M_INTERNAL_X, "internal_x", F, C, 0}, {CSI_F_M_INTERNAL_Y, "internal_y", C, F, 0},
    {CSI_F_M_FORCING_X, "forcing_x", F, C, 0}, {CSI_F_M_FORCING_Y, "forcing_y", C, F, 0}, {CSI_F_FLUX_COEFFICIENT, "flux_coefficient", C, C, S},
    {CSI_F_FLUX_REFERENCE_TEMPERATURE, "flux_reference_temperature", C, C, S}, {CSI_F_BOTTOM_SALINITY, "bottom_salinity", C, C, S},
    {CSI_F_TOP_HEAT_FLUX_USED, "top_heat_flux_used", C, C, 0}, {CSI_F_BOTTOM_HEAT_FLUX_USED, "bottom_heat_flux_used", C, C, 0},
    {CSI_F_ML_TEMPERATURE, "ocean_temperature", C, C, 0}, {CSI_F_ML_TEMPERATURE_M, "ocean_temperature-", C, C, 0},
    {CSI_F_ML_SURFACE_HEAT_FLUX, "ocean_surface_heat_flux", C, C, S}, {CSI_F_ML_COEFFICIENT, "ocean_coefficient", C, C, S},
    {CSI_F_ML_REFERENCE_TEMPERATURE, "ocean_reference_temperature", C, C, S}, {CSI_F_ML_DEEP_HEAT_FLUX, "ocean_deep_heat_flux", C, C, S},
    {CSI_F_ML_SURFACE_FLUX_USED, "ocean_surface_flux_used", C, C, 0}, {CSI_F_SHORTWAVE, "shortwave", C, C, S},
    {CSI_F_ALBEDO_USED, "albedo_used", C, C, 0}};
}  // namespace slot_rows
using slot_rows::kSlots;

constexpr bool slots_in_id_order(int k = 0) { return k == kSlotCount || (kSlots[k].id == k && slots_in_id_order(k + 1)); }
static_assert(sizeof kSlots / sizeof kSlots[0] == kSlotCount, "kSlots: one row per enumerator of include/csi.h, up to its last count");
static_assert(slots_in_id_order(), "kSlots: row k describes slot id k");

constexpr bool slot_known(int fid) { return fid >= 0 && fid < kSlotCount; }
constexpr const char* slot_name(int fid) { return kSlots[fid].name; }
constexpr int slot_loc(int fid, int axis) { return axis == 0 ? kSlots[fid].lx : kSlots[fid].ly; }
constexpr bool slot_has(int fid, unsigned role) { return slot_known(fid) && (kSlots[fid].roles & role) != 0; }      // (false for an unknown id)
inline std::vector<int> slots_with(unsigned role) {      // the ids of a role in table order
    std::vector<int> ids;
    for (int k = 0; k < kSlotCount; ++k) if (slot_has(k, role)) ids.push_back(k);
    return ids;
}
}  // namespace csi_host
