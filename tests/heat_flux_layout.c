/* heat_flux_layout.c -- sizeof / offsetof of the heat-flux structs of include/csi.h as a C compiler lays them out, printed as JSON
 * for tests/test_heat_fluxes.py (compared with the ctypes mirrors in climaseaice.jl_amd/_lib.py). */
#include <stddef.h>
#include <stdio.h>

#include "csi.h"

#define FIELD(T, f) printf("%s\"%s\": %zu", first ? "" : ", ", #f, offsetof(T, f)), first = 0

int main(void) {
    int first = 1;
    printf("{\"csi_heat_flux_term\": {\"size\": %zu, \"fields\": {", sizeof(csi_heat_flux_term));
    FIELD(csi_heat_flux_term, kind); FIELD(csi_heat_flux_term, reserved); FIELD(csi_heat_flux_term, value);
    FIELD(csi_heat_flux_term, emissivity); FIELD(csi_heat_flux_term, stefan_boltzmann_constant);
    FIELD(csi_heat_flux_term, reference_temperature);
    first = 1;
    printf("}}, \"csi_surface_solve\": {\"size\": %zu, \"fields\": {", sizeof(csi_surface_solve));
    FIELD(csi_surface_solve, tol); FIELD(csi_surface_solve, maxiters); FIELD(csi_surface_solve, prescribed_array);
    FIELD(csi_surface_solve, snowfall_array); FIELD(csi_surface_solve, reserved);
    printf("}}, \"enums\": {\"CSI_FLUX_CONSTANT\": %d, \"CSI_FLUX_ARRAY\": %d, \"CSI_FLUX_RADIATIVE_EMISSION\": %d, \"CSI_HEAT_TOP\": %d, "
           "\"CSI_HEAT_BOTTOM\": %d, \"CSI_MAX_HEAT_FLUX_TERMS\": %d, \"CSI_F_TOP_HEAT_FLUX\": %d, \"CSI_F_BOTTOM_HEAT_FLUX\": %d, "
           "\"CSI_F_SNOWFALL\": %d, \"CSI_F_COUNT\": %d, \"CSI_F_COUNT_ALL\": %d, \"CSI_VERSION\": %d}}\n",
           CSI_FLUX_CONSTANT, CSI_FLUX_ARRAY, CSI_FLUX_RADIATIVE_EMISSION, CSI_HEAT_TOP, CSI_HEAT_BOTTOM, CSI_MAX_HEAT_FLUX_TERMS,
           CSI_F_TOP_HEAT_FLUX, CSI_F_BOTTOM_HEAT_FLUX, CSI_F_SNOWFALL, CSI_F_COUNT, CSI_F_COUNT_ALL, CSI_VERSION);
    return 0;
}
