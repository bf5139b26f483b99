/* thermo_linear_layout.c -- the heat-flux structs and the enums added with the LINEAR top-flux term, the per-cell bottom salinity and
 * the used-flux outputs, as a C compiler sees include/csi.h, printed as JSON for tests/test_thermo_linear_ref.py. */
#include <stddef.h>
#include <stdio.h>

#include "csi.h"

#define VAL(x) printf("%s\"%s\": %d", first ? "" : ", ", #x, (int)(x)), first = 0
#define OFF(T, f) printf("%s\"%s.%s\": %d", first ? "" : ", ", #T, #f, (int)offsetof(T, f)), first = 0

int main(void) {
    int first = 1;
    printf("{");
    VAL(CSI_FLUX_CONSTANT); VAL(CSI_FLUX_ARRAY); VAL(CSI_FLUX_RADIATIVE_EMISSION); VAL(CSI_FLUX_LINEAR);
    VAL(CSI_WEIGHT_NONE); VAL(CSI_WEIGHT_CONCENTRATION); VAL(CSI_WEIGHT_ICE_PRESENT);
    VAL(CSI_LINEAR_WEIGHT_MASK); VAL(CSI_LINEAR_COEFFICIENT_ARRAY); VAL(CSI_LINEAR_REFERENCE_ARRAY); VAL(CSI_SOLVE_BOTTOM_SALINITY_ARRAY);
    VAL(CSI_F_COUNT); VAL(CSI_F_COUNT_ALL); VAL(CSI_F_COUNT_TOTAL); VAL(CSI_F_COUNT_DERIVED); VAL(CSI_F_COUNT_BINDABLE);
    VAL(CSI_F_FLUX_COEFFICIENT); VAL(CSI_F_FLUX_REFERENCE_TEMPERATURE); VAL(CSI_F_BOTTOM_SALINITY); VAL(CSI_F_TOP_HEAT_FLUX_USED);
    VAL(CSI_F_BOTTOM_HEAT_FLUX_USED); VAL(CSI_F_COUNT_THERMO); VAL(CSI_VERSION);
    printf(", \"sizeof_term\": %d, \"sizeof_solve\": %d", (int)sizeof(csi_heat_flux_term), (int)sizeof(csi_surface_solve));
    OFF(csi_heat_flux_term, kind); OFF(csi_heat_flux_term, reserved); OFF(csi_heat_flux_term, value); OFF(csi_heat_flux_term, emissivity);
    OFF(csi_heat_flux_term, stefan_boltzmann_constant); OFF(csi_heat_flux_term, reference_temperature);
    OFF(csi_surface_solve, tol); OFF(csi_surface_solve, maxiters); OFF(csi_surface_solve, prescribed_array);
    OFF(csi_surface_solve, snowfall_array); OFF(csi_surface_solve, reserved);
    printf("}\n");
    return 0;
}
