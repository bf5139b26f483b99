/* thermo_shortwave_layout.c -- csi_shortwave, CSI_FLUX_SHORTWAVE and the slots added with the shortwave term, as a C compiler sees
 * include/csi.h, printed as JSON for tests/test_thermo_shortwave_ref.py. */
#include <stddef.h>
#include <stdio.h>

#include "csi.h"

#define VAL(x) printf("%s\"%s\": %d", first ? "" : ", ", #x, (int)(x)), first = 0
#define OFF(T, f) printf("%s\"%s.%s\": %d", first ? "" : ", ", #T, #f, (int)offsetof(T, f)), first = 0

int main(void) {
    int first = 1;
    printf("{");
    VAL(CSI_FLUX_CONSTANT); VAL(CSI_FLUX_ARRAY); VAL(CSI_FLUX_RADIATIVE_EMISSION); VAL(CSI_FLUX_LINEAR); VAL(CSI_FLUX_SHORTWAVE);
    VAL(CSI_WEIGHT_NONE); VAL(CSI_WEIGHT_CONCENTRATION); VAL(CSI_WEIGHT_ICE_PRESENT);
    VAL(CSI_F_COUNT); VAL(CSI_F_COUNT_ALL); VAL(CSI_F_COUNT_TOTAL); VAL(CSI_F_COUNT_DERIVED); VAL(CSI_F_COUNT_BINDABLE);
    VAL(CSI_F_COUNT_THERMO); VAL(CSI_F_COUNT_MIXED_LAYER);
    VAL(CSI_F_SHORTWAVE); VAL(CSI_F_ALBEDO_USED); VAL(CSI_F_COUNT_SHORTWAVE);
    VAL(CSI_VERSION);
    printf(", \"sizeof_shortwave\": %d, \"sizeof_term\": %d", (int)sizeof(csi_shortwave), (int)sizeof(csi_heat_flux_term));
    OFF(csi_shortwave, flux); OFF(csi_shortwave, cold); OFF(csi_shortwave, warm); OFF(csi_shortwave, threshold);
    OFF(csi_shortwave, snow_cold); OFF(csi_shortwave, snow_warm); OFF(csi_shortwave, snow_threshold);
    OFF(csi_shortwave, weighting); OFF(csi_shortwave, per_cell); OFF(csi_shortwave, has_snow_pair); OFF(csi_shortwave, reserved);
    OFF(csi_heat_flux_term, kind); OFF(csi_heat_flux_term, reserved); OFF(csi_heat_flux_term, value); OFF(csi_heat_flux_term, emissivity);
    OFF(csi_heat_flux_term, stefan_boltzmann_constant); OFF(csi_heat_flux_term, reference_temperature);
    printf("}\n");
    return 0;
}
