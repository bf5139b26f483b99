/* mixed_layer_layout.c -- csi_mixed_layer_params, its flags and the slots added with the slab-ocean mixed layer, as a C compiler sees
 * include/csi.h, printed as JSON for tests/test_mixed_layer_ref.py. */
#include <stddef.h>
#include <stdio.h>

#include "csi.h"

#define VAL(x) printf("%s\"%s\": %d", first ? "" : ", ", #x, (int)(x)), first = 0
#define OFF(T, f) printf("%s\"%s.%s\": %d", first ? "" : ", ", #T, #f, (int)offsetof(T, f)), first = 0

int main(void) {
    int first = 1;
    printf("{");
    VAL(CSI_ML_SURFACE_ARRAY); VAL(CSI_ML_BULK_ARRAYS); VAL(CSI_ML_DEEP_ARRAY); VAL(CSI_ML_HAS_SURFACE); VAL(CSI_ML_HAS_BULK);
    VAL(CSI_F_COUNT); VAL(CSI_F_COUNT_ALL); VAL(CSI_F_COUNT_TOTAL); VAL(CSI_F_COUNT_DERIVED); VAL(CSI_F_COUNT_BINDABLE);
    VAL(CSI_F_COUNT_THERMO);
    VAL(CSI_F_ML_TEMPERATURE); VAL(CSI_F_ML_TEMPERATURE_M); VAL(CSI_F_ML_SURFACE_HEAT_FLUX); VAL(CSI_F_ML_COEFFICIENT);
    VAL(CSI_F_ML_REFERENCE_TEMPERATURE); VAL(CSI_F_ML_DEEP_HEAT_FLUX); VAL(CSI_F_ML_SURFACE_FLUX_USED); VAL(CSI_F_COUNT_MIXED_LAYER);
    VAL(CSI_VERSION);
    printf(", \"sizeof_params\": %d", (int)sizeof(csi_mixed_layer_params));
    OFF(csi_mixed_layer_params, density); OFF(csi_mixed_layer_params, heat_capacity); OFF(csi_mixed_layer_params, depth);
    OFF(csi_mixed_layer_params, exchange_velocity); OFF(csi_mixed_layer_params, surface_heat_flux); OFF(csi_mixed_layer_params, coefficient);
    OFF(csi_mixed_layer_params, reference_temperature); OFF(csi_mixed_layer_params, deep_heat_flux); OFF(csi_mixed_layer_params, flags);
    OFF(csi_mixed_layer_params, reserved);
    printf("}\n");
    return 0;
}
