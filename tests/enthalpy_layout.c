/* enthalpy_layout.c -- csi_enthalpy_params, csi_enthalpy_launch and the enums added with the enthalpy-method column model, as a C
 * compiler sees include/csi.h, printed as JSON for tests/test_enthalpy_ref.py. */
#include <stddef.h>
#include <stdio.h>

#include "csi.h"

#define VAL(x) printf("%s\"%s\": %d", first ? "" : ", ", #x, (int)(x)), first = 0
#define OFF(T, f) printf("%s\"%s.%s\": %d", first ? "" : ", ", #T, #f, (int)offsetof(T, f)), first = 0

int main(void) {
    int first = 1;
    printf("{");
    VAL(CSI_ENTH_H); VAL(CSI_ENTH_T); VAL(CSI_ENTH_PHI); VAL(CSI_ENTH_KAPPA);
    VAL(CSI_ENTH_T_BOTTOM); VAL(CSI_ENTH_T_TOP); VAL(CSI_ENTH_H_BOTTOM); VAL(CSI_ENTH_H_TOP);
    VAL(CSI_ENTH_BC_NONE); VAL(CSI_ENTH_BC_NUMBER); VAL(CSI_ENTH_BC_ARRAY); VAL(CSI_ENTH_BC_SERIES_SCALAR); VAL(CSI_ENTH_BC_SERIES_PLANE);
    VAL(CSI_ENTH_BC_FLUX); VAL(CSI_ENTH_BC_GRADIENT);
    VAL(CSI_ENTH_PER_STEP); VAL(CSI_ENTH_ON_CHIP); VAL(CSI_ENTH_MAX_SUBSTEPS); VAL(CSI_ENTH_MIN_WAVES_PER_CU); VAL(CSI_ENTH_LDS_PER_CU);
    VAL(CSI_F_COUNT_SHORTWAVE); VAL(CSI_VERSION);
    printf(", \"sizeof_params\": %d, \"sizeof_launch\": %d", (int)sizeof(csi_enthalpy_params), (int)sizeof(csi_enthalpy_launch));
    OFF(csi_enthalpy_params, Nx); OFF(csi_enthalpy_params, Ny); OFF(csi_enthalpy_params, Nz); OFF(csi_enthalpy_params, reserved);
    OFF(csi_enthalpy_params, z_faces); OFF(csi_enthalpy_params, ice_heat_capacity); OFF(csi_enthalpy_params, water_heat_capacity);
    OFF(csi_enthalpy_params, fusion_enthalpy); OFF(csi_enthalpy_params, kappa_ice); OFF(csi_enthalpy_params, kappa_water);
    OFF(csi_enthalpy_launch, form); OFF(csi_enthalpy_launch, launches); OFF(csi_enthalpy_launch, substeps_per_launch);
    OFF(csi_enthalpy_launch, lds_bytes);
    printf("}\n");
    return 0;
}
