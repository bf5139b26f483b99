/* What a C compiler makes of the derived-field and energy-budget additions to include/csi.h (tests/test_derived_ref.py): the layout of
 * csi_budget, the derived slots and the mask bits.  Prints NAME=value lines. */
#include <stddef.h>
#include <stdio.h>
#include "csi.h"

#define OFF(f) printf("offset_" #f "=%d\n", (int)offsetof(csi_budget, f))
#define VAL(n) printf(#n "=%d\n", (int)(n))

int main(void) {
    VAL(CSI_VERSION); VAL(CSI_F_COUNT); VAL(CSI_F_COUNT_ALL); VAL(CSI_F_COUNT_TOTAL); VAL(CSI_F_FREE_DRIFT_V);
    VAL(CSI_F_D_DIVERGENCE); VAL(CSI_F_D_SHEAR); VAL(CSI_F_D_DEFORMATION); VAL(CSI_F_D_SPEED); VAL(CSI_F_D_SIGMA_I); VAL(CSI_F_D_SIGMA_II);
    VAL(CSI_F_D_STRESS_POWER); VAL(CSI_F_COUNT_DERIVED);
    VAL(CSI_DERIVED_DIVERGENCE); VAL(CSI_DERIVED_SHEAR); VAL(CSI_DERIVED_DEFORMATION); VAL(CSI_DERIVED_SPEED); VAL(CSI_DERIVED_SIGMA_I);
    VAL(CSI_DERIVED_SIGMA_II); VAL(CSI_DERIVED_STRESS_POWER); VAL(CSI_DERIVED_ALL);
    VAL(CSI_BUDGET_STRESS); VAL(CSI_BUDGET_KINETIC); VAL(CSI_BUDGET_ALL);
    printf("sizeof=%d\n", (int)sizeof(csi_budget));
    printf("sizeof_diagnostics=%d\n", (int)sizeof(csi_diagnostics));
    OFF(what); OFF(reserved); OFF(internal_work); OFF(stress_power); OFF(kinetic_energy);
    /* the prototypes of the new entry points as a C client sees them (unevaluated: nothing to link against) */
    printf("derived_result_bytes=%d\n", (int)sizeof(csi_derived_compute((csi_context*)0, CSI_DERIVED_ALL)));
    printf("budget_result_bytes=%d\n", (int)sizeof(csi_budget_compute((csi_context*)0, CSI_BUDGET_ALL, (csi_budget*)0)));
    printf("stats_result_bytes=%d\n", (int)sizeof(csi_derived_stats((csi_context*)0, (int64_t*)0, (int64_t*)0)));
    return 0;
}
