/* What a C compiler makes of the momentum-term additions to include/csi.h (tests/test_momentum_terms_ref.py): the layout of
 * csi_momentum_budget, the term slots, the mask bits and the groups.  Prints NAME=value lines. */
#include <stddef.h>
#include <stdio.h>
#include "csi.h"

#define OFF(f) printf("offset_" #f "=%d\n", (int)offsetof(csi_momentum_budget, f))
#define VAL(n) printf(#n "=%d\n", (int)(n))

int main(void) {
    VAL(CSI_VERSION); VAL(CSI_F_COUNT); VAL(CSI_F_COUNT_ALL); VAL(CSI_F_COUNT_TOTAL); VAL(CSI_F_COUNT_DERIVED); VAL(CSI_F_D_STRESS_POWER);
    VAL(CSI_F_M_CORIOLIS_X); VAL(CSI_F_M_CORIOLIS_Y); VAL(CSI_F_M_TOP_X); VAL(CSI_F_M_TOP_Y); VAL(CSI_F_M_BOTTOM_X); VAL(CSI_F_M_BOTTOM_Y);
    VAL(CSI_F_M_INTERNAL_X); VAL(CSI_F_M_INTERNAL_Y); VAL(CSI_F_M_FORCING_X); VAL(CSI_F_M_FORCING_Y); VAL(CSI_F_COUNT_BINDABLE);
    VAL(CSI_MTERM_CORIOLIS); VAL(CSI_MTERM_TOP); VAL(CSI_MTERM_BOTTOM); VAL(CSI_MTERM_INTERNAL); VAL(CSI_MTERM_FORCING); VAL(CSI_MTERM_ALL);
    VAL(CSI_MTERM_RAW_STRESS);
    VAL(CSI_MBUDGET_EXTERNAL); VAL(CSI_MBUDGET_BODY); VAL(CSI_MBUDGET_INTERNAL); VAL(CSI_MBUDGET_ALL);
    printf("sizeof=%d\n", (int)sizeof(csi_momentum_budget));
    printf("sizeof_budget=%d\n", (int)sizeof(csi_budget));
    OFF(what); OFF(reserved); OFF(coriolis); OFF(top); OFF(bottom); OFF(internal); OFF(forcing);
    /* the prototypes of the new entry points as a C client sees them (unevaluated: nothing to link against) */
    printf("terms_result_bytes=%d\n", (int)sizeof(csi_momentum_terms_compute((csi_context*)0, CSI_MTERM_ALL)));
    printf("budget_result_bytes=%d\n", (int)sizeof(csi_momentum_budget_compute((csi_context*)0, CSI_MBUDGET_ALL, (csi_momentum_budget*)0)));
    printf("stats_result_bytes=%d\n", (int)sizeof(csi_momentum_terms_stats((csi_context*)0, (int64_t*)0, (int64_t*)0)));
    return 0;
}
