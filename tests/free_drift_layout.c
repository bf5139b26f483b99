/* What a C compiler makes of the free-drift additions to include/csi.h (tests/test_free_drift.py): the values of the new
 * enumerators next to the counts the older tests pin.  Prints NAME=value lines. */
#include <stdio.h>
#include "csi.h"

int main(void) {
    printf("CSI_VERSION=%d\n", (int)CSI_VERSION);
    printf("CSI_F_COUNT=%d\n", (int)CSI_F_COUNT);
    printf("CSI_F_COUNT_ALL=%d\n", (int)CSI_F_COUNT_ALL);
    printf("CSI_F_FREE_DRIFT_U=%d\n", (int)CSI_F_FREE_DRIFT_U);
    printf("CSI_F_FREE_DRIFT_V=%d\n", (int)CSI_F_FREE_DRIFT_V);
    printf("CSI_F_COUNT_TOTAL=%d\n", (int)CSI_F_COUNT_TOTAL);
    printf("CSI_FREE_DRIFT_FIELDS=%d\n", (int)CSI_FREE_DRIFT_FIELDS);
    printf("CSI_DYNAMICS_FREE_DRIFT=%d\n", (int)CSI_DYNAMICS_FREE_DRIFT);
    /* the prototype of the new entry point as a C client sees it (unevaluated: nothing to link against) */
    printf("csi_dynamics_set_result_bytes=%d\n", (int)sizeof(csi_dynamics_set((csi_context*)0, CSI_DYNAMICS_FREE_DRIFT)));
    return 0;
}
