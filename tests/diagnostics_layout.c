/* What a C compiler makes of the diagnostics additions to include/csi.h (tests/test_diagnostics_ref.py): the layout of
 * csi_diagnostics and the values of the group bits.  Prints NAME=value lines. */
#include <stddef.h>
#include <stdio.h>
#include "csi.h"

#define OFF(f) printf("offset_" #f "=%d\n", (int)offsetof(csi_diagnostics, f))

int main(void) {
    printf("CSI_VERSION=%d\n", (int)CSI_VERSION);
    printf("CSI_F_COUNT_TOTAL=%d\n", (int)CSI_F_COUNT_TOTAL);
    printf("CSI_DIAG_VELOCITY=%d\n", (int)CSI_DIAG_VELOCITY);
    printf("CSI_DIAG_TRACERS=%d\n", (int)CSI_DIAG_TRACERS);
    printf("CSI_DIAG_ALL=%d\n", (int)CSI_DIAG_ALL);
    printf("sizeof=%d\n", (int)sizeof(csi_diagnostics));
    OFF(what); OFF(has_snow);
    OFF(advection_timescale); OFF(inv_timescale_max); OFF(max_abs_u); OFF(max_abs_v);
    OFF(nonfinite_u); OFF(nonfinite_v); OFF(nan_u); OFF(nan_v);
    OFF(ice_volume); OFF(ice_area); OFF(ice_extent); OFF(snow_volume); OFF(active_area);
    OFF(min_h); OFF(max_h); OFF(min_aice); OFF(max_aice); OFF(max_hs);
    OFF(nonfinite_h); OFF(nonfinite_aice); OFF(nonfinite_hs); OFF(active_cells);
    OFF(extent_threshold);
    /* the prototype of the new entry point as a C client sees it (unevaluated: nothing to link against) */
    printf("compute_result_bytes=%d\n", (int)sizeof(csi_diagnostics_compute((csi_context*)0, CSI_DIAG_ALL, 0.15, (csi_diagnostics*)0)));
    return 0;
}
