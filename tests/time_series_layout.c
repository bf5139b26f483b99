/* What a C compiler makes of the time-series additions to include/csi.h (tests/test_time_series_plan.py): the layout of
 * csi_time_series and the values of the new enumerators.  Prints NAME=value lines. */
#include <stddef.h>
#include <stdio.h>
#include "csi.h"

#define OFF(f) printf("offset_" #f "=%d\n", (int)offsetof(csi_time_series, f))

int main(void) {
    printf("CSI_VERSION=%d\n", (int)CSI_VERSION);
    printf("CSI_F_COUNT_TOTAL=%d\n", (int)CSI_F_COUNT_TOTAL);
    printf("CSI_TIME_CLAMP=%d\n", (int)CSI_TIME_CLAMP);
    printf("CSI_TIME_CYCLICAL=%d\n", (int)CSI_TIME_CYCLICAL);
    printf("CSI_TIME_LINEAR=%d\n", (int)CSI_TIME_LINEAR);
    printf("CSI_SERIES_DEVICE=%d\n", (int)CSI_SERIES_DEVICE);
    printf("CSI_SERIES_HOST=%d\n", (int)CSI_SERIES_HOST);
    printf("sizeof=%d\n", (int)sizeof(csi_time_series));
    OFF(nt); OFF(indexing); OFF(backend); OFF(window); OFF(period); OFF(times); OFF(data); OFF(ld); OFF(slice_stride);
    /* the prototypes of the new entry points as a C client sees them (unevaluated: nothing to link against) */
    printf("plan_result_bytes=%d\n", (int)sizeof(csi_time_series_plan((const double*)0, 2, CSI_TIME_CLAMP, 0.0, 0.0, (int32_t*)0, (int32_t*)0, (double*)0)));
    printf("set_result_bytes=%d\n", (int)sizeof(csi_time_series_set((csi_context*)0, CSI_F_SNOWFALL, (const csi_time_series*)0)));
    printf("update_result_bytes=%d\n", (int)sizeof(csi_time_series_update((csi_context*)0, 0.0)));
    printf("status_result_bytes=%d\n", (int)sizeof(csi_time_series_status((csi_context*)0, CSI_F_SNOWFALL, (int32_t*)0, (int64_t*)0)));
    return 0;
}
