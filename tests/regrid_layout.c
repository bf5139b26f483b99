/* What a C compiler makes of the regridding additions to include/csi.h (tests/test_regrid_ref.py): the layout of csi_regrid_map and the
 * values of the new enumerators.  Prints NAME=value lines. */
#include <stddef.h>
#include <stdio.h>
#include "csi.h"

#define OFF(f) printf("offset_" #f "=%d\n", (int)offsetof(csi_regrid_map, f))

int main(void) {
    printf("CSI_REGRID_FACE_CENTER=%d\n", (int)CSI_REGRID_FACE_CENTER);
    printf("CSI_REGRID_CENTER_FACE=%d\n", (int)CSI_REGRID_CENTER_FACE);
    printf("CSI_REGRID_CENTER_CENTER=%d\n", (int)CSI_REGRID_CENTER_CENTER);
    printf("CSI_REGRID_MAX_MAPS=%d\n", (int)CSI_REGRID_MAX_MAPS);
    printf("CSI_REGRID_MAX_SOURCE_EXTENT=%d\n", (int)CSI_REGRID_MAX_SOURCE_EXTENT);
    printf("sizeof=%d\n", (int)sizeof(csi_regrid_map));
    printf("sizeof_time_series=%d\n", (int)sizeof(csi_time_series));
    OFF(location); OFF(nx); OFF(ny); OFF(src_nx); OFF(src_ny); OFF(reserved); OFF(i0); OFF(i1); OFF(j0); OFF(j1); OFF(wx); OFF(wy); OFF(cos); OFF(sin);
    /* the prototypes of the new entry points as a C client sees them (unevaluated: nothing to link against) */
    printf("plan_axis_result_bytes=%d\n", (int)sizeof(csi_regrid_plan_axis((const double*)0, 2, 0, 0.0, 0.0, (int32_t*)0, (int32_t*)0, (double*)0)));
    printf("create_result_bytes=%d\n", (int)sizeof(csi_regrid_map_create((csi_context*)0, (const csi_regrid_map*)0, (int32_t*)0)));
    printf("destroy_result_bytes=%d\n", (int)sizeof(csi_regrid_map_destroy((csi_context*)0, 0)));
    printf("set_result_bytes=%d\n", (int)sizeof(csi_time_series_set_regridded((csi_context*)0, CSI_F_SNOWFALL, (const csi_time_series*)0, 0, (const csi_time_series*)0, 0)));
    printf("stats_result_bytes=%d\n", (int)sizeof(csi_regrid_stats((csi_context*)0, (int64_t*)0, (int32_t*)0)));
    return 0;
}
