/* regions_layout.c -- csi_regions, csi_region_record and CSI_REGIONS_MAX as a C compiler sees include/csi.h, printed as JSON for
 * tests/test_regional_ref.py. */
#include <stddef.h>
#include <stdio.h>

#include "csi.h"

#define VAL(x) printf("%s\"%s\": %d", first ? "" : ", ", #x, (int)(x)), first = 0
#define OFF(T, f) printf("%s\"%s.%s\": %d", first ? "" : ", ", #T, #f, (int)offsetof(T, f)), first = 0

int main(void) {
    int first = 1;
    printf("{");
    VAL(CSI_REGIONS_MAX); VAL(CSI_F_COUNT_SHORTWAVE); VAL(CSI_VERSION);
    printf(", \"sizeof_regions\": %d, \"sizeof_region_record\": %d", (int)sizeof(csi_regions), (int)sizeof(csi_region_record));
    OFF(csi_regions, ids); OFF(csi_regions, ld); OFF(csi_regions, n_regions); OFF(csi_regions, reserved);
    OFF(csi_region_record, ice_volume); OFF(csi_region_record, ice_area); OFF(csi_region_record, ice_extent);
    OFF(csi_region_record, snow_volume); OFF(csi_region_record, region_area); OFF(csi_region_record, min_h);
    OFF(csi_region_record, max_h); OFF(csi_region_record, min_aice); OFF(csi_region_record, max_aice);
    OFF(csi_region_record, max_hs); OFF(csi_region_record, cells);
    printf("}\n");
    return 0;
}
