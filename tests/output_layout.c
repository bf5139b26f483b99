/* What a C compiler makes of the output additions to include/csi.h (tests/test_output_ref.py): the layout of csi_output_field and
 * the values of the constants.  Prints NAME=value lines. */
#include <stddef.h>
#include <stdio.h>
#include "csi.h"

#define OFF(f) printf("offset_" #f "=%d\n", (int)offsetof(csi_output_field, f))

int main(void) {
    printf("CSI_OUT_F64=%d\n", (int)CSI_OUT_F64);
    printf("CSI_OUT_F32=%d\n", (int)CSI_OUT_F32);
    printf("CSI_OUTPUT_MAX_FIELDS=%d\n", (int)CSI_OUTPUT_MAX_FIELDS);
    printf("CSI_OUTPUT_MAX_SETS=%d\n", (int)CSI_OUTPUT_MAX_SETS);
    printf("CSI_OUTPUT_MAX_SLOTS=%d\n", (int)CSI_OUTPUT_MAX_SLOTS);
    printf("sizeof=%d\n", (int)sizeof(csi_output_field));
    OFF(field_id); OFF(dtype); OFF(averaged); OFF(masked); OFF(fill_value);
    /* the prototypes as a C client sees them (unevaluated: nothing to link against) */
    printf("create_result_bytes=%d\n", (int)sizeof(csi_output_create((csi_context*)0, (const csi_output_field*)0, 1, 2, (int32_t*)0)));
    printf("wait_result_bytes=%d\n", (int)sizeof(csi_output_wait((csi_context*)0, 1, 0, (void**)0)));
    return 0;
}
