/* tracers_layout.c -- csi_tracers, CSI_TRACERS_MAX, the weighting codes and CSI_TRACER_FIELD as a C compiler sees include/csi.h, printed
 * as JSON for tests/test_tracers_ref.py. */
#include <stddef.h>
#include <stdio.h>

#include "csi.h"

#define VAL(x) printf("%s\"%s\": %d", first ? "" : ", ", #x, (int)(x)), first = 0
#define OFF(T, f) printf("%s\"%s.%s\": %d", first ? "" : ", ", #T, #f, (int)offsetof(T, f)), first = 0

int main(void) {
    int first = 1;
    printf("{");
    VAL(CSI_TRACERS_MAX); VAL(CSI_TRACER_PLAIN); VAL(CSI_TRACER_BY_CONCENTRATION); VAL(CSI_F_COUNT_SHORTWAVE); VAL(CSI_VERSION);
    printf(", \"CSI_TRACER_FIELD_0\": %d, \"CSI_TRACER_FIELD_7\": %d", (int)CSI_TRACER_FIELD(0), (int)CSI_TRACER_FIELD(7));
    printf(", \"sizeof_tracers\": %d", (int)sizeof(csi_tracers));
    OFF(csi_tracers, n); OFF(csi_tracers, c); OFF(csi_tracers, G); OFF(csi_tracers, weighting); OFF(csi_tracers, nonnegative);
    OFF(csi_tracers, source);
    printf("}\n");
    return 0;
}
