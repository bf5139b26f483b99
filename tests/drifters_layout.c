/* drifters_layout.c -- csi_drifters and the bits added with the Lagrangian ice drifters, as a C compiler sees include/csi.h, printed as
 * JSON for tests/test_drifters_ref.py. */
#include <stddef.h>
#include <stdio.h>

#include "csi.h"

#define VAL(x) printf("%s\"%s\": %d", first ? "" : ", ", #x, (int)(x)), first = 0
#define OFF(T, f) printf("%s\"%s.%s\": %d", first ? "" : ", ", #T, #f, (int)offsetof(T, f)), first = 0

int main(void) {
    int first = 1;
    printf("{");
    VAL(CSI_DRIFTER_CLAMPED_X); VAL(CSI_DRIFTER_CLAMPED_Y); VAL(CSI_DRIFTER_HELD); VAL(CSI_DRIFTER_LOST); VAL(CSI_DRIFTER_INACTIVE);
    VAL(CSI_DRIFTER_COL_XI); VAL(CSI_DRIFTER_COL_ETA); VAL(CSI_DRIFTER_COL_U); VAL(CSI_DRIFTER_COL_V); VAL(CSI_DRIFTER_COL_H);
    VAL(CSI_DRIFTER_COL_A); VAL(CSI_DRIFTER_COL_HS); VAL(CSI_DRIFTER_COL_ALL);
    VAL(CSI_F_COUNT_SHORTWAVE); VAL(CSI_VERSION);
    printf(", \"sizeof_drifters\": %d", (int)sizeof(csi_drifters));
    OFF(csi_drifters, n); OFF(csi_drifters, xi); OFF(csi_drifters, eta); OFF(csi_drifters, status);
    printf("}\n");
    return 0;
}
