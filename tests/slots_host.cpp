// Prints the library's slot table (csrc/csi_slots.h), one row per line: id, display name, x location, y location, role bits.
// Plain g++, no HIP: tests/test_slot_table.py compiles it and compares the rows with _lib.SLOTS.
#include "../climaseaice.jl_amd/csrc/csi_slots.h"
#include <cstdio>

int main() {
    using namespace csi_host;
    for (int k = 0; k < kSlotCount; ++k)
        if (slot_known(k)) printf("%d %s %d %d %u\n", kSlots[k].id, slot_name(k), slot_loc(k, 0), slot_loc(k, 1), kSlots[k].roles);
    printf("roles %u %u %u %u\n", (unsigned)SLOT_HALO, (unsigned)SLOT_PEER, (unsigned)SLOT_FORCING, (unsigned)SLOT_SERIES);
    printf("forcing");
    for (int id : slots_with(SLOT_FORCING)) printf(" %d", id);
    printf("\nknown %d %d\n", (int)slot_known(-1), (int)slot_known(kSlotCount));
    return 0;
}
