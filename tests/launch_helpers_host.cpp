// The pure-host launch helpers of csrc/csi_ctx.h in a program of their own (tests/test_launch_helpers.py builds it with the host
// sanitizers and runs it): the advection scheme table, the copy batch's add with its alignment flag, the row clip of a sub-step's
// ranges.  No HIP call is made.
#include "csi_ctx.h"

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main() {
    // every scheme of include/csi.h and its halo; anything else is unknown
    const int known[6][2] = {{CSI_ADVECT_UPWIND1, 1}, {CSI_ADVECT_WENO3, 2}, {CSI_ADVECT_UPWIND3, 2}, {CSI_ADVECT_WENO5, 3}, {CSI_ADVECT_UPWIND5, 3}, {CSI_ADVECT_WENO7, 4}};
    for (int s = -9; s <= 9; ++s) {
        int want = 0;
        for (const auto& k : known) if (k[0] == s) want = k[1];
        CHECK(advect_halo(s) == want);
    }
    csi_context c;
    c.Hx = 3; c.Hy = 4;
    CHECK(advect_fits(&c, CSI_ADVECT_WENO5) && !advect_fits(&c, CSI_ADVECT_WENO7) && !advect_fits(&c, CSI_ADVECT_NONE) && !advect_fits(&c, 2));

    // copy batches: aligned16 follows the pointers of a batch started aligned, and stays 0 in one started as CopyBatch{}
    alignas(16) static double a[8], b[8];
    CopyBatch B = copy_batch_aligned();
    CHECK(B.count == 0 && B.aligned16 == 1);
    copy_add(B, a, b, 8); copy_add(B, a + 2, b + 4, 4);
    CHECK(B.count == 2 && B.aligned16 == 1 && B.src[1] == a + 2 && B.dst[1] == b + 4 && B.n[0] == 8 && B.n[1] == 4);
    copy_add(B, a, b + 1, 2);
    CHECK(B.count == 3 && B.aligned16 == 0);
    copy_add(B, a, b, 2);
    CHECK(B.count == 4 && B.aligned16 == 0);
    CopyBatch F{};
    for (int q = 0; q < 6; ++q) copy_add(F, a, b, 1);      // (six entries: the batch's capacity)
    CHECK(F.count == 6 && F.aligned16 == 0);

    // the fold band's clip: the stress from row jlo, the velocities from jlo + 1, never below the range's own first row
    const SubstepRanges R{Range{-2, 11, -2, 11}, Range{1, 8, 1, 8}, Range{1, 8, 2, 8}, Range{1, 8, 1, 8}};
    const SubstepRanges lo = R.from_row(-100), hi = R.from_row(5);
    CHECK(lo.rs.j0 == -2 && lo.ru1.j0 == 1 && lo.rv1.j0 == 2 && lo.r2.j0 == 1);
    CHECK(hi.rs.j0 == 5 && hi.ru1.j0 == 6 && hi.rv1.j0 == 6 && hi.r2.j0 == 6 && hi.rs.j1 == 11 && hi.rs.i0 == -2 && hi.r2.i1 == 8);
    printf("ok\n");
    return 0;
}
