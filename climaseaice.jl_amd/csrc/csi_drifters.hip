// csi_drifters.hip -- csi_drifters_locate, csi_drifters_advance, csi_drifters_sample, csi_drifters_stats (include/csi.h): Lagrangian ice
// drifters.  Stands where users of the reference copy u and v to the host after every step and integrate their buoy tracks there.
// The kernels: drifters.hip; the rule: drifters_dev.h.
//
// Host side: csi_drifters_locate is drifters_dev.h's locate() itself, callable without a context or a GPU; the two device entries are
// argument and binding checks by name and ONE launch each on the context's stream (nothing is waited for: the positions are read by
// whatever is queued next).  The arrays are the caller's and arrive with every call: the library keeps no drifter state.
#include "csi_ctx.h"
#include "drifters_dev.h"

namespace csi_host {

// what both device entries check; *D holds the grid, u, v and the caller's arrays afterwards
static int32_t drifters_common(csi_context* c, const char* who, const csi_drifters* d, DriftersDev* D) {
    const std::string w = std::string(who) + ": ";
    if (!d) return fail(c, CSI_ERR_INVALID_ARGUMENT, w + "the csi_drifters pointer is NULL");
    if (d->n < 0) return fail(c, CSI_ERR_INVALID_ARGUMENT, w + "n < 0");
    if (d->n > 0 && (!d->xi || !d->eta || !d->status)) return fail(c, CSI_ERR_INVALID_ARGUMENT, w + "xi, eta and status must be device arrays of n entries (NULL with n > 0)");
    if (!c->grid_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_grid_set has not been called");
    if (c->Hx < 1 || c->Hy < 1) return fail(c, CSI_ERR_INVALID_ARGUMENT, w + "the grid needs halo >= 1");
    if (is_tiled(c)) return fail(c, CSI_ERR_UNSUPPORTED, w + "a tiled context is not supported (a drifter would have to migrate between ranks)");
    if (c->g.yhi == SIDE_FOLD) return fail(c, CSI_ERR_UNSUPPORTED, w + "a RIGHT_FOLDED topology is not supported (crossing the fold re-orients the drifter)");
    if (int32_t rc = need_named(c, who, "every call ", {CSI_F_U, CSI_F_V}, ": a model without velocities moves no drifters")) return rc;
    D->g = c->g;
    D->u = ref_of(c, CSI_F_U);
    D->v = ref_of(c, CSI_F_V);
    D->xi = d->xi; D->eta = d->eta; D->status = d->status;
    D->n = (long)d->n;
    return CSI_OK;
}

}  // namespace csi_host

extern "C" {

int32_t csi_drifters_locate(int32_t Nx, int32_t Ny, double xi, double eta, int32_t* idx, double* w) {
    if (Nx < 1 || Ny < 1 || !idx || !w) return CSI_ERR_INVALID_ARGUMENT;
    const csi::drift::Stencil s = csi::drift::locate(Nx, Ny, xi, eta);
    idx[0] = s.ia; idx[1] = s.ja; idx[2] = s.ib; idx[3] = s.jb; idx[4] = s.ic; idx[5] = s.jc;
    w[0] = s.sx; w[1] = s.sy; w[2] = s.rx; w[3] = s.ry;
    return CSI_OK;
}

int32_t csi_drifters_advance(csi_context* c, const csi_drifters* d, double dt, int32_t substeps) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    int32_t rc = peer_check_entry(c);
    if (rc) return rc;
    if (!std::isfinite(dt)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "drifters advance: dt is not finite");
    if (substeps < 1) return fail(c, CSI_ERR_INVALID_ARGUMENT, "drifters advance: substeps < 1");
    DriftersDev D{};
    if ((rc = drifters_common(c, "drifters advance", d, &D))) return rc;
    if (D.n == 0) return CSI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const double tau = dt / (double)substeps;      // formed once, here
    launch_drifters_advance(D, tau, substeps, c->stream);
    HIP_TRY(c, hipGetLastError());
    ++c->drifter_launches;
    return CSI_OK;
}

int32_t csi_drifters_sample(csi_context* c, const csi_drifters* d, int32_t columns, void* dev_out, int64_t ld) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    int32_t rc = peer_check_entry(c);
    if (rc) return rc;
    if (columns == 0 || (columns & ~CSI_DRIFTER_COL_ALL)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "drifters sample: `columns` must be a non-empty set of the CSI_DRIFTER_COL_* bits (1 .. 64); unknown bit");
    DriftersDev D{};
    if ((rc = drifters_common(c, "drifters sample", d, &D))) return rc;
    if (D.n > 0 && !dev_out) return fail(c, CSI_ERR_INVALID_ARGUMENT, "drifters sample: dev_out == NULL");
    if (ld < d->n) return fail(c, CSI_ERR_INVALID_ARGUMENT, "drifters sample: ld < n");
    const struct { int bit, fid; FRef* ref; } cell[3] = {{CSI_DRIFTER_COL_H, CSI_F_H, &D.h}, {CSI_DRIFTER_COL_A, CSI_F_A, &D.a}, {CSI_DRIFTER_COL_HS, CSI_F_HS, &D.hs}};
    for (const auto& k : cell) {
        if (!(columns & k.bit)) continue;
        if (!c->f[k.fid].p) return fail(c, CSI_ERR_NOT_BOUND, std::string("drifters sample: field ") + slot_name(k.fid) + " is requested as a column but not bound");
        *k.ref = ref_of(c, k.fid);
    }
    if (D.n == 0) return CSI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    launch_drifters_sample(D, columns, (double*)dev_out, (long)ld, c->stream);
    HIP_TRY(c, hipGetLastError());
    ++c->drifter_launches;
    return CSI_OK;
}

int32_t csi_drifters_stats(csi_context* c, int64_t* launches) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (launches) *launches = c->drifter_launches;
    return CSI_OK;
}

}
