// csi_diagnostics.hip -- csi_diagnostics_compute (include/csi.h): scalars computed from the bound fields on the device.
// Stands where the reference's root module has cell_advection_timescale(model::SeaIceModel) (src/ClimaSeaIce.jl:63-69) and where its
// tests and validation scripts reduce whole fields on the host.  The kernels and the summation order: diagnostics.hip.
//
// Host side: argument and binding checks, the two launches and the copy of the DQ_COUNT result slots into page-locked memory on the
// context's stream, ONE wait for that stream; on a tiled context the all-gather of every rank's slots and their combine in rank
// order.  A rank that fails locally (a missing field, a HIP error) still reaches the all-gather, with a status word that makes every
// rank return an error: an early return would strand the others inside the collective (as in csi_peer.hip peer_setup).
#include "csi_ctx.h"

namespace csi_host {

static int32_t diag_local(csi_context* c, int32_t what, double thr, double* slots) {
    if (what == 0 || (what & ~CSI_DIAG_ALL)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "diagnostics: `what` must be a non-empty mask of CSI_DIAG_VELOCITY (1) and CSI_DIAG_TRACERS (2); unknown bit");
    if (!std::isfinite(thr) || thr < 0.0) return fail(c, CSI_ERR_INVALID_ARGUMENT, "diagnostics: extent_threshold must be finite and >= 0");
    if (!c->grid_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_grid_set has not been called");
    const bool vel = what & CSI_DIAG_VELOCITY, trc = what & CSI_DIAG_TRACERS;
    if (vel)
        for (int id : {CSI_F_U, CSI_F_V})
            if (!c->f[id].p) return fail(c, CSI_ERR_NOT_BOUND, std::string("diagnostics: the velocity group needs field ") + kName[id] + " (not bound: a model without dynamics supports CSI_DIAG_TRACERS only)");
    if (trc)
        for (int id : {CSI_F_H, CSI_F_A})
            if (!c->f[id].p) return fail(c, CSI_ERR_NOT_BOUND, std::string("diagnostics: the tracer group needs field ") + kName[id] + " (not bound)");
    HIP_TRY(c, hipSetDevice(c->device));
    DiagDev D{};
    D.g = c->g;
    D.u = ref_of(c, CSI_F_U); D.v = ref_of(c, CSI_F_V); D.h = ref_of(c, CSI_F_H); D.a = ref_of(c, CSI_F_A); D.hs = ref_of(c, CSI_F_HS);
    D.has_hs = c->f[CSI_F_HS].p != nullptr;
    D.exu = extra_x(c, CSI_F_U); D.eyv = extra_y(c, CSI_F_V);
    // the kernel reads u up to column Nx + exu and v up to row Ny + eyv: what csi_field_bind has checked the parents against
    if (vel && (c->f[CSI_F_U].ni < c->Nx + 2 * c->Hx + D.exu || c->f[CSI_F_V].nj < c->Ny + 2 * c->Hy + D.eyv))
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "diagnostics: u / v parents are smaller than the grid's Face fields");
    D.threshold = thr;
    int nbx, nby;
    diag_geometry(c->Nx, c->Ny, &nbx, &nby);
    D.nrec = (long)nbx * nby;
    HIP_TRY(c, c->diag_part.ensure((size_t)(D.nrec + 1) * DQ_COUNT, c->stream, false));
    if (!c->diag_host) HIP_TRY(c, c->diag_host.alloc(DQ_COUNT, hipHostMallocDefault));
    D.part = c->diag_part.get();
    double* result = D.part + (size_t)D.nrec * DQ_COUNT;
    launch_diagnostics(D, vel, trc, result, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->diag_host.get(), result, sizeof(double) * DQ_COUNT, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(slots, c->diag_host.get(), sizeof(double) * DQ_COUNT);
    return CSI_OK;
}

static int64_t as_count(double slot) { int64_t n; memcpy(&n, &slot, sizeof n); return n; }
static double from_count(int64_t n) { double d; memcpy(&d, &n, sizeof d); return d; }
static bool is_sum(int q) { return q >= DQ_VOLUME && q <= DQ_ACTIVE_AREA; }
static bool is_max(int q) { return q == DQ_INV_TIMESCALE || q == DQ_MAX_ABS_U || q == DQ_MAX_ABS_V || q == DQ_MAX_H || q == DQ_MAX_AICE || q == DQ_MAX_HS; }
static bool is_min(int q) { return q == DQ_MIN_H || q == DQ_MIN_AICE; }

}  // namespace csi_host

extern "C" {

int32_t csi_diagnostics_compute(csi_context* c, int32_t what, double extent_threshold, csi_diagnostics* out) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, CSI_ERR_INVALID_ARGUMENT, "diagnostics: out == NULL");
    struct Payload { int64_t status; double slot[DQ_COUNT]; } mine{};
    int32_t rc = peer_check_entry(c);
    if (!rc) rc = diag_local(c, what, extent_threshold, mine.slot);
    mine.status = rc;
    double slot[DQ_COUNT];
    memcpy(slot, mine.slot, sizeof slot);
    if (has_comm(c)) {
        std::vector<uint8_t> all;
        const std::string local_err = c->err;
        const int32_t grc = comm_allgather(c, &mine, sizeof mine, all);
        if (rc) { c->err = local_err; return rc; }
        if (grc) return grc;
        const bool vel = what & CSI_DIAG_VELOCITY;
        for (int r = 0; r < c->world; ++r) {
            Payload p;
            memcpy(&p, all.data() + (size_t)r * sizeof p, sizeof p);
            if (p.status) return fail(c, CSI_ERR_COMM, "diagnostics: rank " + std::to_string(r) + " of the decomposition failed locally (status " + std::to_string((long)p.status) + ")");
            for (int q = vel ? 0 : DQ_VOLUME; q < ((what & CSI_DIAG_TRACERS) ? DQ_COUNT : DQ_VOLUME); ++q) {
                if (r == 0) slot[q] = p.slot[q];
                else if (is_sum(q)) slot[q] = slot[q] + p.slot[q];
                else if (is_max(q)) slot[q] = std::fmax(slot[q], p.slot[q]);
                else if (is_min(q)) slot[q] = std::fmin(slot[q], p.slot[q]);
                else slot[q] = from_count(as_count(slot[q]) + as_count(p.slot[q]));
            }
        }
    } else if (rc) {
        return rc;
    }
    const double nan = std::nan("");
    csi_diagnostics d{};
    d.what = what;
    d.has_snow = c->f[CSI_F_HS].p != nullptr && (what & CSI_DIAG_TRACERS) ? 1 : 0;
    d.extent_threshold = extent_threshold;
    d.advection_timescale = d.inv_timescale_max = d.max_abs_u = d.max_abs_v = nan;
    d.nonfinite_u = d.nonfinite_v = d.nan_u = d.nan_v = -1;
    d.ice_volume = d.ice_area = d.ice_extent = d.snow_volume = d.active_area = nan;
    d.min_h = d.max_h = d.min_aice = d.max_aice = d.max_hs = nan;
    d.nonfinite_h = d.nonfinite_aice = d.nonfinite_hs = d.active_cells = -1;
    if (what & CSI_DIAG_VELOCITY) {
        d.inv_timescale_max = slot[DQ_INV_TIMESCALE]; d.max_abs_u = slot[DQ_MAX_ABS_U]; d.max_abs_v = slot[DQ_MAX_ABS_V];
        d.nonfinite_u = as_count(slot[DQ_NONFINITE_U]); d.nonfinite_v = as_count(slot[DQ_NONFINITE_V]);
        d.nan_u = as_count(slot[DQ_NAN_U]); d.nan_v = as_count(slot[DQ_NAN_V]);
        d.advection_timescale = (d.nan_u + d.nan_v > 0) ? nan : 1.0 / d.inv_timescale_max;
    }
    if (what & CSI_DIAG_TRACERS) {
        d.ice_volume = slot[DQ_VOLUME]; d.ice_area = slot[DQ_AREA]; d.ice_extent = slot[DQ_EXTENT]; d.active_area = slot[DQ_ACTIVE_AREA];
        d.min_h = slot[DQ_MIN_H]; d.max_h = slot[DQ_MAX_H]; d.min_aice = slot[DQ_MIN_AICE]; d.max_aice = slot[DQ_MAX_AICE];
        d.nonfinite_h = as_count(slot[DQ_NONFINITE_H]); d.nonfinite_aice = as_count(slot[DQ_NONFINITE_AICE]);
        d.active_cells = as_count(slot[DQ_ACTIVE_CELLS]);
        if (d.has_snow) { d.snow_volume = slot[DQ_SNOW_VOLUME]; d.max_hs = slot[DQ_MAX_HS]; d.nonfinite_hs = as_count(slot[DQ_NONFINITE_HS]); }
    }
    *out = d;
    return CSI_OK;
}

}
