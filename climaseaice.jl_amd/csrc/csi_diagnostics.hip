// csi_diagnostics.hip -- csi_diagnostics_compute (include/csi.h): scalars computed from the bound fields on the device.
// Stands where the reference's root module has cell_advection_timescale(model::SeaIceModel) (src/ClimaSeaIce.jl:63-69) and where its
// tests and validation scripts reduce whole fields on the host.  The kernels and the summation order: diagnostics.hip.
//
// Host side: argument and binding checks, then the host path of every ordered reduction, stated here once (csi_ctx.h reduce_begin / reduce_end,
// reduce_ranks; csi_budget_compute and csi_momentum_budget_compute use it too): the two launches and the copy of the result slots
// into page-locked memory on the context's stream, ONE wait for that stream; on a tiled context the all-gather of every rank's slots
// and their combine in rank order.
#include "csi_ctx.h"
#include "ordered_reduce.h"

namespace csi_host {

static_assert(DQ_COUNT >= BQ_COUNT && DQ_COUNT >= MQ_COUNT, "the reduction buffers are sized for the diagnostics' slot count");

int32_t need_named(csi_context* c, const char* who, const char* group, std::initializer_list<int> ids, const char* hint) {
    for (int id : ids)
        if (!c->f[id].p) return fail(c, CSI_ERR_NOT_BOUND, std::string(who) + ": " + group + "needs field " + slot_name(id) + " (not bound" + hint + ")");
    return CSI_OK;
}

int32_t reduce_begin(csi_context* c, double** part, long* nrec, double** result) {
    HIP_TRY(c, hipSetDevice(c->device));
    int nbx, nby;
    red::diag_geometry(c->Nx, c->Ny, &nbx, &nby);
    *nrec = (long)nbx * nby;
    HIP_TRY(c, c->reduce_part.ensure((size_t)(*nrec + 1) * DQ_COUNT, c->stream, false));
    if (!c->reduce_host) HIP_TRY(c, c->reduce_host.alloc(DQ_COUNT, hipHostMallocDefault));
    *part = c->reduce_part.get();
    *result = *part + (size_t)*nrec * DQ_COUNT;
    return CSI_OK;
}

int32_t reduce_end(csi_context* c, int n, const double* result, double* slots) {
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->reduce_host.get(), result, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(slots, c->reduce_host.get(), sizeof(double) * n);
    return CSI_OK;
}

int32_t reduce_ranks(csi_context* c, const char* who, int32_t rc, int n, int q0, int q1, double (*combine)(int q, double a, double b), double* slots) {
    if (!has_comm(c)) return rc;
    // a rank's payload: the status word, then its n slots
    const size_t nb = sizeof(int64_t) + sizeof(double) * n;
    std::vector<uint8_t> mine(nb), all;
    const int64_t status = rc;
    memcpy(mine.data(), &status, sizeof status);
    memcpy(mine.data() + sizeof status, slots, sizeof(double) * n);
    const std::string local_err = c->err;
    const int32_t grc = comm_allgather(c, mine.data(), nb, all);
    if (rc) { c->err = local_err; return rc; }
    if (grc) return grc;
    std::vector<double> theirs(n);
    for (int r = 0; r < c->world; ++r) {
        int64_t st;
        memcpy(&st, all.data() + (size_t)r * nb, sizeof st);
        memcpy(theirs.data(), all.data() + (size_t)r * nb + sizeof st, sizeof(double) * n);
        if (st) return fail(c, CSI_ERR_COMM, std::string(who) + ": rank " + std::to_string(r) + " of the decomposition failed locally (status " + std::to_string((long)st) + ")");
        for (int q = q0; q < q1; ++q) slots[q] = r == 0 ? theirs[q] : (combine ? combine(q, slots[q], theirs[q]) : slots[q] + theirs[q]);
    }
    return CSI_OK;
}

static int32_t diag_local(csi_context* c, int32_t what, double thr, double* slots) {
    if (what == 0 || (what & ~CSI_DIAG_ALL)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "diagnostics: `what` must be a non-empty mask of CSI_DIAG_VELOCITY (1) and CSI_DIAG_TRACERS (2); unknown bit");
    if (!std::isfinite(thr) || thr < 0.0) return fail(c, CSI_ERR_INVALID_ARGUMENT, "diagnostics: extent_threshold must be finite and >= 0");
    if (!c->grid_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_grid_set has not been called");
    const bool vel = what & CSI_DIAG_VELOCITY, trc = what & CSI_DIAG_TRACERS;
    if (vel)
        for (int id : {CSI_F_U, CSI_F_V})
            if (!c->f[id].p) return fail(c, CSI_ERR_NOT_BOUND, std::string("diagnostics: the velocity group needs field ") + slot_name(id) + " (not bound: a model without dynamics supports CSI_DIAG_TRACERS only)");
    if (trc)
        for (int id : {CSI_F_H, CSI_F_A})
            if (!c->f[id].p) return fail(c, CSI_ERR_NOT_BOUND, std::string("diagnostics: the tracer group needs field ") + slot_name(id) + " (not bound)");
    DiagDev D{};
    D.g = c->g;
    D.u = ref_of(c, CSI_F_U); D.v = ref_of(c, CSI_F_V); D.h = ref_of(c, CSI_F_H); D.a = ref_of(c, CSI_F_A); D.hs = ref_of(c, CSI_F_HS);
    D.has_hs = c->f[CSI_F_HS].p != nullptr;
    D.exu = extra_x(c, CSI_F_U); D.eyv = extra_y(c, CSI_F_V);
    // the kernel reads u up to column Nx + exu and v up to row Ny + eyv: what csi_field_bind has checked the parents against
    if (vel && (c->f[CSI_F_U].ni < c->Nx + 2 * c->Hx + D.exu || c->f[CSI_F_V].nj < c->Ny + 2 * c->Hy + D.eyv))
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "diagnostics: u / v parents are smaller than the grid's Face fields");
    D.threshold = thr;
    double* result;
    int32_t rc = reduce_begin(c, &D.part, &D.nrec, &result);
    if (rc) return rc;
    launch_diagnostics(D, vel, trc, result, c->stream);
    return reduce_end(c, DQ_COUNT, result, slots);
}

static int64_t as_count(double slot) { int64_t n; memcpy(&n, &slot, sizeof n); return n; }
static double from_count(int64_t n) { double d; memcpy(&d, &n, sizeof d); return d; }
static double diag_combine(int q, double a, double b) {
    switch (DiagKinds::kind(q)) {
        case K_SUM: return a + b;
        case K_MAX: return std::fmax(a, b);
        case K_MIN: return std::fmin(a, b);
        default: return from_count(as_count(a) + as_count(b));
    }
}

}  // namespace csi_host

extern "C" {

int32_t csi_diagnostics_compute(csi_context* c, int32_t what, double extent_threshold, csi_diagnostics* out) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, CSI_ERR_INVALID_ARGUMENT, "diagnostics: out == NULL");
    double slot[DQ_COUNT] = {};
    int32_t rc = peer_check_entry(c);
    if (!rc) rc = diag_local(c, what, extent_threshold, slot);
    const int q0 = (what & CSI_DIAG_VELOCITY) ? 0 : DQ_VOLUME, q1 = (what & CSI_DIAG_TRACERS) ? DQ_COUNT : DQ_VOLUME;
    if ((rc = reduce_ranks(c, "diagnostics", rc, DQ_COUNT, q0, q1, diag_combine, slot))) return rc;
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
