// csi_regions.hip -- csi_regions_compute, csi_regions_layout, csi_regions_stats (include/csi.h): the diagnostics' tracer group per region of
// a caller-supplied id map.  Stands where users of the reference copy h, aice, hs and the metrics to the host and bin them there.
// The kernels and the record layout: regions.hip, csi_kernels.h RegionsDev; the summation order: ordered_reduce.h.
//
// Host side: argument and binding checks by name, the two launches and ONE copy of the result slots into page-locked memory on the
// context's stream, ONE wait; on a tiled context the all-gather of every rank's slots and their combine in rank order (reduce_ranks,
// csi_diagnostics.hip).  The map is the caller's and arrives with every call: the library keeps none.  The partial buffer and the
// page-locked result are the context's, made at the first call; the partial buffer only grows.
#include "csi_ctx.h"
#include "ordered_reduce.h"

namespace csi_host {

static_assert(CSI_REGIONS_MAX == kRegionsMax, "include/csi.h and csi_kernels.h state one limit");
static_assert(sizeof(csi_region_record) == sizeof(double) * RQ_COUNT, "a record is its RQ_COUNT slots, in slot order");
constexpr int kRegionSlotsMax = 1 + kRegionsMax * RQ_COUNT;      // what travels between ranks: the count of the cells of no region, then the records

static void regions_sizes(int Nx, int Ny, int n, int64_t* records, int64_t* bytes) {
    int nbx, nby;
    red::diag_geometry(Nx, Ny, &nbx, &nby);
    *records = (int64_t)nbx * nby;
    *bytes = *records * (int64_t)(n + 1) * RQ_COUNT * (int64_t)sizeof(double);
}

// slots[0]: the cells of no region (a count); slots[1 + r * RQ_COUNT + q]: slot q of region r
static int32_t regions_local(csi_context* c, const csi_regions* r, double thr, double* slots) {
    if (!r) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regions: the csi_regions pointer is NULL");
    if (!r->ids) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regions: ids == NULL");
    if (r->n_regions < 1 || r->n_regions > CSI_REGIONS_MAX) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regions: n_regions must be between 1 and CSI_REGIONS_MAX (64); call again with another map for more");
    if (r->reserved != 0) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regions: reserved must be 0");
    if (!std::isfinite(thr) || thr < 0.0) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regions: extent_threshold must be finite and >= 0");
    if (!c->grid_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_grid_set has not been called");
    if (r->ld < c->Nx + 2 * c->Hx) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regions: ld < Nx + 2 Hx (the map is laid out like a (c,c) parent)");
    if (int32_t rc = need_named(c, "regions", "every call ", {CSI_F_H, CSI_F_A}, "")) return rc;
    const int n = r->n_regions;
    RegionsDev D{};
    D.g = c->g;
    D.h = ref_of(c, CSI_F_H); D.a = ref_of(c, CSI_F_A); D.hs = ref_of(c, CSI_F_HS);
    D.has_hs = c->f[CSI_F_HS].p != nullptr;
    D.ids = origin_of(c, r->ids, r->ld);
    D.ids_ld = (long)r->ld;
    D.n_regions = n;
    D.threshold = thr;
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t records, bytes;
    regions_sizes(c->Nx, c->Ny, n, &records, &bytes);
    const size_t nslots = (size_t)(n + 1) * RQ_COUNT;
    const size_t want = (size_t)bytes / sizeof(double) + nslots;      // the records, then the folded slots
    if (c->regions_part.size() < want) HIP_TRY(c, c->regions_part.ensure(want, c->stream, false));
    if (!c->regions_host) HIP_TRY(c, c->regions_host.alloc((size_t)(kRegionsMax + 1) * RQ_COUNT, hipHostMallocDefault));
    D.part = c->regions_part.get();
    D.nrec = (long)records;
    double* result = D.part + (size_t)records * nslots;
    launch_regions(D, result, c->stream);
    c->region_launches += 2;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->regions_host.get(), result, sizeof(double) * nslots, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double* got = c->regions_host.get();
    slots[0] = got[(size_t)n * RQ_COUNT + RQ_CELLS];
    memcpy(slots + 1, got, sizeof(double) * (size_t)n * RQ_COUNT);
    return CSI_OK;
}

static int64_t bits_of(double slot) { int64_t n; memcpy(&n, &slot, sizeof n); return n; }
static double regions_combine(int q, double a, double b) {
    switch (q == 0 ? K_CNT : RegionKinds::kind((q - 1) % RQ_COUNT)) {
        case K_SUM: return a + b;
        case K_MAX: return std::fmax(a, b);
        case K_MIN: return std::fmin(a, b);
        default: { const int64_t n = bits_of(a) + bits_of(b); double d; memcpy(&d, &n, sizeof d); return d; }
    }
}

}  // namespace csi_host

extern "C" {

int32_t csi_regions_layout(int32_t Nx, int32_t Ny, int32_t n_regions, int64_t* records, int64_t* bytes) {
    if (Nx < 1 || Ny < 1 || n_regions < 1 || n_regions > CSI_REGIONS_MAX) return CSI_ERR_INVALID_ARGUMENT;
    int64_t r, b;
    csi_host::regions_sizes(Nx, Ny, n_regions, &r, &b);
    if (records) *records = r;
    if (bytes) *bytes = b;
    return CSI_OK;
}

int32_t csi_regions_compute(csi_context* c, const csi_regions* r, double extent_threshold, csi_region_record* out, int64_t* unassigned_cells) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regions: out == NULL");
    double slot[kRegionSlotsMax] = {};
    int32_t rc = peer_check_entry(c);
    if (!rc) rc = regions_local(c, r, extent_threshold, slot);
    // (a rank that has failed locally still enters the gather: its status word comes first in the payload, so every rank fails)
    const int n = (r && r->n_regions >= 1 && r->n_regions <= CSI_REGIONS_MAX) ? r->n_regions : 1;
    const int nslots = 1 + n * RQ_COUNT;
    if ((rc = reduce_ranks(c, "regions", rc, nslots, 0, nslots, regions_combine, slot))) return rc;
    const bool snow = c->f[CSI_F_HS].p != nullptr;
    const double nan = std::nan("");
    for (int k = 0; k < n; ++k) {
        const double* s = slot + 1 + k * RQ_COUNT;
        csi_region_record d{};
        d.ice_volume = s[RQ_VOLUME]; d.ice_area = s[RQ_AREA]; d.ice_extent = s[RQ_EXTENT]; d.region_area = s[RQ_REGION_AREA];
        d.snow_volume = snow ? s[RQ_SNOW_VOLUME] : nan;
        d.min_h = s[RQ_MIN_H]; d.max_h = s[RQ_MAX_H]; d.min_aice = s[RQ_MIN_AICE]; d.max_aice = s[RQ_MAX_AICE];
        d.max_hs = snow ? s[RQ_MAX_HS] : nan;
        d.cells = bits_of(s[RQ_CELLS]);
        out[k] = d;
    }
    if (unassigned_cells) *unassigned_cells = bits_of(slot[0]);
    return CSI_OK;
}

int32_t csi_regions_stats(csi_context* c, int64_t* launches) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (launches) *launches = c->region_launches;
    return CSI_OK;
}

}
