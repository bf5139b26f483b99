// csi_time_series.hip -- forcing time series interpolated at the model clock (include/csi.h: csi_time_series_plan / _set / _update /
// _status).  Stands where the reference's update_state! ends with update_model_field_time_series!(model, clock)
// (src/sea_ice_model.jl:391-408) and where its kernels index a FieldTimeSeries with Time(clock.time)
// (SeaIceThermodynamics/thermodynamic_time_step.jl:326-329): here every series-driven slot is interpolated once per update, in ONE
// launch (time_series.hip), IN PLACE into the bound array that the momentum / thermodynamic kernels already read -- to them a
// series-driven array is an array.
//
// DEVICE backend: all slices live in the caller's device array; nothing is copied.
// HOST backend: the slices live in the caller's host memory; the library keeps `window` of them in a device ring.
//   Residency is a slot table (ring slot -> slice), NOT slice mod window: the cyclical wrap pair (nt - 1, 0) would collide whenever
//   window divides nt - 1.  A slot is evicted only if neither current index uses it (an empty one first, else the least recently used).
//   Ordering: an upload runs on the library's copy stream; it first waits for `series_launched`, the event recorded on the context's
//   stream behind the newest interpolation launch (so behind the last one that read the slot); the interpolation launch waits for the
//   `uploaded` events of the slots it reads.  The slice the indexing rule needs NEXT (time moving forward) is uploaded into a free slot
//   under the step that follows: the update only notes it, and series_prefetch -- called at the end of the entry points that advance
//   the model, once their launches are queued, and by the next update or status call at the latest -- stages and copies it, so that
//   the host's staging copy, too, runs while the device is busy (measured: profiles/r13_time_series.md).  Pageable host memory is staged through one pinned slice per
//   ring slot, rewritten only after the copy that last read it has completed (the one place where the host may wait); page-locked host
//   memory is copied from directly.  Ring slices have the bound array's row stride and its interior's alignment modulo 16 bytes, so the
//   kernel's 16-byte accesses apply to every row.  Any time is legal: forward or backward jumps, a first call in the middle.
//
// REGRIDDED series (csi_regrid_map_create / csi_time_series_set_regridded; time_series_regrid.hip): a slot's series lives on a source
// grid of its own; its slices -- and so its ring slices -- have the SOURCE shape, packed (the kernel gathers single values from them).
// A slot is a scalar's series or the east and north series of a vector pair, each a TimeSeries like any other: describe_series,
// ring_init, ring_acquire, upload and the look-ahead are the same code for both kinds.  All regridded slots ride in ONE further launch.
#include "csi_ctx.h"

namespace csi_host {

static int find_series(const csi_context* c, int fid) {
    for (size_t k = 0; k < c->series.size(); ++k) if (c->series[k].fid == fid) return (int)k;
    return -1;
}

static int find_regrid(const csi_context* c, int fid) {
    for (size_t k = 0; k < c->regrid.size(); ++k) if (c->regrid[k].fid == fid) return (int)k;
    return -1;
}

bool series_drives(const csi_context* c, int fid) { return find_series(c, fid) >= 0 || find_regrid(c, fid) >= 0; }

static void series_free(TimeSeries& S) {
    for (TimeSeries::Slot& s : S.slots) if (s.uploaded) { hipEventDestroy(s.uploaded); s.uploaded = nullptr; }
    S.slots.clear();
}

// every TimeSeries of the context: the model-grid ones and the parts of the regridded slots
template <class F>
static int32_t each_series(csi_context* c, F f) {
    int32_t rc;
    for (TimeSeries& S : c->series) if ((rc = f(S))) return rc;
    for (RegridSeries& R : c->regrid)
        for (int q = 0; q < R.parts; ++q) if ((rc = f(R.part[q]))) return rc;
    return CSI_OK;
}

void series_release(csi_context* c) {
    if (c->series_stream) hipStreamSynchronize(c->series_stream);
    each_series(c, [](TimeSeries& S) { series_free(S); return CSI_OK; });
    c->series.clear();                   // (rings and staging slices: freed by their owners)
    c->regrid.clear();
    c->maps.clear();
    if (c->series_launched) { hipEventDestroy(c->series_launched); c->series_launched = nullptr; }
    if (c->series_stream) { hipStreamDestroy(c->series_stream); c->series_stream = nullptr; }
    c->series_launched_valid = false;
}

// largest n with times[n] <= t (times[0] <= t < times[nt - 1])
static int lower_node(const double* times, int nt, double t) {
    int lo = 0, hi = nt - 1;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (times[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

static void between(const double* times, int nt, double t, int* n1, int* n2, double* frac) {
    const int n = lower_node(times, nt, t);
    if (times[n] == t) { *n1 = *n2 = n; *frac = 0.0; return; }
    *n1 = n; *n2 = n + 1;
    *frac = (t - times[n]) / (times[n + 1] - times[n]);
}

static int32_t plan(const double* times, int nt, int indexing, double period, double t, int* n1, int* n2, double* frac) {
    if (!times || !n1 || !n2 || !frac || nt < 2 || !std::isfinite(t)) return CSI_ERR_INVALID_ARGUMENT;
    if (indexing != CSI_TIME_CLAMP && indexing != CSI_TIME_CYCLICAL && indexing != CSI_TIME_LINEAR) return CSI_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < nt; ++k)
        if (!std::isfinite(times[k]) || (k > 0 && !(times[k] > times[k - 1]))) return CSI_ERR_INVALID_ARGUMENT;
    const double first = times[0], last = times[nt - 1];
    if (indexing == CSI_TIME_CYCLICAL) {
        const double span = last - first;
        double P = period;
        if (!(P > 0.0)) P = span + (last - times[nt - 2]);
        else if (!(P > span) || !std::isfinite(P)) return CSI_ERR_INVALID_ARGUMENT;
        double r = std::fmod(t - first, P);
        if (r < 0.0) r += P;
        const double tp = first + r;
        if (tp > last) { *n1 = nt - 1; *n2 = 0; *frac = (tp - last) / (P - span); return CSI_OK; }
        if (tp == last) { *n1 = *n2 = nt - 1; *frac = 0.0; return CSI_OK; }
        if (tp <= first) { *n1 = *n2 = 0; *frac = 0.0; return CSI_OK; }
        between(times, nt, tp, n1, n2, frac);
        return CSI_OK;
    }
    if (t <= first || t >= last) {
        const bool low = t <= first;
        if (indexing == CSI_TIME_CLAMP || t == first || t == last) { *n1 = *n2 = low ? 0 : nt - 1; *frac = 0.0; return CSI_OK; }
        *n1 = low ? 0 : nt - 2; *n2 = *n1 + 1;            // LINEAR: extrapolate from the first / last two slices
        *frac = (t - times[*n1]) / (times[*n2] - times[*n1]);
        return CSI_OK;
    }
    between(times, nt, t, n1, n2, frac);
    return CSI_OK;
}

// the slice the indexing rule needs next when time moves forward (-1: none)
static int next_slice(const TimeSeries& S, int n1, int n2) {
    (void)n1;
    const int top = n2;                                      // the newer of the two (the wrap pair's is slice 0; n1 == n2: the slice itself)
    if (top + 1 < S.nt) return top + 1;
    return S.indexing == CSI_TIME_CYCLICAL ? 0 : -1;
}

static int resident_slot(const TimeSeries& S, int slice) {
    for (size_t k = 0; k < S.slots.size(); ++k) if (S.slots[k].slice == slice) return (int)k;
    return -1;
}

// a slot that holds neither keep1 nor keep2: an empty one first, else the least recently used (-1: none)
static int victim_slot(const TimeSeries& S, int keep1, int keep2) {
    int best = -1;
    for (size_t k = 0; k < S.slots.size(); ++k) {
        const TimeSeries::Slot& s = S.slots[k];
        if (s.slice >= 0 && (s.slice == keep1 || s.slice == keep2)) continue;
        if (s.slice < 0) return (int)k;
        if (best < 0 || s.used < S.slots[best].used) best = (int)k;
    }
    return best;
}

static double* ring_slice(const TimeSeries& S, int slot) { return S.ring.get() + S.ring_off + (int64_t)slot * S.ring_stride; }

// slice -> ring slot, on the copy stream, behind every interpolation launch issued so far
static int32_t upload(csi_context* c, TimeSeries& S, int slot, int slice) {
    TimeSeries::Slot& s = S.slots[slot];
    if (c->series_launched_valid) HIP_TRY(c, hipStreamWaitEvent(c->series_stream, c->series_launched, 0));
    const double* src = S.data + (int64_t)slice * S.slice_stride;
    size_t spitch = (size_t)S.ld * sizeof(double);
    if (!S.data_pinned) {
        double* st = S.stage.get() + (size_t)slot * S.nx * S.ny;
        if (s.staged) HIP_TRY(c, hipEventSynchronize(s.uploaded));       // the copy that last read this staging slice
        for (int j = 0; j < S.ny; ++j) memcpy(st + (size_t)j * S.nx, src + (int64_t)j * S.ld, (size_t)S.nx * sizeof(double));
        src = st;
        spitch = (size_t)S.nx * sizeof(double);
        s.staged = true;
    }
    HIP_TRY(c, hipMemcpy2DAsync(ring_slice(S, slot), (size_t)S.ring_ld * sizeof(double), src, spitch, (size_t)S.nx * sizeof(double), (size_t)S.ny,
                                hipMemcpyHostToDevice, c->series_stream));
    HIP_TRY(c, hipEventRecord(s.uploaded, c->series_stream));
    s.slice = slice;
    s.pending = true;
    ++S.uploads;
    return CSI_OK;
}

// ---- what csi_time_series_set and csi_time_series_set_regridded share ------------------------------------------------------------------
static int32_t slot_check(csi_context* c, int fid, bool setting) {
    if (!slot_has(fid, SLOT_SERIES)) {
        std::string names;
        for (int id : slots_with(SLOT_SERIES)) names += std::string(names.empty() ? "" : ", ") + slot_name(id);
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: the slot is not one a series may drive (" + names + ")");
    }
    if (setting && fid == CSI_F_BOTTOM_HEAT_FLUX && c->ml_set)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series on bottom_heat_flux: the mixed layer (csi_mixed_layer_set) writes that array at every step");
    return CSI_OK;
}

// remove the slot's series of either kind (replacing or removing one: whatever may still read its ring or staging slices has to finish first)
static int32_t slot_clear(csi_context* c, int fid) {
    const int old = find_series(c, fid), oldr = find_regrid(c, fid);
    if (old < 0 && oldr < 0) return CSI_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->series_stream) HIP_TRY(c, hipStreamSynchronize(c->series_stream));
    if (old >= 0) {
        series_free(c->series[old]);
        c->series.erase(c->series.begin() + old);
    }
    if (oldr >= 0) {
        for (int q = 0; q < c->regrid[oldr].parts; ++q) series_free(c->regrid[oldr].part[q]);
        c->regrid.erase(c->regrid.begin() + oldr);
    }
    return CSI_OK;
}

// the caller's description of a series whose slices are nx x ny (`shape`: what that is, for the message), validated
static int32_t describe_series(csi_context* c, TimeSeries& S, int fid, const csi_time_series* ts, int nx, int ny, const char* shape) {
    S.fid = fid;
    S.nt = ts->nt; S.indexing = ts->indexing; S.backend = ts->backend; S.period = ts->period;
    S.nx = nx; S.ny = ny;
    S.data = (const double*)ts->data; S.ld = ts->ld; S.slice_stride = ts->slice_stride;
    if (S.backend != CSI_SERIES_DEVICE && S.backend != CSI_SERIES_HOST) return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: unknown backend");
    if (!ts->times || !ts->data) return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: times and data must not be NULL");
    if (((uintptr_t)ts->data) & 7) return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: data must be 8-byte aligned");
    if (S.ld < S.nx || S.slice_stride < S.ld * (int64_t)(S.ny - 1) + S.nx)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("time series of ") + slot_name(fid) + ": ld / slice_stride too small for slices of " + shape);
    int n1, n2;
    double frac;
    if (ts->nt < 2 || plan(ts->times, ts->nt, ts->indexing, ts->period, ts->times[0], &n1, &n2, &frac))
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: nt >= 2, strictly increasing finite times, a known indexing kind and (CYCLICAL) a period longer "
                                                 "than the span of the times are required");
    S.times.assign(ts->times, ts->times + ts->nt);
    if (S.backend == CSI_SERIES_HOST) {
        S.window = ts->window == 0 ? 3 : ts->window;
        if (S.window < 2) return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: window >= 2 required (0: the default, 3)");
    }
    return CSI_OK;
}

// HOST backend: the device ring of S.window slices with rows ring_ld doubles apart and an even slice stride, its staging slices and
// slot events.  like != NULL: the first element gets that address's alignment modulo 16 bytes.
static int32_t ring_init(csi_context* c, TimeSeries& S, int64_t ring_ld, const double* like) {
    hipSetDevice(c->device);
    if (!c->series_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->series_stream, hipStreamNonBlocking));
    if (!c->series_launched) HIP_TRY(c, hipEventCreateWithFlags(&c->series_launched, hipEventDisableTiming));
    S.ring_ld = ring_ld;
    S.ring_stride = ((S.ring_ld * (int64_t)S.ny + 1) / 2) * 2 + 2;
    HIP_TRY(c, S.ring.alloc((size_t)(S.ring_stride * S.window + 2)));
    S.ring_off = (like && ((((uintptr_t)like) ^ ((uintptr_t)S.ring.get())) & 15)) ? 1 : 0;
    hipPointerAttribute_t at{};
    S.data_pinned = hipPointerGetAttributes(&at, S.data) == hipSuccess && at.type == hipMemoryTypeHost;
    (void)hipGetLastError();                               // (pageable memory: the query fails, which is the answer)
    if (!S.data_pinned) HIP_TRY(c, S.stage.alloc((size_t)S.window * S.nx * S.ny));
    S.slots.resize(S.window);
    for (TimeSeries::Slot& s : S.slots) {
        hipError_t e = hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming);
        if (e != hipSuccess) { series_free(S); return fail(c, CSI_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e)); }
    }
    return CSI_OK;
}

// ---- regridding maps ------------------------------------------------------------------------------------------------------------------
static const int kLocationField[3] = {CSI_F_U, CSI_F_V, CSI_F_H};      // a field at each csi_regrid_location

// which device layout of a map the rows of a bound array select: (the first interior row starts 8 bytes behind a 16-byte boundary) * 2
// + (the row stride is odd, so that this alternates from row to row)
static int regrid_variant(const double* dst, int64_t ld) { return (int)((((uintptr_t)dst) >> 3) & 1) * 2 + (int)(ld & 1); }

// pack the map's planes for one alignment pattern (csi_kernels.h RegridDesc) and copy them to the device; padding entries are zero
static int32_t map_upload(csi_context* c, RegridMap& M, int variant) {
    const int planes = M.rotation ? 5 : 3;
    std::vector<unsigned long long> host((size_t)M.plane * planes, 0ull);
    const double* src[4] = {M.wx.data(), M.wy.data(), M.cs.data(), M.sn.data()};
    for (int j = 0; j < M.ny; ++j) {
        const int head = ((variant >> 1) + (variant & 1) * j) & 1;
        unsigned long long* row = host.data() + (size_t)j * M.mld + head;
        memcpy(row, M.idx.data() + (size_t)j * M.nx, (size_t)M.nx * 8);
        for (int p = 1; p < planes; ++p) memcpy(row + (size_t)p * M.plane, src[p - 1] + (size_t)j * M.nx, (size_t)M.nx * 8);
    }
    HIP_TRY(c, M.dev[variant].alloc(host.size()));
    HIP_TRY(c, hipMemcpy(M.dev[variant].get(), host.data(), host.size() * 8, hipMemcpyHostToDevice));
    return CSI_OK;
}

// HOST backend: the ring slots that hold slices n1 and n2 (uploaded now if they are not resident), which the context's stream waits for
static int32_t ring_acquire(csi_context* c, TimeSeries& S, int n1, int n2, int slot[2]) {
    int32_t rc;
    const int want[2] = {n1, n2};
    for (int q = 0; q < (n1 == n2 ? 1 : 2); ++q) {
        slot[q] = resident_slot(S, want[q]);
        if (slot[q] < 0) {
            slot[q] = victim_slot(S, n1, n2);          // (window >= 2: there is one)
            if ((rc = upload(c, S, slot[q], want[q]))) return rc;
        }
        TimeSeries::Slot& s = S.slots[slot[q]];
        if (s.pending) { HIP_TRY(c, hipStreamWaitEvent(c->stream, s.uploaded, 0)); s.pending = false; }
        s.used = c->series_updates;
    }
    if (n1 == n2) slot[1] = slot[0];
    return CSI_OK;
}

// the two slices of S around time t (*a: psi_1, *b: psi_2), their row stride and weights; notes the pair and the slice wanted next
static int32_t series_at(csi_context* c, TimeSeries& S, double t, const double** a, const double** b, long* ld, double* w1, double* w2, int* same) {
    int n1, n2;
    double frac;
    int32_t rc;
    if ((rc = plan(S.times.data(), S.nt, S.indexing, S.period, t, &n1, &n2, &frac)))
        return fail(c, rc, std::string("time series of ") + slot_name(S.fid) + ": the time is not a finite number");
    *w2 = frac; *w1 = 1.0 - frac;
    *same = n1 == n2;
    if (S.backend == CSI_SERIES_DEVICE) {
        *a = S.data + (int64_t)n1 * S.slice_stride;
        *b = S.data + (int64_t)n2 * S.slice_stride;
        *ld = (long)S.ld;
    } else {
        int slot[2];
        if ((rc = ring_acquire(c, S, n1, n2, slot))) return rc;
        *a = ring_slice(S, slot[0]);
        *b = ring_slice(S, slot[1]);
        *ld = (long)S.ring_ld;
    }
    S.cur[0] = n1; S.cur[1] = n2;
    S.next = S.backend == CSI_SERIES_HOST ? next_slice(S, n1, n2) : -1;
    return CSI_OK;
}

static int32_t do_series_update(csi_context* c, double t) {
    if (c->series.empty() && c->regrid.empty()) return CSI_OK;
    ++c->series_updates;
    int32_t rc;
    if ((rc = series_prefetch(c))) return rc;                  // (a look-ahead nobody has issued yet: its victim was chosen for the OLD pair)
    if (!c->series.empty()) {
        SeriesTable T{};
        for (TimeSeries& S : c->series) {
            const Bound& b = c->f[S.fid];
            if (!b.p) return fail(c, CSI_ERR_NOT_BOUND, std::string("time series: field ") + slot_name(S.fid) + " is no longer bound");
            SeriesDesc& D = T.d[T.n];
            D.dst = b.p + c->Hx + (int64_t)c->Hy * b.ld;
            D.ldd = (long)b.ld;
            D.nx = S.nx; D.ny = S.ny;
            if (S.backend == CSI_SERIES_HOST && (b.ld != S.ring_ld || (((uintptr_t)D.dst ^ (uintptr_t)ring_slice(S, 0)) & 15)))
                return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("time series of ") + slot_name(S.fid) + ": the field was re-bound with another row stride or alignment; call csi_time_series_set again");
            if ((rc = series_at(c, S, t, &D.a, &D.b, &D.lda, &D.w1, &D.w2, &D.same))) return rc;
            D.ldb = D.lda;
            ++T.n;
        }
        launch_time_series(T, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    if (!c->regrid.empty()) {
        RegridTable T{};
        for (RegridSeries& R : c->regrid) {
            const Bound& b = c->f[R.fid];
            if (!b.p) return fail(c, CSI_ERR_NOT_BOUND, std::string("time series: field ") + slot_name(R.fid) + " is no longer bound");
            const RegridMap& M = c->maps[R.map];
            RegridDesc& D = T.d[T.n];
            D.dst = b.p + c->Hx + (int64_t)c->Hy * b.ld;
            D.ldd = (long)b.ld;
            if (b.ld != R.dst_ld || regrid_variant(D.dst, b.ld) != R.variant || b.ni - 2 * c->Hx != M.nx || b.nj - 2 * c->Hy != M.ny)
                return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("regridded time series of ") + slot_name(R.fid) + ": the field was re-bound with another shape, row stride or alignment; call csi_time_series_set_regridded again");
            D.nx = M.nx; D.ny = M.ny;
            D.map = M.dev[R.variant].get(); D.mld = (long)M.mld; D.plane = (long)M.plane;
            D.pair = R.parts == 2; D.component = R.component;
            for (int q = 0; q < R.parts; ++q)
                if ((rc = series_at(c, R.part[q], t, &D.a[q], &D.b[q], &D.lds[q], &D.w1[q], &D.w2[q], &D.same[q]))) return rc;
            ++T.n;
        }
        launch_time_series_regrid(T, c->stream);
        HIP_TRY(c, hipGetLastError());
        ++c->regrid_launches;
    }
    bool host = false;
    each_series(c, [&](TimeSeries& S) { host |= S.backend == CSI_SERIES_HOST; return CSI_OK; });
    if (!host) return CSI_OK;
    HIP_TRY(c, hipEventRecord(c->series_launched, c->stream));
    c->series_launched_valid = true;
    c->series_prefetch_pending = true;
    return CSI_OK;
}

// the slice each HOST series needs next, into a slot neither current index uses
int32_t series_prefetch(csi_context* c) {
    if (!c->series_prefetch_pending) return CSI_OK;
    c->series_prefetch_pending = false;
    return each_series(c, [&](TimeSeries& S) -> int32_t {
        if (S.backend != CSI_SERIES_HOST || S.next < 0 || resident_slot(S, S.next) >= 0) return CSI_OK;
        const int slot = victim_slot(S, S.cur[0], S.cur[1]);
        if (slot < 0) return CSI_OK;                           // window 2 with two current slices: no room to look ahead
        return upload(c, S, slot, S.next);
    });
}

}  // namespace csi_host

extern "C" {

int32_t csi_time_series_plan(const double* times, int32_t nt, int32_t indexing, double period, double t, int32_t* n1, int32_t* n2, double* frac) {
    int a = 0, b = 0;
    double f = 0.0;
    if (!n1 || !n2 || !frac) return CSI_ERR_INVALID_ARGUMENT;
    const int32_t rc = plan(times, nt, indexing, period, t, &a, &b, &f);
    if (rc) return rc;
    *n1 = a; *n2 = b; *frac = f;
    return CSI_OK;
}

int32_t csi_time_series_set(csi_context* c, int32_t fid, const csi_time_series* ts) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    int32_t rc;
    if ((rc = slot_check(c, fid, ts != nullptr)) || (rc = slot_clear(c, fid))) return rc;
    if (!ts) return CSI_OK;
    const Bound& b = c->f[fid];
    if (!c->grid_set || !b.p) return fail(c, CSI_ERR_NOT_BOUND, std::string("time series: bind field ") + slot_name(fid) + " first (the series writes into the bound array)");
    TimeSeries S;
    // the interior: field_size minus halos (a Face field on a Bounded side is one wider)
    if ((rc = describe_series(c, S, fid, ts, b.ni - 2 * c->Hx, b.nj - 2 * c->Hy, "the field's interior shape"))) return rc;
    // ring slices: the bound array's row stride and the interior's alignment modulo 16 bytes
    if (S.backend == CSI_SERIES_HOST && (rc = ring_init(c, S, b.ld, b.p + c->Hx + (int64_t)c->Hy * b.ld))) return rc;
    c->series.push_back(std::move(S));
    return CSI_OK;
}

int32_t csi_regrid_plan_axis(const double* nodes, int32_t n, int32_t periodic, double period, double x, int32_t* i0, int32_t* i1, double* w) {
    int a = 0, b = 0;
    double f = 0.0;
    if (!i0 || !i1 || !w) return CSI_ERR_INVALID_ARGUMENT;
    const int32_t rc = plan(nodes, n, periodic ? CSI_TIME_CYCLICAL : CSI_TIME_CLAMP, periodic ? period : 0.0, x, &a, &b, &f);
    if (rc) return rc;
    *i0 = a; *i1 = b; *w = f;
    return CSI_OK;
}

int32_t csi_regrid_map_create(csi_context* c, const csi_regrid_map* d, int32_t* map_id) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!d || !map_id) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regrid map: desc and map_id must not be NULL");
    if (!c->grid_set) return fail(c, CSI_ERR_NOT_BOUND, "regrid map: csi_grid_set has not been called");
    if (d->location < CSI_REGRID_FACE_CENTER || d->location > CSI_REGRID_CENTER_CENTER || d->reserved)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "regrid map: unknown location (reserved must be 0)");
    const int rep = kLocationField[d->location];
    const int nx = c->Nx + extra_x(c, rep), ny = c->Ny + extra_y(c, rep);
    if (d->nx != nx || d->ny != ny) {
        char buf[200];
        snprintf(buf, sizeof buf, "regrid map: target extents (%d, %d) are not the interior of a field at that location (%d, %d)", d->nx, d->ny, nx, ny);
        return fail(c, CSI_ERR_INVALID_ARGUMENT, buf);
    }
    if (d->src_nx < 2 || d->src_ny < 2 || d->src_nx > CSI_REGRID_MAX_SOURCE_EXTENT || d->src_ny > CSI_REGRID_MAX_SOURCE_EXTENT)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "regrid map: source extents beyond the layout's limit (2 .. 65536 per axis: the indices are stored as uint16)");
    if (!d->i0 || !d->i1 || !d->j0 || !d->j1 || !d->wx || !d->wy || (!d->cos != !d->sin))
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "regrid map: i0, i1, j0, j1, wx, wy must not be NULL; cos and sin come together");
    int id = -1;
    for (size_t k = 0; k < c->maps.size() && id < 0; ++k) if (!c->maps[k].live) id = (int)k;
    if (id < 0) {
        if ((int)c->maps.size() >= CSI_REGRID_MAX_MAPS) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regrid map: CSI_REGRID_MAX_MAPS maps are alive");
        c->maps.emplace_back();
        id = (int)c->maps.size() - 1;
    }
    RegridMap M;
    M.location = d->location; M.nx = nx; M.ny = ny; M.src_nx = d->src_nx; M.src_ny = d->src_ny;
    M.rotation = d->cos != nullptr;
    const size_t n = (size_t)nx * ny;
    M.idx.resize(n);
    for (size_t k = 0; k < n; ++k) {
        const int32_t i0 = d->i0[k], i1 = d->i1[k], j0 = d->j0[k], j1 = d->j1[k];
        if (i0 < 0 || i0 >= d->src_nx || i1 < 0 || i1 >= d->src_nx || j0 < 0 || j0 >= d->src_ny || j1 < 0 || j1 >= d->src_ny) {
            char buf[200];
            snprintf(buf, sizeof buf, "regrid map: index out of range at point (%d, %d): i0 %d, i1 %d, j0 %d, j1 %d, source %d x %d",
                     (int)(k % nx), (int)(k / nx), i0, i1, j0, j1, d->src_nx, d->src_ny);
            return fail(c, CSI_ERR_INVALID_ARGUMENT, buf);
        }
        if (!(d->wx[k] >= 0.0 && d->wx[k] <= 1.0) || !(d->wy[k] >= 0.0 && d->wy[k] <= 1.0)) {
            char buf[200];
            snprintf(buf, sizeof buf, "regrid map: weight outside [0, 1] at point (%d, %d): wx %g, wy %g", (int)(k % nx), (int)(k / nx), d->wx[k], d->wy[k]);
            return fail(c, CSI_ERR_INVALID_ARGUMENT, buf);
        }
        if (M.rotation && (!std::isfinite(d->cos[k]) || !std::isfinite(d->sin[k])))
            return fail(c, CSI_ERR_INVALID_ARGUMENT, "regrid map: cos and sin must be finite");
        M.idx[k] = (unsigned long long)i0 | ((unsigned long long)i1 << 16) | ((unsigned long long)j0 << 32) | ((unsigned long long)j1 << 48);
    }
    M.wx.assign(d->wx, d->wx + n); M.wy.assign(d->wy, d->wy + n);
    if (M.rotation) { M.cs.assign(d->cos, d->cos + n); M.sn.assign(d->sin, d->sin + n); }
    M.mld = (nx + 3) & ~1;                                      // even, and room for the leading and the trailing padding entry
    M.plane = M.mld * ny;
    M.live = true;
    c->maps[id] = std::move(M);
    *map_id = id;
    return CSI_OK;
}

int32_t csi_regrid_map_destroy(csi_context* c, int32_t map_id) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (map_id < 0 || map_id >= (int)c->maps.size() || !c->maps[map_id].live) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regrid map: unknown map");
    for (const RegridSeries& R : c->regrid)
        if (R.map == map_id) return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("regrid map: the series of ") + slot_name(R.fid) + " still uses the map");
    HIP_TRY(c, hipStreamSynchronize(c->stream));                // (a launch that read it may still run)
    c->maps[map_id] = RegridMap{};
    return CSI_OK;
}

int32_t csi_time_series_set_regridded(csi_context* c, int32_t fid, const csi_time_series* ts, int32_t map_id, const csi_time_series* other, int32_t component) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!ts) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regridded time series: ts must not be NULL (csi_time_series_set(ctx, slot, NULL) removes a series)");
    int32_t rc;
    if ((rc = slot_check(c, fid, true))) return rc;
    if (map_id < 0 || map_id >= (int)c->maps.size() || !c->maps[map_id].live) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regridded time series: unknown map");
    RegridMap& M = c->maps[map_id];
    const Bound& b = c->f[fid];
    if (!c->grid_set || !b.p) return fail(c, CSI_ERR_NOT_BOUND, std::string("time series: bind field ") + slot_name(fid) + " first (the series writes into the bound array)");
    if (slot_loc(fid, 0) != slot_loc(kLocationField[M.location], 0) || slot_loc(fid, 1) != slot_loc(kLocationField[M.location], 1) ||
        b.ni - 2 * c->Hx != M.nx || b.nj - 2 * c->Hy != M.ny)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("regridded time series of ") + slot_name(fid) + ": wrong location -- the map was made for another location (or another grid) than the slot's");
    if (component != 0 && component != 1) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regridded time series: component is 0 (x) or 1 (y)");
    if (!other && component != 0) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regridded time series: component without other -- a scalar series has component 0");
    if (other) {
        if (!M.rotation) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regridded time series: a vector pair needs a map with cos and sin");
        if (slot_loc(fid, 0) != (component == 0 ? LOC_F : LOC_C) || slot_loc(fid, 1) != (component == 0 ? LOC_C : LOC_F))
            return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("regridded time series of ") + slot_name(fid) + ": the x component of a pair drives a slot at (Face, Center), the y component one at (Center, Face)");
    }
    RegridSeries R;
    R.fid = fid; R.map = map_id; R.parts = other ? 2 : 1; R.component = component;
    const csi_time_series* src[2] = {ts, other};
    for (int q = 0; q < R.parts; ++q) {
        if ((rc = describe_series(c, R.part[q], fid, src[q], M.src_nx, M.src_ny, "the map's source shape"))) return rc;
        if (R.part[q].ld * (int64_t)M.src_ny > 0x7fffffff) return fail(c, CSI_ERR_INVALID_ARGUMENT, "regridded time series: a source slice of more than 2^31 doubles");
    }
    // the device layout of the map for the alignment pattern of the bound array's rows
    double* dst = b.p + c->Hx + (int64_t)c->Hy * b.ld;
    R.variant = regrid_variant(dst, b.ld);
    R.dst_ld = b.ld;
    hipSetDevice(c->device);
    if (!M.dev[R.variant] && (rc = map_upload(c, M, R.variant))) return rc;
    if ((rc = slot_clear(c, fid))) return rc;
    // ring slices of source shape, packed: the kernel gathers single values
    for (int q = 0; q < R.parts; ++q)
        if (R.part[q].backend == CSI_SERIES_HOST && (rc = ring_init(c, R.part[q], M.src_nx, nullptr))) {
            for (int p = 0; p < q; ++p) series_free(R.part[p]);
            return rc;
        }
    c->regrid.push_back(std::move(R));
    return CSI_OK;
}

int32_t csi_regrid_stats(csi_context* c, int64_t* launches, int32_t* maps) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (launches) *launches = c->regrid_launches;
    if (maps) { *maps = 0; for (const RegridMap& M : c->maps) *maps += M.live ? 1 : 0; }
    return CSI_OK;
}

int32_t csi_time_series_update(csi_context* c, double time) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    return do_series_update(c, time);
}

int32_t csi_time_series_status(csi_context* c, int32_t fid, int32_t* resident, int64_t* uploads) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    const int k = find_series(c, fid), r = find_regrid(c, fid);
    if (k < 0 && r < 0) return fail(c, CSI_ERR_NOT_BOUND, "time series: no series is set on this slot");
    int32_t rc = series_prefetch(c);
    if (rc) return rc;
    const TimeSeries& S = k >= 0 ? c->series[k] : c->regrid[r].part[0];      // (a pair: the east series)
    if (resident) for (size_t q = 0; q < S.slots.size(); ++q) resident[q] = S.slots[q].slice;
    if (uploads) *uploads = S.uploads;
    return CSI_OK;
}

}
