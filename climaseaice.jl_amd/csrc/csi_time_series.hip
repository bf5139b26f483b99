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
#include "csi_ctx.h"

namespace csi_host {

static bool series_slot(int fid) {
    for (int id : kForcingFields) if (fid == id) return true;
    return fid == CSI_F_TOP_HEAT_FLUX || fid == CSI_F_BOTTOM_HEAT_FLUX || fid == CSI_F_SNOWFALL || fid == CSI_F_FLUX_COEFFICIENT ||
           fid == CSI_F_FLUX_REFERENCE_TEMPERATURE || fid == CSI_F_BOTTOM_SALINITY || fid == CSI_F_ML_SURFACE_HEAT_FLUX ||
           fid == CSI_F_ML_COEFFICIENT || fid == CSI_F_ML_REFERENCE_TEMPERATURE || fid == CSI_F_ML_DEEP_HEAT_FLUX ||
           fid == CSI_F_SHORTWAVE;
}

static int find_series(const csi_context* c, int fid) {
    for (size_t k = 0; k < c->series.size(); ++k) if (c->series[k].fid == fid) return (int)k;
    return -1;
}

static void series_free(TimeSeries& S) {
    for (TimeSeries::Slot& s : S.slots) if (s.uploaded) { hipEventDestroy(s.uploaded); s.uploaded = nullptr; }
    S.slots.clear();
}

void series_release(csi_context* c) {
    if (c->series_stream) hipStreamSynchronize(c->series_stream);
    for (TimeSeries& S : c->series) series_free(S);
    c->series.clear();                   // (rings and staging slices: freed by their owners)
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

static int32_t do_series_update(csi_context* c, double t) {
    if (c->series.empty()) return CSI_OK;
    ++c->series_updates;
    SeriesTable T{};
    int32_t rc;
    if ((rc = series_prefetch(c))) return rc;                  // (a look-ahead nobody has issued yet: its victim was chosen for the OLD pair)
    for (TimeSeries& S : c->series) {
        const Bound& b = c->f[S.fid];
        if (!b.p) return fail(c, CSI_ERR_NOT_BOUND, std::string("time series: field ") + kName[S.fid] + " is no longer bound");
        int n1, n2;
        double frac;
        if ((rc = plan(S.times.data(), S.nt, S.indexing, S.period, t, &n1, &n2, &frac)))
            return fail(c, rc, std::string("time series of ") + kName[S.fid] + ": the time is not a finite number");
        SeriesDesc& D = T.d[T.n];
        D.dst = b.p + c->Hx + (int64_t)c->Hy * b.ld;
        D.ldd = (long)b.ld;
        D.nx = S.nx; D.ny = S.ny;
        D.w2 = frac; D.w1 = 1.0 - frac;
        D.same = n1 == n2;
        if (S.backend == CSI_SERIES_DEVICE) {
            D.a = S.data + (int64_t)n1 * S.slice_stride;
            D.b = S.data + (int64_t)n2 * S.slice_stride;
            D.lda = D.ldb = (long)S.ld;
        } else {
            if (b.ld != S.ring_ld || (((uintptr_t)D.dst ^ (uintptr_t)ring_slice(S, 0)) & 15))
                return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("time series of ") + kName[S.fid] + ": the field was re-bound with another row stride or alignment; call csi_time_series_set again");
            int slot[2];
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
            D.a = ring_slice(S, slot[0]);
            D.b = ring_slice(S, slot[1]);
            D.lda = D.ldb = (long)S.ring_ld;
        }
        S.cur[0] = n1; S.cur[1] = n2;
        S.next = S.backend == CSI_SERIES_HOST ? next_slice(S, n1, n2) : -1;
        ++T.n;
    }
    launch_time_series(T, c->stream);
    HIP_TRY(c, hipGetLastError());
    bool host = false;
    for (const TimeSeries& S : c->series) host |= S.backend == CSI_SERIES_HOST;
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
    int32_t rc;
    for (TimeSeries& S : c->series) {
        if (S.backend != CSI_SERIES_HOST || S.next < 0 || resident_slot(S, S.next) >= 0) continue;
        const int slot = victim_slot(S, S.cur[0], S.cur[1]);
        if (slot < 0) continue;                                // window 2 with two current slices: no room to look ahead
        if ((rc = upload(c, S, slot, S.next))) return rc;
    }
    return CSI_OK;
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
    if (fid < 0 || fid >= CSI_F_COUNT_SHORTWAVE || !series_slot(fid))
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: the slot is not one of the eleven forcing slots (stress / external-velocity arrays, model.forcing, "
                                                 "free-drift fields, top / bottom heat flux, snowfall) nor one of the eight per-cell inputs that joined them: the LinearHeatFlux "
                                                 "coefficient and reference temperature, the bottom salinity, the mixed layer's four inputs, the shortwave flux");
    if (ts && fid == CSI_F_BOTTOM_HEAT_FLUX && c->ml_set)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series on bottom_heat_flux: the mixed layer (csi_mixed_layer_set) writes that array at every step");
    // (replacing or removing a series: whatever may still read its ring or staging slices has to finish first)
    const int old = find_series(c, fid);
    if (old >= 0) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (c->series_stream) HIP_TRY(c, hipStreamSynchronize(c->series_stream));
        series_free(c->series[old]);
        c->series.erase(c->series.begin() + old);
    }
    if (!ts) return CSI_OK;
    const Bound& b = c->f[fid];
    if (!c->grid_set || !b.p) return fail(c, CSI_ERR_NOT_BOUND, std::string("time series: bind field ") + kName[fid] + " first (the series writes into the bound array)");
    TimeSeries S;
    S.fid = fid;
    S.nt = ts->nt; S.indexing = ts->indexing; S.backend = ts->backend; S.period = ts->period;
    S.nx = b.ni - 2 * c->Hx; S.ny = b.nj - 2 * c->Hy;          // the interior: field_size minus halos (a Face field on a Bounded side is one wider)
    S.data = (const double*)ts->data; S.ld = ts->ld; S.slice_stride = ts->slice_stride;
    if (S.backend != CSI_SERIES_DEVICE && S.backend != CSI_SERIES_HOST) return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: unknown backend");
    if (!ts->times || !ts->data) return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: times and data must not be NULL");
    if (((uintptr_t)ts->data) & 7) return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: data must be 8-byte aligned");
    if (S.ld < S.nx || S.slice_stride < S.ld * (int64_t)(S.ny - 1) + S.nx)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("time series of ") + kName[fid] + ": ld / slice_stride too small for slices of the field's interior shape");
    {
        int n1, n2;
        double frac;
        if (ts->nt < 2 || plan(ts->times, ts->nt, ts->indexing, ts->period, ts->times[0], &n1, &n2, &frac))
            return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: nt >= 2, strictly increasing finite times, a known indexing kind and (CYCLICAL) a period longer "
                                                     "than the span of the times are required");
    }
    S.times.assign(ts->times, ts->times + ts->nt);
    if (S.backend == CSI_SERIES_HOST) {
        S.window = ts->window == 0 ? 3 : ts->window;
        if (S.window < 2) return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series: window >= 2 required (0: the default, 3)");
        hipSetDevice(c->device);
        if (!c->series_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->series_stream, hipStreamNonBlocking));
        if (!c->series_launched) HIP_TRY(c, hipEventCreateWithFlags(&c->series_launched, hipEventDisableTiming));
        // ring slices: the bound array's row stride, an even slice stride and the interior's alignment modulo 16 bytes
        S.ring_ld = b.ld;
        S.ring_stride = ((S.ring_ld * (int64_t)S.ny + 1) / 2) * 2 + 2;
        HIP_TRY(c, S.ring.alloc((size_t)(S.ring_stride * S.window + 2)));
        const double* dst = b.p + c->Hx + (int64_t)c->Hy * b.ld;
        S.ring_off = ((((uintptr_t)dst) ^ ((uintptr_t)S.ring.get())) & 15) ? 1 : 0;
        hipPointerAttribute_t at{};
        S.data_pinned = hipPointerGetAttributes(&at, ts->data) == hipSuccess && at.type == hipMemoryTypeHost;
        (void)hipGetLastError();                               // (pageable memory: the query fails, which is the answer)
        if (!S.data_pinned) HIP_TRY(c, S.stage.alloc((size_t)S.window * S.nx * S.ny));
        S.slots.resize(S.window);
        for (TimeSeries::Slot& s : S.slots) {
            hipError_t e = hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming);
            if (e != hipSuccess) { series_free(S); return fail(c, CSI_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e)); }
        }
    }
    c->series.push_back(std::move(S));
    return CSI_OK;
}

int32_t csi_time_series_update(csi_context* c, double time) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    return do_series_update(c, time);
}

int32_t csi_time_series_status(csi_context* c, int32_t fid, int32_t* resident, int64_t* uploads) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    const int k = find_series(c, fid);
    if (k < 0) return fail(c, CSI_ERR_NOT_BOUND, "time series: no series is set on this slot");
    int32_t rc = series_prefetch(c);
    if (rc) return rc;
    const TimeSeries& S = c->series[k];
    if (resident) for (size_t q = 0; q < S.slots.size(); ++q) resident[q] = S.slots[q].slice;
    if (uploads) *uploads = S.uploads;
    return CSI_OK;
}

}
