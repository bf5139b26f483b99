// csi_output.hip -- device-side output (include/csi.h: csi_output_*).  Stands where the reference attaches an output writer to a
// Simulation (examples/ice_advected_by_anticyclone.jl:161-163, test/distributed_tests_utils.jl:159).  The kernels: output.hip.
//
// Host side: output sets (field list, record layout, accumulators, staging slots), the copy stream and the slot events.
//   snapshot:  pack launch on the context's stream -> event `packed[slot]` -> the copy stream waits for it -> ONE device-to-host copy of
//              the record into the slot's page-locked buffer -> event `done[slot]`.  No call here waits for the device except
//              csi_output_wait (for done[slot] only) and csi_output_destroy.
//   A slot is free -> in flight at snapshot and in flight -> free at release; the pack launch into a slot therefore follows the
//   release, hence the wait, of the previous copy out of it: nothing else orders the two.
//   A set remembers what its fields were bound to; another binding, or a new grid, makes every later call on it fail.
#include "csi_ctx.h"

namespace csi_host {

static int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }

static int32_t plan_layout(const int32_t* nx, const int32_t* ny, const int32_t* dtype, int n, int64_t* off, int64_t* bytes) {
    if (!nx || !ny || !dtype || n < 1 || n > CSI_OUTPUT_MAX_FIELDS) return CSI_ERR_INVALID_ARGUMENT;
    int64_t at = 0;
    for (int k = 0; k < n; ++k) {
        if (nx[k] < 1 || ny[k] < 1 || (dtype[k] != CSI_OUT_F64 && dtype[k] != CSI_OUT_F32)) return CSI_ERR_INVALID_ARGUMENT;
        if (off) off[k] = at;
        at = round256(at + (int64_t)nx[k] * ny[k] * (dtype[k] == CSI_OUT_F32 ? 4 : 8));
    }
    if (bytes) *bytes = at;
    return CSI_OK;
}

static void set_free(OutputSet& S) {
    for (hipEvent_t e : S.packed) if (e) hipEventDestroy(e);
    for (hipEvent_t e : S.done) if (e) hipEventDestroy(e);
    S.packed.clear(); S.done.clear(); S.in_flight.clear();
    S.acc.release(); S.stage.release(); S.host.release();
    S.live = false; S.W = 0.0; S.n = S.slots = 0;
}

void output_release(csi_context* c) {
    if (c->out_stream) hipStreamSynchronize(c->out_stream);
    for (OutputSet& S : c->out_sets) if (S.live) set_free(S);
    if (c->out_stream) { hipStreamDestroy(c->out_stream); c->out_stream = nullptr; }
}

// A field of a set: a slot, or CSI_TRACER_FIELD(k) once tracers are set (a (Center, Center) array of h's shape; csi_tracers.hip).  Its
// binding now, its name in messages, whether the id names anything, and whether it is a (Center, Center) field.
static Bound out_bound(const csi_context* c, int32_t id) { int k; return tracer_field_id(id, &k) ? tracer_bound(c, k) : c->f[id]; }
static std::string out_name(int32_t id) { int k; return tracer_field_id(id, &k) ? "tracer " + std::to_string(k) : std::string(slot_name(id)); }
static bool out_known(int32_t id) { int k; return tracer_field_id(id, &k) || slot_known(id); }
static bool out_center(int32_t id) { int k; return tracer_field_id(id, &k) || (slot_loc(id, 0) == LOC_C && slot_loc(id, 1) == LOC_C); }

// the set of a handle (null + error: a bad handle); `check`: also refuse a set whose fields or grid have changed since it was made
static OutputSet* set_of(csi_context* c, int32_t handle, bool check = true) {
    if (handle < 1 || handle > kMaxOutputSets || !c->out_sets[handle - 1].live) {
        fail(c, CSI_ERR_INVALID_ARGUMENT, "output: bad handle (not a live output set of this context)");
        return nullptr;
    }
    OutputSet* S = &c->out_sets[handle - 1];
    if (!check) return S;
    if (S->grid_gen != c->grid_gen) {
        fail(c, CSI_ERR_INVALID_ARGUMENT, "output: csi_grid_set was called after csi_output_create -- the set is invalid; destroy it and create it again");
        return nullptr;
    }
    for (int k = 0; k < S->n; ++k) {
        const Bound b = out_bound(c, S->f[k].field_id);
        const Bound& s = S->sig[k];
        if (b.p != s.p || b.ld != s.ld || b.ni != s.ni || b.nj != s.nj) {
            fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("output: field ") + out_name(S->f[k].field_id) +
                                                  " was re-bound after csi_output_create -- the set is invalid; destroy it and create it again");
            return nullptr;
        }
    }
    return S;
}

static int32_t slot_check(csi_context* c, const OutputSet* S, int32_t slot) {
    if (slot < 0 || slot >= S->slots) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: slot out of range");
    if (!S->in_flight[slot]) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: slot " + std::to_string(slot) + " is not in flight (no snapshot since its release)");
    return CSI_OK;
}

static OutputDesc desc_of(const csi_context* c, const OutputSet& S, int k, uint8_t* record) {
    const Bound& b = S.sig[k];
    OutputDesc D{};
    D.src = b.p + c->Hx + (int64_t)c->Hy * b.ld;
    D.lds = (long)b.ld;
    D.acc = S.f[k].averaged ? S.acc.get() + S.acc_off[k] : nullptr;
    D.dst = record ? record + S.off[k] : nullptr;
    D.nx = S.nx[k]; D.ny = S.ny[k];
    D.f32 = S.f[k].dtype == CSI_OUT_F32;
    D.averaged = S.f[k].averaged != 0;
    D.masked = S.f[k].masked != 0;
    D.fill = S.f[k].fill_value;
    return D;
}

}  // namespace csi_host

extern "C" {

int32_t csi_output_plan_layout(const int32_t* nx, const int32_t* ny, const int32_t* dtype, int32_t n, int64_t* byte_offsets, int64_t* record_bytes) {
    return plan_layout(nx, ny, dtype, n, byte_offsets, record_bytes);
}

int32_t csi_output_create(csi_context* c, const csi_output_field* fields, int32_t n, int32_t slots, int32_t* handle) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!fields || !handle) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: fields and handle must not be NULL");
    if (n < 1 || n > CSI_OUTPUT_MAX_FIELDS) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: n must be 1 .. 16 fields");
    if (slots < 1 || slots > CSI_OUTPUT_MAX_SLOTS) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: slots must be 1 .. 64");
    if (!c->grid_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_grid_set has not been called");
    int32_t nx[kMaxOutputFields], ny[kMaxOutputFields], dt[kMaxOutputFields];
    for (int k = 0; k < n; ++k) {
        const csi_output_field& f = fields[k];
        if (!out_known(f.field_id)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: unknown field id at position " + std::to_string(k));
        if (f.dtype != CSI_OUT_F64 && f.dtype != CSI_OUT_F32)
            return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("output: field ") + out_name(f.field_id) + ": unknown dtype (CSI_OUT_F64 or CSI_OUT_F32)");
        if (f.masked && !out_center(f.field_id))
            return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("output: field ") + out_name(f.field_id) + ": masking is for (Center, Center) fields only");
        const Bound b = out_bound(c, f.field_id);
        if (!b.p) return fail(c, CSI_ERR_NOT_BOUND, std::string("output: field ") + out_name(f.field_id) + " is not bound");
        nx[k] = b.ni - 2 * c->Hx; ny[k] = b.nj - 2 * c->Hy; dt[k] = f.dtype;
    }
    int at = -1;
    for (int q = 0; q < kMaxOutputSets && at < 0; ++q) if (!c->out_sets[q].live) at = q;
    if (at < 0) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: a context holds at most 4 output sets; destroy one first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->out_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->out_stream, hipStreamNonBlocking));
    OutputSet& S = c->out_sets[at];
    S.n = n; S.slots = slots; S.W = 0.0; S.any_averaged = false; S.grid_gen = c->grid_gen;
    plan_layout(nx, ny, dt, n, S.off, &S.record_bytes);
    int64_t acc = 0;
    for (int k = 0; k < n; ++k) {
        S.f[k] = fields[k]; S.sig[k] = out_bound(c, fields[k].field_id); S.nx[k] = nx[k]; S.ny[k] = ny[k];
        S.acc_off[k] = acc;
        if (fields[k].averaged) { S.any_averaged = true; acc += ((int64_t)nx[k] * ny[k] + 1) / 2 * 2; }
    }
    hipError_t e = hipSuccess;
    if (acc) {
        e = S.acc.alloc((size_t)acc);
        if (e == hipSuccess) e = hipMemsetAsync(S.acc.get(), 0, (size_t)acc * sizeof(double), c->stream);
    }
    if (e == hipSuccess) e = S.stage.alloc((size_t)(S.record_bytes * slots));
    if (e == hipSuccess) e = S.host.alloc((size_t)(S.record_bytes * slots), hipHostMallocDefault);
    S.packed.assign(slots, nullptr); S.done.assign(slots, nullptr); S.in_flight.assign(slots, 0);
    for (int q = 0; q < slots && e == hipSuccess; ++q) {
        e = hipEventCreateWithFlags(&S.packed[q], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&S.done[q], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        hipStreamSynchronize(c->stream);
        set_free(S);
        return fail(c, CSI_ERR_HIP, std::string("csi_output_create: ") + hipGetErrorString(e));
    }
    S.live = true;
    *handle = at + 1;
    return CSI_OK;
}

int32_t csi_output_layout(csi_context* c, int32_t handle, int32_t k, int64_t* byte_offset, int32_t* nx, int32_t* ny) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    const OutputSet* S = set_of(c, handle);
    if (!S) return CSI_ERR_INVALID_ARGUMENT;
    if (k < 0 || k >= S->n) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: field index out of range");
    if (byte_offset) *byte_offset = S->off[k];
    if (nx) *nx = S->nx[k];
    if (ny) *ny = S->ny[k];
    return CSI_OK;
}

int32_t csi_output_record_bytes(csi_context* c, int32_t handle, int64_t* bytes) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    const OutputSet* S = set_of(c, handle);
    if (!S) return CSI_ERR_INVALID_ARGUMENT;
    if (!bytes) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: bytes == NULL");
    *bytes = S->record_bytes;
    return CSI_OK;
}

int32_t csi_output_accumulate(csi_context* c, int32_t handle, double w) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    OutputSet* S = set_of(c, handle);
    if (!S) return CSI_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(w) || !(w > 0.0)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: the weight must be finite and > 0");
    if (S->any_averaged) {
        HIP_TRY(c, hipSetDevice(c->device));
        OutputTable T{};
        T.w = w;
        for (int k = 0; k < S->n; ++k) if (S->f[k].averaged) T.d[T.n++] = desc_of(c, *S, k, nullptr);
        launch_output_accumulate(T, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    S->W = S->W + w;
    return CSI_OK;
}

int32_t csi_output_snapshot(csi_context* c, int32_t handle, int32_t* slot) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    OutputSet* S = set_of(c, handle);
    if (!S) return CSI_ERR_INVALID_ARGUMENT;
    if (!slot) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: slot == NULL");
    if (S->any_averaged && S->W == 0.0)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: the set has averaged fields and nothing has been accumulated since the last snapshot (W == 0)");
    int q = -1;
    for (int k = 0; k < S->slots && q < 0; ++k) if (!S->in_flight[k]) q = k;
    if (q < 0) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: no free slot -- all " + std::to_string(S->slots) + " records of the set are in flight; wait for one and release it");
    HIP_TRY(c, hipSetDevice(c->device));
    uint8_t* record = S->stage.get() + (size_t)q * S->record_bytes;
    OutputTable T{};
    T.w = S->W;
    T.mask = c->g.has_mask ? c->g.mask + 1 + c->g.mask_ld : nullptr;
    T.mask_ld = c->g.mask_ld;
    for (int k = 0; k < S->n; ++k) T.d[T.n++] = desc_of(c, *S, k, record);
    launch_output_pack(T, c->stream);
    HIP_TRY(c, hipGetLastError());
    S->W = 0.0;                          // (the launch clears the accumulators)
    HIP_TRY(c, hipEventRecord(S->packed[q], c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->out_stream, S->packed[q], 0));
    HIP_TRY(c, hipMemcpyAsync(S->host.get() + (size_t)q * S->record_bytes, record, (size_t)S->record_bytes, hipMemcpyDeviceToHost, c->out_stream));
    HIP_TRY(c, hipEventRecord(S->done[q], c->out_stream));
    S->in_flight[q] = 1;
    *slot = q;
    return CSI_OK;
}

int32_t csi_output_test(csi_context* c, int32_t handle, int32_t slot, int32_t* done) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    OutputSet* S = set_of(c, handle);
    if (!S) return CSI_ERR_INVALID_ARGUMENT;
    if (!done) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: done == NULL");
    if (int32_t rc = slot_check(c, S, slot)) return rc;
    const hipError_t e = hipEventQuery(S->done[slot]);
    if (e != hipSuccess && e != hipErrorNotReady) return fail(c, CSI_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
    *done = e == hipSuccess;
    return CSI_OK;
}

int32_t csi_output_wait(csi_context* c, int32_t handle, int32_t slot, void** host_ptr) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    OutputSet* S = set_of(c, handle);
    if (!S) return CSI_ERR_INVALID_ARGUMENT;
    if (!host_ptr) return fail(c, CSI_ERR_INVALID_ARGUMENT, "output: host_ptr == NULL");
    if (int32_t rc = slot_check(c, S, slot)) return rc;
    HIP_TRY(c, hipEventSynchronize(S->done[slot]));
    *host_ptr = S->host.get() + (size_t)slot * S->record_bytes;
    return CSI_OK;
}

int32_t csi_output_release(csi_context* c, int32_t handle, int32_t slot) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    OutputSet* S = set_of(c, handle);
    if (!S) return CSI_ERR_INVALID_ARGUMENT;
    if (int32_t rc = slot_check(c, S, slot)) return rc;
    HIP_TRY(c, hipEventSynchronize(S->done[slot]));      // (a release without a wait: the copy must not land in a slot that is free)
    S->in_flight[slot] = 0;
    return CSI_OK;
}

int32_t csi_output_destroy(csi_context* c, int32_t handle) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    OutputSet* S = set_of(c, handle, false);
    if (!S) return CSI_ERR_INVALID_ARGUMENT;
    hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->out_stream) HIP_TRY(c, hipStreamSynchronize(c->out_stream));
    set_free(*S);
    return CSI_OK;
}

}
