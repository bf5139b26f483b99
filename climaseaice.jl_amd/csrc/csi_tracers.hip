// csi_tracers.hip -- csi_tracers_set, csi_tracers_tendencies, csi_tracers_update, csi_tracers_stats, csi_tracers_last (include/csi.h,
// "advected ice tracers and ice age").  The kernels: tracers.hip; their description: csi_kernels.h TracersDev.
//
// Host side: argument checks by name, the library-owned arrays (the dense c* of a stage, the Psi^- copies c^- of an RK3 step), the two
// halves of a stage as the step entries call them (csi_abi.hip), the Psi^- copy batch and update_state!'s mask and halo fill of the
// tracers.  The tracer arrays are the caller's; the context keeps a copy of the csi_tracers.  Nothing here waits for the device except
// csi_tracers_set, when it replaces arrays of another size.
#include "csi_ctx.h"

namespace csi_host {

static_assert(CSI_TRACERS_MAX == kTracersMax, "include/csi.h and csi_kernels.h state one limit");

// what the tracers were set against: the parent of h as it was bound then (a re-bind or a new grid since: csi_tracers_set again)
static int32_t tracers_current(csi_context* c, const char* who) {
    if (!c->trc.set) return fail(c, CSI_ERR_NOT_BOUND, std::string(who) + ": csi_tracers_set has not been called");
    const Bound &h = c->f[CSI_F_H], &s = c->trc.shape;
    if (c->trc.grid_gen != c->grid_gen || h.p == nullptr || h.ld != s.ld || h.ni != s.ni || h.nj != s.nj)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string(who) + ": the grid or the binding of h changed after csi_tracers_set -- call csi_tracers_set again");
    if (c->f[CSI_F_A].p == nullptr || c->f[CSI_F_A].ld != h.ld || c->f[CSI_F_A].nj != h.nj)
        return fail(c, CSI_ERR_NOT_BOUND, std::string(who) + ": needs field aice bound with the parent shape of h");
    return CSI_OK;
}

static TracersDev tracers_dev(const csi_context* c, int scheme, double dt, int from_cache) {
    const csi_context::Tracers& R = c->trc;
    TracersDev T{};
    T.g = c->g;
    T.u = ref_of(c, CSI_F_U); T.v = ref_of(c, CSI_F_V);
    T.a = ref_of(c, CSI_F_A);
    T.ab = from_cache ? ref_of(c, CSI_F_AM) : T.a;
    T.Ga = ref_of(c, CSI_F_GA);
    T.im = image_spec(c, CSI_F_H);
    T.n = R.t.n; T.scheme = scheme; T.w32 = c->weno_w32;
    T.dt = dt;
    T.ld = (long)R.shape.ld;
    const size_t plane = (size_t)R.shape.ld * (size_t)R.shape.nj;
    for (int k = 0; k < R.t.n; ++k) {
        T.c[k] = origin_of(c, R.t.c[k], R.shape.ld);
        const bool sourced = R.t.source[k] != 0.0 && R.free_;
        double* fr = sourced ? origin_of(c, R.free_.get() + (size_t)k * plane, R.shape.ld) : nullptr;
        T.cin[k] = (from_cache && R.free_valid && sourced) ? fr : T.c[k];
        T.cfree[k] = R.star_from_cache ? fr : nullptr;
        T.cb[k] = from_cache ? origin_of(c, R.base.get() + (size_t)k * plane, R.shape.ld) : T.c[k];
        T.G[k] = R.t.G[k] ? origin_of(c, R.t.G[k], R.shape.ld) : nullptr;
        T.weighting[k] = R.t.weighting[k]; T.nonnegative[k] = R.t.nonnegative[k]; T.source[k] = R.t.source[k];
    }
    T.star = R.star.get(); T.star_ld = (long)R.star_ld; T.star_plane = (long)R.star_plane;
    return T;
}

static bool any_weighted(const csi_tracers& t) {
    for (int k = 0; k < t.n; ++k) if (t.weighting[k] == CSI_TRACER_BY_CONCENTRATION) return true;
    return false;
}

int32_t tracers_first_half(csi_context* c, int scheme, double dt, int from_cache) {
    int32_t rc;
    if ((rc = tracers_current(c, "tracers"))) return rc;
    if (!std::isfinite(dt)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "tracers: dt must be finite");
    if (scheme && (rc = need_named(c, "tracers", "the tendencies ", {CSI_F_U, CSI_F_V}, ""))) return rc;
    if (any_weighted(c->trc.t) && (rc = need_named(c, "tracers", "a BY_CONCENTRATION tracer ", {CSI_F_GA}, ""))) return rc;
    if (from_cache) {
        if ((rc = need_named(c, "tracers", "from_cache ", {CSI_F_AM}, ""))) return rc;
        if (!c->trc.base_valid) return fail(c, CSI_ERR_INVALID_ARGUMENT, "tracers: from_cache needs csi_cache_current_fields after csi_tracers_set");
    }
    for (int id : {CSI_F_GA, CSI_F_AM})
        if (c->f[id].p && c->f[id].ld != c->trc.shape.ld) return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("tracers: parent shape mismatch: ") + slot_name(id) + " vs h");
    if (scheme && (rc = advect_scheme_check(c, scheme))) return rc;
    c->trc.star_from_cache = from_cache != 0;
    const TracersDev T = tracers_dev(c, scheme, dt, from_cache);
    if (scheme) {
        c->trc.last = launch_tracers_tendencies(T, c->mode, c->tune.trc_ntr > 0 ? c->tune.trc_ntr : 0, c->stream);
        ++c->trc.stencil_launches;
    } else {
        launch_tracers_star_noadv(T, c->stream);
        ++c->trc.update_launches;
    }
    HIP_TRY(c, hipGetLastError());
    c->trc.star_valid = true;
    return CSI_OK;
}

int32_t tracers_second_half(csi_context* c, double dt) {
    int32_t rc;
    if ((rc = tracers_current(c, "tracers"))) return rc;
    if (!std::isfinite(dt)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "tracers: dt must be finite");
    if (!c->trc.star_valid) return fail(c, CSI_ERR_INVALID_ARGUMENT, "tracers: csi_tracers_update needs a csi_tracers_tendencies before it (the stage's first half)");
    if ((rc = fill_width_check(c, CSI_F_H))) return rc;
    launch_tracers_finish(tracers_dev(c, 0, dt, 0), c->stream);
    ++c->trc.update_launches;
    HIP_TRY(c, hipGetLastError());
    c->trc.star_valid = false;
    if (c->trc.star_from_cache) c->trc.free_valid = true;
    return CSI_OK;
}

// cache_current_fields! of the tracers: c -> c^-, whole parents, in a batch of their own (two beyond six tracers)
int32_t tracers_cache(csi_context* c) {
    int32_t rc;
    if ((rc = tracers_current(c, "tracers"))) return rc;
    const csi_context::Tracers& R = c->trc;
    const size_t plane = (size_t)R.shape.ld * (size_t)R.shape.nj;
    for (int k0 = 0; k0 < R.t.n; k0 += 6) {
        CopyBatch B = copy_batch_aligned();
        for (int k = k0; k < R.t.n && k < k0 + 6; ++k) copy_add(B, R.t.c[k], R.base.get() + (size_t)k * plane, (long)plane);
        launch_copy_batch(B, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
    c->trc.base_valid = true;
    c->trc.free_valid = false;      // (the first stage's stencil reads the tracers themselves)
    return CSI_OK;
}

// update_state! outside a step: mask_immersed_field_xy! and the local halo fill of every tracer, as hs gets them (inside a step the
// second half's stores have written the zeros and the images)
int32_t tracers_update_state(csi_context* c) {
    int32_t rc;
    if ((rc = tracers_current(c, "tracers"))) return rc;
    const csi_context::Tracers& R = c->trc;
    const ImageSpec im = image_spec(c, CSI_F_H);
    for (int k = 0; k < R.t.n; ++k) launch_mask_center(FRef{origin_of(c, R.t.c[k], R.shape.ld), (int)R.shape.ld}, c->g, c->stream);
    for (int k0 = 0; k0 < R.t.n; k0 += 6) {
        HaloBatch B{};
        for (int k = k0; k < R.t.n && k < k0 + 6; ++k) { B.f[B.n] = FRef{origin_of(c, R.t.c[k], R.shape.ld), (int)R.shape.ld}; B.im[B.n] = im; ++B.n; }
        launch_fill_halo_batch(B, c->g, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

// CSI_TRACER_FIELD(k) as an output field: the binding an output set remembers (p == nullptr: no such tracer now)
bool tracer_field_id(int32_t id, int* k) {
    if (id < CSI_TRACER_FIELD(0) || id >= CSI_TRACER_FIELD(CSI_TRACERS_MAX)) return false;
    *k = id - CSI_TRACER_FIELD(0);
    return true;
}
Bound tracer_bound(const csi_context* c, int k) {
    Bound b{};
    if (c->trc.set && k < c->trc.t.n) { b = c->trc.shape; b.p = c->trc.t.c[k]; }
    return b;
}

struct Span { const char* name; int k; uintptr_t lo, hi; };

}  // namespace csi_host

extern "C" {

int32_t csi_tracers_set(csi_context* c, const csi_tracers* t) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    csi_context::Tracers& R = c->trc;
    if (!t) {
        if (R.set) HIP_TRY(c, hipStreamSynchronize(c->stream));
        R.set = false; R.star_valid = R.base_valid = R.free_valid = false;
        R.star.release(); R.base.release(); R.free_.release();
        return CSI_OK;
    }
    if (c->tile.set || is_tiled(c)) return fail(c, CSI_ERR_UNSUPPORTED, "tracers: tiled contexts are not supported (csi_tile_set was called on this context, or its grid has connected sides)");
    if (!c->grid_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_grid_set has not been called");
    if (int32_t rc = need_named(c, "tracers", "csi_tracers_set ", {CSI_F_H, CSI_F_A}, " -- the tracers take the parent shape of h")) return rc;
    if (t->n < 1 || t->n > CSI_TRACERS_MAX) return fail(c, CSI_ERR_INVALID_ARGUMENT, "tracers: n must be between 1 and CSI_TRACERS_MAX (8)");
    const Bound h = c->f[CSI_F_H];
    if (c->f[CSI_F_A].ld != h.ld || c->f[CSI_F_A].nj != h.nj) return fail(c, CSI_ERR_INVALID_ARGUMENT, "tracers: parent shape mismatch: aice vs h");
    const size_t plane = (size_t)h.ld * (size_t)h.nj, bytes = plane * sizeof(double);
    std::vector<Span> spans;
    for (int id : {CSI_F_H, CSI_F_A, CSI_F_HS})
        if (c->f[id].p) spans.push_back(Span{slot_name(id), -1, (uintptr_t)c->f[id].p, (uintptr_t)c->f[id].p + (size_t)c->f[id].ld * (size_t)c->f[id].nj * sizeof(double)});
    HIP_TRY(c, hipSetDevice(c->device));
    for (int k = 0; k < t->n; ++k) {
        const std::string who = "tracers: tracer " + std::to_string(k);
        if (!t->c[k]) return fail(c, CSI_ERR_INVALID_ARGUMENT, who + ": c == NULL");
        if (t->weighting[k] != CSI_TRACER_PLAIN && t->weighting[k] != CSI_TRACER_BY_CONCENTRATION)
            return fail(c, CSI_ERR_INVALID_ARGUMENT, who + ": unknown weighting (CSI_TRACER_PLAIN or CSI_TRACER_BY_CONCENTRATION)");
        if (t->nonnegative[k] != 0 && t->nonnegative[k] != 1) return fail(c, CSI_ERR_INVALID_ARGUMENT, who + ": nonnegative must be 0 or 1");
        if (!std::isfinite(t->source[k])) return fail(c, CSI_ERR_INVALID_ARGUMENT, who + ": source must be finite");
        for (int q = 0; q < 2; ++q) {
            double* p = q == 0 ? t->c[k] : t->G[k];
            if (!p) continue;
            // a shape that is not h's: the allocation that holds the array must hold a whole parent of h behind the pointer
            void* base = nullptr; size_t size = 0;
            if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
                (void)hipGetLastError();
                return fail(c, CSI_ERR_INVALID_ARGUMENT, who + (q ? ": G" : ": c") + " is not a device array");
            }
            if ((uintptr_t)p + bytes > (uintptr_t)base + size)
                return fail(c, CSI_ERR_INVALID_ARGUMENT, who + (q ? ": G" : ": c") + " is smaller than the parent of h (the tracers take its shape: " +
                                                             std::to_string(h.ld) + " x " + std::to_string(h.nj) + " doubles)");
            const Span s{q ? "G" : "c", k, (uintptr_t)p, (uintptr_t)p + bytes};
            for (const Span& o : spans)
                if (s.lo < o.hi && o.lo < s.hi)
                    return fail(c, CSI_ERR_INVALID_ARGUMENT, who + ": " + s.name + " aliases " + (o.k < 0 ? std::string("field ") + o.name : std::string(o.name) + " of tracer " + std::to_string(o.k)));
            spans.push_back(s);
        }
    }
    const int64_t star_ld = ((int64_t)c->Nx + 1) / 2 * 2, star_plane = star_ld * c->Ny;
    HIP_TRY(c, R.star.ensure((size_t)star_plane * (size_t)t->n, c->stream, true));
    HIP_TRY(c, R.base.ensure(plane * (size_t)t->n, c->stream, true));
    bool any_source = false;
    for (int k = 0; k < t->n; ++k) any_source |= t->source[k] != 0.0;
    if (any_source) HIP_TRY(c, R.free_.ensure(plane * (size_t)t->n, c->stream, true));
    else if (R.free_) { HIP_TRY(c, hipStreamSynchronize(c->stream)); R.free_.release(); }
    R.t = *t;
    for (int k = t->n; k < CSI_TRACERS_MAX; ++k) { R.t.c[k] = R.t.G[k] = nullptr; R.t.weighting[k] = R.t.nonnegative[k] = 0; R.t.source[k] = 0.0; }
    R.shape = h; R.grid_gen = c->grid_gen;
    R.star_ld = star_ld; R.star_plane = star_plane;
    R.star_valid = R.base_valid = R.free_valid = false;
    R.set = true;
    return CSI_OK;
}

int32_t csi_tracers_tendencies(csi_context* c, int32_t scheme, double dt, int32_t from_cache) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    return tracers_first_half(c, scheme, dt, from_cache);
}

int32_t csi_tracers_update(csi_context* c, double dt) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    return tracers_second_half(c, dt);
}

int32_t csi_tracers_stats(csi_context* c, int64_t* stencil_launches, int64_t* update_launches) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (stencil_launches) *stencil_launches = c->trc.stencil_launches;
    if (update_launches) *update_launches = c->trc.update_launches;
    return CSI_OK;
}

int32_t csi_tracers_last(csi_context* c, int32_t* tracers_per_thread, int32_t* tile_x, int32_t* tile_y, int32_t* groups) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (tracers_per_thread) *tracers_per_thread = c->trc.last.ntr;
    if (tile_x) *tile_x = c->trc.last.tx;
    if (tile_y) *tile_y = c->trc.last.ty;
    if (groups) *groups = c->trc.last.groups;
    return CSI_OK;
}

}
