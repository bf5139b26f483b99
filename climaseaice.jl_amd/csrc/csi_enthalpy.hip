// csi_enthalpy.hip -- the host side of the enthalpy-method column model (include/csi.h, "enthalpy-method column model"; kernels:
// enthalpy.hip).  Stands where the reference has EnthalpyMethodSeaIceModel's constructor, set!, update_state! and time_step!
// (src/EnthalpyMethodSeaIceModel.jl:50-185): the model object with its bound arrays and boundary temperatures, the rule that chooses
// the kernel form (csi_enthalpy_plan), and the launch loop, which evaluates the time indexing of series-valued boundary temperatures
// at every sub-step's start time on the host and queues launches without ever waiting for the device.
#include "csi_ctx.h"
#include "enthalpy_dev.h"

struct csi_enthalpy {
    csi_context* ctx = nullptr;
    csi_enthalpy_params p{};
    std::vector<double> zf;
    DeviceBuf<double> metrics;           // dzc[Nz], dzf[Nz + 1], zc[Nz]
    double* arr[4] = {nullptr, nullptr, nullptr, nullptr};
    struct Side {
        int kind = CSI_ENTH_BC_NONE;
        double number = 0.0;
        const double* data = nullptr;
        int64_t ld = 0, slice_stride = 0;
        int indexing = 0;
        double period = 0.0;
        std::vector<double> times;
    } side[2];
    int form = 0;                        // CSI_ENTH_PER_STEP | CSI_ENTH_ON_CHIP, chosen at creation
    int64_t lds_bytes = 0;
    int cap = 1;
    csi_enthalpy_launch last{0, 0, 0, 0};
};

namespace csi_host {

static const char* const kEnthName[4] = {"H", "T", "phi", "kappa"};

static int32_t enth_plan(int Nz, int forced, int* form, int64_t* lds, int* waves, int* cap) {
    if (Nz < 1 || forced < 0 || forced > 2) return CSI_ERR_INVALID_ARGUMENT;
    const int64_t bytes = (2 * (int64_t)Nz + 2) * 512;
    const int w = (int)(CSI_ENTH_LDS_PER_CU / bytes);
    bool chip = w >= CSI_ENTH_MIN_WAVES_PER_CU;
    if (forced == 1) chip = false;
    if (forced == 2) {
        if (w < 1) return CSI_ERR_UNSUPPORTED;
        chip = true;
    }
    *form = chip ? CSI_ENTH_ON_CHIP : CSI_ENTH_PER_STEP;
    *lds = chip ? bytes : 0;
    *waves = chip ? w : 0;
    *cap = chip ? CSI_ENTH_MAX_SUBSTEPS : 1;
    return CSI_OK;
}

static int32_t need_arrays(csi_enthalpy* e, const char* who, std::initializer_list<int> ids) {
    for (int id : ids)
        if (!e->arr[id]) return fail(e->ctx, CSI_ERR_NOT_BOUND, std::string(who) + ": array " + kEnthName[id] + " is not bound (csi_enthalpy_bind)");
    return CSI_OK;
}

static EnthDev enth_dev(const csi_enthalpy* e, double dt) {
    EnthDev E{};
    E.nx = e->p.Nx; E.ny = e->p.Ny; E.nz = e->p.Nz;
    E.plane = (long)e->p.Nx * e->p.Ny;
    E.H = e->arr[CSI_ENTH_H]; E.T = e->arr[CSI_ENTH_T]; E.phi = e->arr[CSI_ENTH_PHI]; E.kappa = e->arr[CSI_ENTH_KAPPA];
    E.dzc = e->metrics.get(); E.dzf = E.dzc + e->p.Nz; E.zc = E.dzf + e->p.Nz + 1;
    E.c = e->p.ice_heat_capacity; E.L = e->p.fusion_enthalpy; E.k_ice = e->p.kappa_ice; E.k_water = e->p.kappa_water;
    E.dt = dt;
    for (int s = 0; s < 2; ++s) {
        const csi_enthalpy::Side& b = e->side[s];
        E.side[s] = EnthSide{b.kind, 0, b.number, b.data, (long)b.ld, (long)b.slice_stride};
    }
    return E;
}

// entry q of the table: both sides' series at time t
static int32_t plan_at(csi_enthalpy* e, EnthSteps& S, int q, double t) {
    for (int s = 0; s < 2; ++s) {
        const csi_enthalpy::Side& b = e->side[s];
        S.n1[s][q] = S.n2[s][q] = 0; S.frac[s][q] = 0.0;
        if (b.kind != CSI_ENTH_BC_SERIES_SCALAR && b.kind != CSI_ENTH_BC_SERIES_PLANE) continue;
        int32_t n1, n2;
        double frac;
        if (csi_time_series_plan(b.times.data(), (int32_t)b.times.size(), b.indexing, b.period, t, &n1, &n2, &frac))
            return fail(e->ctx, CSI_ERR_INVALID_ARGUMENT, std::string("enthalpy model: the ") + (s ? "top" : "bottom") + " temperature series cannot be evaluated: the time is not a finite number");
        S.n1[s][q] = n1; S.n2[s][q] = n2; S.frac[s][q] = frac;
    }
    return CSI_OK;
}

void enthalpy_release(csi_context* c) {
    for (csi_enthalpy* e : c->enthalpies) delete e;
    c->enthalpies.clear();
}

}  // namespace csi_host

extern "C" {

int32_t csi_enthalpy_plan(int32_t Nz, int32_t forced_path, int32_t* form, int64_t* lds_bytes, int32_t* waves_per_cu, int32_t* max_substeps) {
    int f = 0, w = 0, cap = 0;
    int64_t lds = 0;
    const int32_t rc = enth_plan(Nz, forced_path, &f, &lds, &w, &cap);
    if (rc) return rc;
    if (form) *form = f;
    if (lds_bytes) *lds_bytes = lds;
    if (waves_per_cu) *waves_per_cu = w;
    if (max_substeps) *max_substeps = cap;
    return CSI_OK;
}

int32_t csi_enthalpy_create(csi_context* c, const csi_enthalpy_params* p, csi_enthalpy** out) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!p || !out) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: params and out must not be NULL");
    *out = nullptr;
    if (p->Nx < 1 || p->Ny < 1 || p->Nz < 1 || p->reserved) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: Nx, Ny, Nz >= 1 (reserved must be 0)");
    if (p->Nz > (1 << 24)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: Nz beyond 2^24");
    if (!p->z_faces) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: z_faces must not be NULL");
    for (int k = 0; k <= p->Nz; ++k)
        if (!std::isfinite(p->z_faces[k]) || (k > 0 && !(p->z_faces[k] > p->z_faces[k - 1])))
            return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: z_faces must be finite and strictly increasing");
    for (double v : {p->ice_heat_capacity, p->water_heat_capacity, p->fusion_enthalpy, p->kappa_ice, p->kappa_water})
        if (!std::isfinite(v)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: ice_heat_capacity, water_heat_capacity, fusion_enthalpy, kappa_ice and kappa_water must be finite");
    if (p->ice_heat_capacity == 0.0) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: ice_heat_capacity must not be zero (T = H / c)");
    csi_enthalpy* e = new csi_enthalpy();
    e->ctx = c;
    e->p = *p;
    e->zf.assign(p->z_faces, p->z_faces + p->Nz + 1);
    e->p.z_faces = nullptr;
    int waves = 0;
    const int32_t rc = enth_plan(p->Nz, c->tune.enth_path, &e->form, &e->lds_bytes, &waves, &e->cap);
    if (rc) {
        delete e;
        return fail(c, rc, "enthalpy model: CSI_ENTH_PATH=2 (on chip), but a column of this Nz does not fit the 160 KiB of a CU ((2 Nz + 2) * 512 bytes per wave)");
    }
    // the operators' metrics (include/csi.h): dzc, dzf, zc
    const int Nz = p->Nz;
    std::vector<double> m((size_t)3 * Nz + 1);
    double *dzc = m.data(), *dzf = dzc + Nz, *zc = dzf + Nz + 1;
    for (int k = 0; k < Nz; ++k) {
        zc[k] = (e->zf[k] + e->zf[k + 1]) / 2.0;
        dzc[k] = e->zf[k + 1] - e->zf[k];
    }
    for (int k = 1; k < Nz; ++k) dzf[k] = zc[k] - zc[k - 1];
    dzf[0] = dzc[0];
    dzf[Nz] = dzc[Nz - 1];
    hipSetDevice(c->device);
    hipError_t he = e->metrics.alloc(m.size());
    if (he == hipSuccess) he = hipMemcpyAsync(e->metrics.get(), m.data(), m.size() * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);      // (creation only: m leaves scope)
    if (he == hipSuccess && e->form == CSI_ENTH_ON_CHIP) he = enthalpy_allow_lds((size_t)e->lds_bytes);
    if (he != hipSuccess) {
        delete e;
        return fail(c, CSI_ERR_HIP, std::string("enthalpy model: ") + hipGetErrorString(he));
    }
    c->enthalpies.push_back(e);
    *out = e;
    return CSI_OK;
}

int32_t csi_enthalpy_destroy(csi_enthalpy* e) {
    if (!e) return CSI_OK;
    csi_context* c = e->ctx;
    hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));         // (a launch that reads the metrics may still run)
    c->enthalpies.erase(std::remove(c->enthalpies.begin(), c->enthalpies.end(), e), c->enthalpies.end());
    delete e;
    return CSI_OK;
}

int32_t csi_enthalpy_bind(csi_enthalpy* e, int32_t which, void* dev) {
    if (!e) return CSI_ERR_INVALID_ARGUMENT;
    if (which < CSI_ENTH_H || which > CSI_ENTH_KAPPA) return fail(e->ctx, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: bind takes H, T, PHI or KAPPA");
    if (((uintptr_t)dev) & 7) return fail(e->ctx, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: arrays must be 8-byte aligned");
    e->arr[which] = (double*)dev;
    return CSI_OK;
}

int32_t csi_enthalpy_boundary_set(csi_enthalpy* e, int32_t side, int32_t kind, double number, const void* dev_array, const csi_time_series* ts) {
    if (!e) return CSI_ERR_INVALID_ARGUMENT;
    csi_context* c = e->ctx;
    if (side < CSI_ENTH_T_BOTTOM || side > CSI_ENTH_H_TOP) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: unknown side");
    if (kind < CSI_ENTH_BC_NONE || kind > CSI_ENTH_BC_GRADIENT) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: unknown boundary condition kind");
    if (side >= CSI_ENTH_H_BOTTOM) {
        if (kind == CSI_ENTH_BC_NONE) return CSI_OK;
        return fail(c, CSI_ERR_UNSUPPORTED, "enthalpy model: a boundary condition on H is not supported -- the reference steps H with its default zero-flux conditions; give value conditions on T");
    }
    if (kind == CSI_ENTH_BC_FLUX || kind == CSI_ENTH_BC_GRADIENT)
        return fail(c, CSI_ERR_UNSUPPORTED, "enthalpy model: a flux or gradient boundary condition on T is not supported -- ValueBoundaryCondition or the default");
    csi_enthalpy::Side b;
    b.kind = kind;
    if (kind == CSI_ENTH_BC_NUMBER) {
        if (!std::isfinite(number)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: a boundary temperature must be finite");
        b.number = number;
    } else if (kind == CSI_ENTH_BC_ARRAY) {
        if (!dev_array || (((uintptr_t)dev_array) & 7)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: a boundary array must not be NULL and must be 8-byte aligned");
        b.data = (const double*)dev_array;
        b.ld = e->p.Nx;
    } else if (kind != CSI_ENTH_BC_NONE) {
        if (!ts || !ts->times || !ts->data || (((uintptr_t)ts->data) & 7)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: a boundary series needs times and 8-byte aligned data");
        if (ts->backend != CSI_SERIES_DEVICE)
            return fail(c, CSI_ERR_UNSUPPORTED, "enthalpy model: the HOST series backend is not supported for boundary temperatures -- the slices of a series live in device memory (CSI_SERIES_DEVICE)");
        int32_t n1, n2;
        double frac;
        if (ts->nt < 2 || csi_time_series_plan(ts->times, ts->nt, ts->indexing, ts->period, ts->times[0], &n1, &n2, &frac))
            return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: boundary series: nt >= 2, strictly increasing finite times, a known indexing kind and (CYCLICAL) a period longer "
                                                     "than the span of the times are required");
        const bool plane = kind == CSI_ENTH_BC_SERIES_PLANE;
        b.ld = plane ? ts->ld : 1;
        b.slice_stride = ts->slice_stride;
        if (plane ? (b.ld < e->p.Nx || b.slice_stride < b.ld * (int64_t)(e->p.Ny - 1) + e->p.Nx) : b.slice_stride < 1)
            return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: boundary series: ld / slice_stride too small for its slices");
        b.data = (const double*)ts->data;
        b.indexing = ts->indexing; b.period = ts->period;
        b.times.assign(ts->times, ts->times + ts->nt);
    }
    e->side[side] = std::move(b);
    return CSI_OK;
}

int32_t csi_enthalpy_set(csi_enthalpy* e, int32_t which, double time) {
    if (!e) return CSI_ERR_INVALID_ARGUMENT;
    csi_context* c = e->ctx;
    if (which != CSI_ENTH_T && which != CSI_ENTH_H) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: set takes T or H");
    int32_t rc;
    if (which == CSI_ENTH_T ? (rc = need_arrays(e, "enthalpy set T", {CSI_ENTH_H, CSI_ENTH_T, CSI_ENTH_PHI}))
                            : (rc = need_arrays(e, "enthalpy set H", {CSI_ENTH_H, CSI_ENTH_T}))) return rc;
    EnthSteps S{};
    S.n = 1;
    if (which == CSI_ENTH_H && (rc = plan_at(e, S, 0, time))) return rc;
    hipSetDevice(c->device);
    launch_enthalpy_state(enth_dev(e, 0.0), S, which == CSI_ENTH_T ? ENTH_SET_T : ENTH_SET_H, c->stream);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

int32_t csi_enthalpy_update_state(csi_enthalpy* e, double time) {
    if (!e) return CSI_ERR_INVALID_ARGUMENT;
    csi_context* c = e->ctx;
    int32_t rc;
    if ((rc = need_arrays(e, "enthalpy update_state", {CSI_ENTH_H, CSI_ENTH_T, CSI_ENTH_PHI, CSI_ENTH_KAPPA}))) return rc;
    EnthSteps S{};
    S.n = 1;
    if ((rc = plan_at(e, S, 0, time))) return rc;
    hipSetDevice(c->device);
    launch_enthalpy_state(enth_dev(e, 0.0), S, ENTH_UPDATE_STATE, c->stream);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

int32_t csi_enthalpy_time_step(csi_enthalpy* e, double dt, int32_t n, double time, double* time_out) {
    if (!e) return CSI_ERR_INVALID_ARGUMENT;
    csi_context* c = e->ctx;
    if (!std::isfinite(dt)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy time step: dt must be finite");
    if (n < 1) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy time step: n >= 1 steps");
    if (!std::isfinite(time)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy time step: the time must be finite");
    int32_t rc;
    if ((rc = need_arrays(e, "enthalpy time step", {CSI_ENTH_H, CSI_ENTH_T, CSI_ENTH_PHI, CSI_ENTH_KAPPA}))) return rc;
    hipSetDevice(c->device);
    const EnthDev E = enth_dev(e, dt);
    const bool chip = e->form == CSI_ENTH_ON_CHIP;
    double t = time;
    int launches = 0;
    for (int done = 0; done < n;) {
        EnthSteps S{};
        S.n = std::min(n - done, e->cap);
        for (int q = 0; q < S.n; ++q) {
            if ((rc = plan_at(e, S, q, t))) return rc;
            t = t + dt;
        }
        launch_enthalpy_steps(E, S, chip, (size_t)e->lds_bytes, c->stream);
        HIP_TRY(c, hipGetLastError());
        done += S.n;
        ++launches;
    }
    e->last = csi_enthalpy_launch{e->form, launches, std::min((int)n, e->cap), (int32_t)e->lds_bytes};
    if (time_out) *time_out = t;
    return CSI_OK;
}

int32_t csi_enthalpy_last_launch(csi_enthalpy* e, csi_enthalpy_launch* out) {
    if (!e) return CSI_ERR_INVALID_ARGUMENT;
    if (!out) return fail(e->ctx, CSI_ERR_INVALID_ARGUMENT, "enthalpy model: out must not be NULL");
    *out = e->last;
    return CSI_OK;
}

int32_t csi_enthalpy_ice_thickness(csi_enthalpy* e, double Tm, void* dev_out) {
    if (!e) return CSI_ERR_INVALID_ARGUMENT;
    csi_context* c = e->ctx;
    if (std::isnan(Tm)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy ice thickness: the melting temperature is NaN");
    if (!dev_out || (((uintptr_t)dev_out) & 7)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "enthalpy ice thickness: the output array must not be NULL and must be 8-byte aligned");
    int32_t rc;
    if ((rc = need_arrays(e, "enthalpy ice thickness", {CSI_ENTH_T}))) return rc;
    hipSetDevice(c->device);
    launch_enthalpy_thickness(enth_dev(e, 0.0), Tm, e->zf[0], (double*)dev_out, c->stream);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

}
