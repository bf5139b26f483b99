// csi_momentum_terms.hip -- csi_momentum_terms_compute, csi_momentum_budget_compute, csi_momentum_terms_stats (include/csi.h): the terms
// of the momentum balance as fields at the velocity points, the interface stresses, and the power of each term.  Stands where users of
// the reference call x_momentum_stress / y_momentum_stress (src/SeaIceDynamics/sea_ice_external_stress.jl:33-37, 162-174) from a coupler
// and restate u_velocity_tendency term by term on the host.  The kernels: momentum_terms.hip.
//
// Host side: argument and binding checks by name, ONE launch for the fields (nothing is waited for); for the power sums the host path
// of the ordered reductions (csi_ctx.h reduce_begin / reduce_end, reduce_ranks).  No halo is filled and nothing is exchanged: the elements read are the ones the step entry points leave valid.
#include "csi_ctx.h"

namespace csi_host {

// The checks both entry points share and the kernels' description of the model.  internal: the internal term is wanted.
static int32_t terms_dev(csi_context* c, const char* who, bool internal, MomTermsDev* out, bool* visc) {
    if (!c->grid_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_grid_set has not been called");
    if (c->Hx < 1 || c->Hy < 1) return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string(who) + ": the grid needs halo >= 1");
    int32_t rc;
    if ((rc = need_named(c, who, "", {CSI_F_U, CSI_F_V}, ": a model without dynamics has no momentum balance"))) return rc;
    if ((rc = need_named(c, who, "", {CSI_F_H, CSI_F_A}, ""))) return rc;
    const bool free_drift = c->dynamics == CSI_DYNAMICS_FREE_DRIFT;
    const bool evp_sigma = internal && !free_drift && c->rheology == CSI_RHEOLOGY_EVP;
    if (evp_sigma && (rc = need_named(c, who, "", {CSI_F_S11, CSI_F_S22, CSI_F_S12}, ": the internal term of an ElastoViscoPlasticRheology reads its stress fields")))
        return rc;
    if ((rc = check_stress_fields(c, CSI_STRESS_TOP))) return rc;
    if ((rc = check_stress_fields(c, CSI_STRESS_BOTTOM))) return rc;
    if ((c->f[CSI_F_FORCING_U].p != nullptr) != (c->f[CSI_F_FORCING_V].p != nullptr))
        return fail(c, CSI_ERR_NOT_BOUND, "model.forcing arrays: bind both CSI_F_FORCING_U and CSI_F_FORCING_V or neither");
    MomTermsDev T{};
    T.P = evp_dev(c, 0.0);
    if (!c->evp_set) T.P.rho = 900.0;           // (csi_budget_compute's rule: the density before csi_evp_params_set)
    // the gather of the stored-stress instantiation also addresses u^n, v^n and alpha, which the terms do not use: any valid array
    if (!T.P.un.p) T.P.un = T.P.u;
    if (!T.P.vn.p) T.P.vn = T.P.v;
    if (!T.P.al.p) T.P.al = T.P.h;
    T.P.free_drift = 0;
    if (free_drift) T.P.has_cor = 0;            // StressBalanceFreeDrift has no Coriolis term
    T.nu = c->nu;
    T.exu = extra_x(c, CSI_F_U);
    T.eyv = extra_y(c, CSI_F_V);
    T.no_internal = (!internal || free_drift) ? 1 : 0;
    *visc = !evp_sigma;
    *out = T;
    return CSI_OK;
}

static int32_t power_local(csi_context* c, int32_t what, double* slots) {
    if (what == 0 || (what & ~CSI_MBUDGET_ALL))
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "momentum budget: `what` must be a non-empty mask of CSI_MBUDGET_EXTERNAL (1), CSI_MBUDGET_BODY (2) and CSI_MBUDGET_INTERNAL (4); unknown bit");
    MomTermsDev T;
    bool visc;
    int32_t rc = terms_dev(c, "momentum budget", what & CSI_MBUDGET_INTERNAL, &T, &visc);
    if (rc) return rc;
    double* result;
    if ((rc = reduce_begin(c, &T.part, &T.nrec, &result))) return rc;
    launch_momentum_power(T, visc, result, c->stream);
    return reduce_end(c, MQ_COUNT, result, slots);
}

}  // namespace csi_host

extern "C" {

int32_t csi_momentum_terms_compute(csi_context* c, int32_t mask) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    int32_t rc = peer_check_entry(c);
    if (rc) return rc;
    if ((mask & CSI_MTERM_ALL) == 0 || (mask & ~(CSI_MTERM_ALL | CSI_MTERM_RAW_STRESS)))
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "momentum terms: `mask` must hold at least one of the CSI_MTERM_* term bits (1 .. 16), optionally with CSI_MTERM_RAW_STRESS (32); unknown bit");
    MomTermsDev T;
    bool visc;
    if ((rc = terms_dev(c, "momentum terms", mask & CSI_MTERM_INTERNAL, &T, &visc))) return rc;
    for (int t = 0; t < MQ_COUNT; ++t) {
        if (!(mask & (1 << t))) continue;
        for (int q = 0; q < 2; ++q) {
            const int id = CSI_F_M_CORIOLIS_X + 2 * t + q;
            if (!c->f[id].p) return fail(c, CSI_ERR_NOT_BOUND, std::string("momentum terms: field ") + slot_name(id) + " is requested but no array is bound to its slot");
            T.out[2 * t + q] = ref_of(c, id);
        }
    }
    T.raw_stress = (mask & CSI_MTERM_RAW_STRESS) ? 1 : 0;
    HIP_TRY(c, hipSetDevice(c->device));
    launch_momentum_terms(T, visc, c->stream);
    HIP_TRY(c, hipGetLastError());
    ++c->mterm_launches;
    return CSI_OK;
}

int32_t csi_momentum_budget_compute(csi_context* c, int32_t what, csi_momentum_budget* out) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, CSI_ERR_INVALID_ARGUMENT, "momentum budget: out == NULL");
    double slot[MQ_COUNT] = {};
    int32_t rc = peer_check_entry(c);
    if (!rc) rc = power_local(c, what, slot);
    if ((rc = reduce_ranks(c, "momentum budget", rc, MQ_COUNT, 0, MQ_COUNT, nullptr, slot))) return rc;
    const double nan = std::nan("");
    csi_momentum_budget b{};
    b.what = what;
    b.coriolis = b.top = b.bottom = b.internal = b.forcing = nan;
    if (what & CSI_MBUDGET_EXTERNAL) { b.top = slot[MQ_TOP]; b.bottom = slot[MQ_BOTTOM]; }
    if (what & CSI_MBUDGET_BODY) { b.coriolis = slot[MQ_CORIOLIS]; b.forcing = slot[MQ_FORCING]; }
    if (what & CSI_MBUDGET_INTERNAL) b.internal = slot[MQ_INTERNAL];
    *out = b;
    ++c->mterm_budget_calls;
    return CSI_OK;
}

int32_t csi_momentum_terms_stats(csi_context* c, int64_t* launches, int64_t* budget_calls) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (launches) *launches = c->mterm_launches;
    if (budget_calls) *budget_calls = c->mterm_budget_calls;
    return CSI_OK;
}

}
