// csi_derived.hip -- csi_derived_compute, csi_budget_compute, csi_derived_stats (include/csi.h): derived (Center, Center) fields and the
// energy budget integrals of the bound state.  Stands where users of the reference rebuild the strain rates that
// _compute_evp_viscosities! drops (src/Rheologies/elasto_visco_plastic_rheology.jl:247-260) on the host, and where its
// test/test_rheology_energy_budget.jl sums the discrete budget cell by cell.  The kernels: derived.hip, budget.hip.
//
// Host side: argument and binding checks by name, ONE launch for the derived fields (nothing is waited for: the fields are read by
// whatever is queued next on the context's stream, e.g. an output set's pack launch); for the budget the host path of the ordered
// reductions (csi_ctx.h reduce_begin / reduce_end, reduce_ranks).
#include "csi_ctx.h"

namespace csi_host {

static const int kStressBits = CSI_DERIVED_SIGMA_I | CSI_DERIVED_SIGMA_II | CSI_DERIVED_STRESS_POWER;

static int32_t budget_local(csi_context* c, int32_t what, double* slots) {
    if (what == 0 || (what & ~CSI_BUDGET_ALL)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "budget: `what` must be a non-empty mask of CSI_BUDGET_STRESS (1) and CSI_BUDGET_KINETIC (2); unknown bit");
    if (!c->grid_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_grid_set has not been called");
    if (c->Hx < 1 || c->Hy < 1) return fail(c, CSI_ERR_INVALID_ARGUMENT, "budget: the grid needs halo >= 1");
    const bool stress = what & CSI_BUDGET_STRESS, kin = what & CSI_BUDGET_KINETIC;
    int32_t rc;
    if ((rc = need_named(c, "budget", "every group ", {CSI_F_U, CSI_F_V}, ": a model without dynamics has no energy budget"))) return rc;
    if (stress) {
        if (c->rheology != CSI_RHEOLOGY_EVP) return fail(c, CSI_ERR_NOT_BOUND, "budget: the stress group needs field sigma11 (an ElastoViscoPlasticRheology's stress fields; this model's rheology has none)");
        if ((rc = need_named(c, "budget", "the stress group ", {CSI_F_S11, CSI_F_S22, CSI_F_S12}, ": an ElastoViscoPlasticRheology's stress fields"))) return rc;
    }
    if (kin && (rc = need_named(c, "budget", "the kinetic group ", {CSI_F_H, CSI_F_A}, ""))) return rc;
    BudgetDev D{};
    D.g = c->g;
    D.u = ref_of(c, CSI_F_U); D.v = ref_of(c, CSI_F_V);
    D.s11 = ref_of(c, CSI_F_S11); D.s22 = ref_of(c, CSI_F_S22); D.s12 = ref_of(c, CSI_F_S12);
    D.h = ref_of(c, CSI_F_H); D.a = ref_of(c, CSI_F_A);
    D.rho = c->evp_set ? c->evp.sea_ice_density : 900.0;
    double* result;
    if ((rc = reduce_begin(c, &D.part, &D.nrec, &result))) return rc;
    launch_budget(D, stress, kin, result, c->stream);
    return reduce_end(c, BQ_COUNT, result, slots);
}

}  // namespace csi_host

extern "C" {

int32_t csi_derived_compute(csi_context* c, int32_t mask) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    int32_t rc = peer_check_entry(c);
    if (rc) return rc;
    if (mask == 0 || (mask & ~CSI_DERIVED_ALL)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "derived: `mask` must be a non-empty set of the CSI_DERIVED_* bits (1 .. 64); unknown bit");
    if (!c->grid_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_grid_set has not been called");
    if (c->Hx < 1 || c->Hy < 1) return fail(c, CSI_ERR_INVALID_ARGUMENT, "derived: the grid needs halo >= 1");
    const bool stress = mask & kStressBits;
    if ((rc = need_named(c, "derived", "every field ", {CSI_F_U, CSI_F_V}, ": a model without velocities has no derived fields"))) return rc;
    if (stress) {
        if (c->rheology != CSI_RHEOLOGY_EVP) return fail(c, CSI_ERR_NOT_BOUND, "derived: the stress group needs field sigma11 (an ElastoViscoPlasticRheology's stress fields; this model's rheology has none)");
        if ((rc = need_named(c, "derived", "the stress group ", {CSI_F_S11, CSI_F_S22, CSI_F_S12, CSI_F_P}, ": an ElastoViscoPlasticRheology's fields"))) return rc;
    }
    DerivedDev D{};
    for (int k = 0; k < DV_COUNT; ++k) {
        if (!(mask & (1 << k))) continue;
        const int id = CSI_F_D_DIVERGENCE + k;
        if (!c->f[id].p) return fail(c, CSI_ERR_NOT_BOUND, std::string("derived: field ") + slot_name(id) + " is requested but no array is bound to its slot");
        D.out[k] = ref_of(c, id);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    D.g = c->g;
    D.u = ref_of(c, CSI_F_U); D.v = ref_of(c, CSI_F_V);
    if (stress) { D.s11 = ref_of(c, CSI_F_S11); D.s22 = ref_of(c, CSI_F_S22); D.s12 = ref_of(c, CSI_F_S12); D.P = ref_of(c, CSI_F_P); }
    launch_derived(D, stress, c->stream);
    HIP_TRY(c, hipGetLastError());
    ++c->derived_launches;
    return CSI_OK;
}

int32_t csi_budget_compute(csi_context* c, int32_t what, csi_budget* out) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, CSI_ERR_INVALID_ARGUMENT, "budget: out == NULL");
    double slot[BQ_COUNT] = {};
    int32_t rc = peer_check_entry(c);
    if (!rc) rc = budget_local(c, what, slot);
    if ((rc = reduce_ranks(c, "budget", rc, BQ_COUNT, 0, BQ_COUNT, nullptr, slot))) return rc;
    const double nan = std::nan("");
    csi_budget b{};
    b.what = what;
    b.internal_work = b.stress_power = b.kinetic_energy = nan;
    if (what & CSI_BUDGET_STRESS) { b.internal_work = slot[BQ_WORK]; b.stress_power = slot[BQ_POWER]; }
    if (what & CSI_BUDGET_KINETIC) b.kinetic_energy = slot[BQ_KINETIC];
    *out = b;
    ++c->budget_calls;
    return CSI_OK;
}

int32_t csi_derived_stats(csi_context* c, int64_t* derived_launches, int64_t* budget_calls) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (derived_launches) *derived_launches = c->derived_launches;
    if (budget_calls) *budget_calls = c->budget_calls;
    return CSI_OK;
}

}
