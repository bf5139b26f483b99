// csi_momentum.hip -- the rheology / momentum-solver dispatch: ViscousRheology's split-explicit sub-cycle and the ExplicitSolver
// (include/csi.h csi_rheology_set, csi_momentum_solver_set; kernels in momentum_viscous.hip / momentum_explicit.hip).  EVP with the
// split-explicit solver goes on through need_evp / do_time_step_momentum (csi_launch.hip), untouched.  See csi_ctx.h.
#include "csi_ctx.h"

namespace csi_host {

static const char* rheology_name(int k) { return k == CSI_RHEOLOGY_VISCOUS ? "ViscousRheology" : "ElastoViscoPlasticRheology"; }
static const char* solver_name(int k) { return k == CSI_SOLVER_EXPLICIT ? "ExplicitSolver" : "SplitExplicitSolver"; }

// Tiles and north folds run EVP with the split-explicit solver only (the reference's distributed and tripolar tests use nothing else)
int32_t momentum_config_check(csi_context* c) {
    if (c->rheology == CSI_RHEOLOGY_EVP && c->solver == CSI_SOLVER_SPLIT_EXPLICIT) return CSI_OK;
    if (!c->grid_set) return CSI_OK;
    const bool fold = c->g.yhi == SIDE_FOLD;
    if (is_tiled(c) || c->tile.set || fold) {
        const char* what = c->rheology != CSI_RHEOLOGY_EVP ? rheology_name(c->rheology) : solver_name(c->solver);
        return fail(c, CSI_ERR_UNSUPPORTED, std::string(what) + " is not supported on " + (fold ? "north-fold (tripolar)" : "tiled") +
                                                " grids: only ElastoViscoPlasticRheology with the SplitExplicitSolver runs there");
    }
    return CSI_OK;
}

// need_evp without the ten auxiliary slots: what every rheology needs (the checks after the slots are need_dynamics_common's, shared
// with need_evp)
static int32_t need_dynamics(csi_context* c) {
    int32_t rc = need(c, {CSI_F_U, CSI_F_V, CSI_F_H, CSI_F_A});
    if (rc) return rc;
    if (c->evp_set && (rc = momentum_config_check(c))) return rc;
    return need_dynamics_common(c);
}

// StressBalanceFreeDrift as the model's dynamics (csi_dynamics_set): u, v, the grid and the two stresses -- none of the EVP slots, no
// csi_evp_params, no rheology / solver / free-drift-kind setting
static int32_t need_free_drift_dynamics(csi_context* c) {
    int32_t rc = need(c, {CSI_F_U, CSI_F_V});
    if (rc) return rc;
    // stress_balance_free_drift.jl:24-32, the constructor's two errors
    const bool ts = c->stress[CSI_STRESS_TOP].kind == CSI_STRESS_SEMI_IMPLICIT, bs = c->stress[CSI_STRESS_BOTTOM].kind == CSI_STRESS_SEMI_IMPLICIT;
    if (ts && bs)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "`StressBalanceFreeDrift` supports a `SemiImplicitStress` only for the `top_momentum_stress` or the `bottom_momentum_stress`, not both");
    if (!ts && !bs)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "`StressBalanceFreeDrift` requires using a `SemiImplicitStress` for either the `top_momentum_stress` or the `bottom_momentum_stress`");
    if ((rc = check_stress_fields(c, CSI_STRESS_TOP))) return rc;
    if ((rc = check_stress_fields(c, CSI_STRESS_BOTTOM))) return rc;
    if (c->Hx < 1 || c->Hy < 1) return fail(c, CSI_ERR_INVALID_ARGUMENT, "the free-drift step needs halo >= 1");      // the four-point averages reach one cell
    if (c->Nx < c->Hx || c->Ny < c->Hy) return fail(c, CSI_ERR_UNSUPPORTED, "tile smaller than its halo");
    if (is_tiled(c) && !c->tile.set) return fail(c, CSI_ERR_NOT_BOUND, "connected topology but csi_tile_set has not been called");
    return CSI_OK;
}

int32_t need_momentum(csi_context* c) {
    if (c->dynamics == CSI_DYNAMICS_FREE_DRIFT) return need_free_drift_dynamics(c);
    if (c->rheology == CSI_RHEOLOGY_EVP && c->solver == CSI_SOLVER_SPLIT_EXPLICIT) return need_evp(c);
    int32_t rc = need_dynamics(c);
    if (rc) return rc;
    // the explicit step with EVP reads the stored sigma, u^n and alpha: the EVP slots
    if (c->rheology == CSI_RHEOLOGY_EVP && (rc = need_evp(c))) return rc;
    if (c->solver == CSI_SOLVER_EXPLICIT && (rc = need(c, {CSI_F_GU, CSI_F_GV}))) return rc;
    if ((c->f[CSI_F_FORCING_U].p != nullptr) != (c->f[CSI_F_FORCING_V].p != nullptr))
        return fail(c, CSI_ERR_NOT_BOUND, "model.forcing arrays: bind both CSI_F_FORCING_U and CSI_F_FORCING_V or neither");
    return CSI_OK;
}

// StressBalanceFreeDrift: the free-drift velocities of marginal ice depend on the forcing only -- once per sub-cycle (EVP: do_subcycle)
// or step into library arrays, at every point whose four-point averages stay inside the parent arrays.  (A launch error surfaces at
// the caller's hipGetLastError.)
// free_drift = (u, v) (CSI_FREE_DRIFT_FIELDS): nothing to do -- evp_dev points P.ufd / P.vfd at the bound arrays, whose halos
// update_external_stress has filled.
int32_t free_drift_fields(csi_context* c, double dt) {
    if (c->free_drift != CSI_FREE_DRIFT_STRESS_BALANCE) return CSI_OK;
    for (ScratchField& f : c->fd) HIP_TRY(c, f.ensure(c));
    launch_free_drift(evp_dev(c, dt), Range{2 - c->Hx, c->Nx + c->Hx - 1, 2 - c->Hy, c->Ny + c->Hy - 1}, c->stream);
    return CSI_OK;
}

// reset_velocities! (split_explicit_momentum_equations.jl:89-93): an RK stage starts from u^-, v^-
int32_t reset_velocities(csi_context* c) {
    int32_t rc;
    if ((rc = need(c, {CSI_F_UM, CSI_F_VM}))) return rc;
    if ((rc = copy_parent(c, CSI_F_U, CSI_F_UM))) return rc;
    return copy_parent(c, CSI_F_V, CSI_F_VM);
}

// update_external_stress! (split_explicit_momentum_equations.jl:133-134): local halos of the stress / forcing arrays
int32_t fill_forcing_halos(csi_context* c) {
    int32_t rc;
    for (int id : slots_with(SLOT_FORCING))
        if (c->f[id].p && (rc = fill_halo(c, id))) return rc;
    return CSI_OK;
}

// ... and, on tiles, the neighbours' values beyond the connected sides: inside an exchange batch the velocity kernels run on ranges
// that reach into the halo and read the forcing / free-drift value there, and the four-point averages of the stresses cross the sides
int32_t update_external_stress(csi_context* c) {
    int32_t rc;
    if ((rc = fill_forcing_halos(c))) return rc;
    if (is_tiled(c)) {
        // (every rank binds the same slots, so every rank issues the same batches: one exchange takes at most MAX_EX_FIELDS fields,
        //  which the six older slots fill; with the two free-drift fields on top of them a second batch follows)
        int ff[8], n = 0;
        for (int id : slots_with(SLOT_FORCING)) if (c->f[id].p) ff[n++] = id;
        const int W = c->Hx < c->Hy ? c->Hx : c->Hy;
        for (int at = 0; at < n; at += MAX_EX_FIELDS)
            if ((rc = exchange(c, ff + at, std::min(n - at, MAX_EX_FIELDS), W))) return rc;
    }
    return CSI_OK;
}

static MomDev mom_dev(const csi_context* c, double dt) {
    MomDev M{};
    M.P = evp_dev(c, dt);
    M.nu = c->nu;
    M.Gu = ref_of(c, CSI_F_GU);
    M.Gv = ref_of(c, CSI_F_GV);
    return M;
}

// ---- ViscousRheology, split-explicit (split_explicit_momentum_equations.jl:103-195 with Rheologies.jl:42-55) ----------------
static int32_t viscous_subcycle(csi_context* c, double dt, int substeps, int rk_reset) {
    int32_t rc;
    if (rk_reset && (rc = reset_velocities(c))) return rc;
    if ((rc = fill_forcing_halos(c))) return rc;           // :133-134 (initialize_rheology!: nothing)
    launch_fill_halo_batch(halo_batch(c, {CSI_F_U, CSI_F_V}), c->g, c->stream);      // :170-171
    if ((rc = free_drift_fields(c, dt))) return rc;
    // the second array of each component.  A launch rewrites every interior point and the halo images of its stores; what no store
    // reaches (halos beyond walls, deeper layers of a ValueBoundaryCondition side) must agree in both arrays: copied once, unless every
    // cell is an image (doubly periodic)
    const int comp[2] = {CSI_F_U, CSI_F_V};
    for (ScratchField& a : c->vis_alt) HIP_TRY(c, a.ensure(c));
    const bool every_cell_imaged = c->g.xlo == SIDE_PERIODIC && c->g.xhi == SIDE_PERIODIC && c->g.ylo == SIDE_PERIODIC && c->g.yhi == SIDE_PERIODIC;
    if (!every_cell_imaged && substeps > 0) {
        CopyBatch B = copy_batch_aligned();
        for (int q = 0; q < 2; ++q) copy_add(B, c->f[comp[q]].p, c->vis_alt[q].get(), (long)c->f[comp[q]].ld * c->f[comp[q]].nj);
        launch_copy_batch(B, c->stream);
    }
    FRef bound[2], alt[2];
    for (int q = 0; q < 2; ++q) {
        bound[q] = ref_of(c, comp[q]);
        alt[q] = c->vis_alt[q].view(c);
    }
    MomDev M = mom_dev(c, dt / substeps);                   // Delta tau = Delta t / substeps (Rheologies.jl:48-49)
    const ImageSpec imu = image_spec(c, CSI_F_U), imv = image_spec(c, CSI_F_V);
    const Range r = interior_range(c);
    const int fast = c->mode == CSI_MODE_FAST;
    int cur[2] = {0, 0};                                    // 0: the bound array holds the component's current values
    auto step = [&](int q) {
        M.P.u = cur[0] ? alt[0] : bound[0];
        M.P.v = cur[1] ? alt[1] : bound[1];
        M.out = cur[q] ? bound[q] : alt[q];
        if (q == 0) launch_viscous_ustep(M, r, imu, fast, c->stream);
        else launch_viscous_vstep(M, r, imv, fast, c->stream);
        cur[q] ^= 1;
    };
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    for (int s = 1; s <= substeps; ++s) {
        if (s % 2 == 0) { step(0); step(1); }               // :178-182
        else { step(1); step(0); }                          // :184-187
    }
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    if (cur[0] | cur[1]) {                                  // one copy back: the components whose result sits in the scratch
        CopyBatch B = copy_batch_aligned();
        for (int q = 0; q < 2; ++q)
            if (cur[q]) copy_add(B, c->vis_alt[q].get(), c->f[comp[q]].p, (long)c->f[comp[q]].ld * c->f[comp[q]].nj);
        launch_copy_batch(B, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
    c->last = csi_context::LastPath{true, 0, 2, 2 * substeps, substeps, 0, 1};
    return CSI_OK;                                          // finalize_rheology!: nothing
}

// ---- ExplicitSolver (explicit_momentum_equations.jl) ---------------------------------------------------------------------------
int32_t do_momentum_tendencies(csi_context* c, double dt) {
    if (c->solver != CSI_SOLVER_EXPLICIT || c->dynamics == CSI_DYNAMICS_FREE_DRIFT) return CSI_OK;     // SplitExplicitSolver: compute_momentum_tendencies! is nothing
    MomDev M = mom_dev(c, dt);
    launch_explicit_tendencies(M, interior_range(c), c->rheology == CSI_RHEOLOGY_VISCOUS, c->mode == CSI_MODE_FAST, c->stream);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

static int32_t explicit_step(csi_context* c, double dt, int rk_reset) {
    int32_t rc;
    if (rk_reset && (rc = need(c, {CSI_F_UM, CSI_F_VM}))) return rc;
    if ((rc = fill_forcing_halos(c))) return rc;
    if ((rc = free_drift_fields(c, dt))) return rc;
    MomDev M = mom_dev(c, dt);
    M.um = rk_reset ? ref_of(c, CSI_F_UM) : M.P.u;          // previous_velocities, :3-5
    M.vm = rk_reset ? ref_of(c, CSI_F_VM) : M.P.v;
    const Range r = interior_range(c);
    const int fast = c->mode == CSI_MODE_FAST;
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    M.out = M.P.u;
    launch_explicit_ustep(M, r, image_spec(c, CSI_F_U), fast, c->stream);     // :31-32
    M.out = M.P.v;
    launch_explicit_vstep(M, r, image_spec(c, CSI_F_V), fast, c->stream);     // :34-35
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    HIP_TRY(c, hipGetLastError());
    c->last = csi_context::LastPath{true, 0, 2, 2, 1, 0, 1};      // (two launches: the tendency launch belongs to csi_compute_momentum_tendencies)
    return CSI_OK;
}

// ---- StressBalanceFreeDrift as the dynamics (stress_balance_free_drift.jl:131-151): one launch, u and v with their halo images ------
static int32_t free_drift_dynamics_step(csi_context* c) {
    int32_t rc;
    if ((rc = peer_check_entry(c))) return rc;
    if ((rc = update_external_stress(c))) return rc;        // the stress arrays' halos: the four-point averages reach one cell
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    // the ranges and images of the EVP three-kernel velocity steps for u and v: the owned points, every side's local images
    launch_free_drift_step(evp_dev(c, 0.0), interior_range(c), image_spec(c, CSI_F_U), image_spec(c, CSI_F_V), c->stream);
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    HIP_TRY(c, hipGetLastError());
    c->last = csi_context::LastPath{true, 0, 1, 1, 1, 0, 1};
    c->peer.last = 0;
    return CSI_OK;
}

int32_t do_momentum(csi_context* c, double dt, int substeps, int rk_reset) {
    if (c->dynamics == CSI_DYNAMICS_FREE_DRIFT) return free_drift_dynamics_step(c);      // (no dt, no sub-steps, no u^-)
    if (c->solver == CSI_SOLVER_EXPLICIT) return explicit_step(c, dt, rk_reset);
    if (c->rheology == CSI_RHEOLOGY_VISCOUS) return viscous_subcycle(c, dt, substeps, rk_reset);
    return do_time_step_momentum(c, dt, substeps, rk_reset);
}

}  // namespace csi_host

extern "C" {

int32_t csi_rheology_set(csi_context* c, int32_t kind, double nu) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (kind != CSI_RHEOLOGY_EVP && kind != CSI_RHEOLOGY_VISCOUS) return fail(c, CSI_ERR_INVALID_ARGUMENT, "unknown rheology kind");
    if (kind == CSI_RHEOLOGY_VISCOUS && !std::isfinite(nu)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "ViscousRheology: nu must be a finite number");
    const int old = c->rheology;
    c->rheology = kind;
    int32_t rc = momentum_config_check(c);
    if (rc) { c->rheology = old; return rc; }
    if (kind == CSI_RHEOLOGY_VISCOUS) c->nu = nu;
    return CSI_OK;
}

int32_t csi_momentum_solver_set(csi_context* c, int32_t kind) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (kind != CSI_SOLVER_SPLIT_EXPLICIT && kind != CSI_SOLVER_EXPLICIT) return fail(c, CSI_ERR_INVALID_ARGUMENT, "unknown momentum solver kind");
    const int old = c->solver;
    c->solver = kind;
    int32_t rc = momentum_config_check(c);
    if (rc) { c->solver = old; return rc; }
    return CSI_OK;
}

int32_t csi_compute_momentum_tendencies(csi_context* c, double dt) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (c->solver != CSI_SOLVER_EXPLICIT || c->dynamics == CSI_DYNAMICS_FREE_DRIFT) return CSI_OK;      // (free-drift dynamics: SeaIceDynamics.jl:41)
    int32_t rc = need_momentum(c);
    if (rc) return rc;
    return do_momentum_tendencies(c, dt);
}

}  // extern "C"
