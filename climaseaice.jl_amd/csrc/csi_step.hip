// csi_step.hip -- whole steps: the checks both steppers open with, ONE step stage, the one-launch-per-stage RK3 step of an advection-only
// model, cache_current_fields!.  The entry points (csi_time_step_fe / _rk3, csi_cache_current_fields) are in csi_abi.hip.  Replaces the
// host side of the reference's
//   time_step!(::FESeaIceModel)   sea_ice_fe_step.jl:13-34
//   rk_substep! / cache_current_fields! / dynamic_time_step!   sea_ice_rk_substep.jl:29-152
// See csi_ctx.h.
#include "csi_ctx.h"

namespace csi_host {

// What both steppers check before they write anything.  dynamics = nothing (csi_evp_params_set never called, no
// csi_dynamics_set(ctx, CSI_DYNAMICS_FREE_DRIFT)): prescribed velocities, time_step_momentum! is a no-op (SeaIceDynamics.jl:40) -- the
// advection-only models of examples/ice_advected_by_anticyclone.jl's family.  rk3: the Psi^- slots as well.
// Every path of a whole step ends by imaging h, aice [, hs] (update_state!, or the tracer update's own stores) and, with dynamics, u and
// v: a grid too narrow for one image per side (fill_width_check) is refused HERE, before the step has written anything -- not at its end,
// and also where the fused stores would have skipped update_state!'s check.
int32_t step_checks(csi_context* c, bool dynamics, bool rk3) {
    int32_t rc = dynamics ? need_momentum(c) : need(c, {CSI_F_H, CSI_F_A});
    if (rc) return rc;
    if (rk3 && (rc = dynamics ? need(c, {CSI_F_HM, CSI_F_AM, CSI_F_UM, CSI_F_VM}) : need(c, {CSI_F_HM, CSI_F_AM}))) return rc;
    if ((rc = fill_width_check(c, CSI_F_H))) return rc;          // (aice, hs: the same location)
    if (dynamics && ((rc = fill_width_check(c, CSI_F_U)) || (rc = fill_width_check(c, CSI_F_V)))) return rc;
    if (rk3 && c->ml_set && c->slab_set && (rc = need(c, {CSI_F_ML_TEMPERATURE, CSI_F_ML_TEMPERATURE_M}))) return rc;
    return CSI_OK;
}

// One stage: the whole forward-Euler step (from_cache 0; sea_ice_fe_step.jl, the first line numbers) or one RK3 stage with its dt / beta
// (from_cache 1: from Psi^-, the velocities reset to u^-; sea_ice_rk_substep.jl, the second)
int32_t step_stage(csi_context* c, double dt, int substeps, int scheme, bool dynamics, int from_cache) {
    int32_t rc;
    if ((rc = do_tendencies_or_zero(c, scheme))) return rc;                              // :19 / :84 (compute_tracer_tendencies!)
    if (c->trc.set && (rc = tracers_first_half(c, scheme, dt, from_cache))) return rc;   // (advected tracers: the first half, include/csi.h)
    if (dynamics && (rc = do_momentum_tendencies(c, dt))) return rc;                     // :19 / :84 (compute_momentum_tendencies!: ExplicitSolver only)
    if (dynamics && (rc = do_momentum(c, dt, substeps, from_cache))) return rc;          // :22 / :87
    // without a mask and without a thermodynamic step the tracer update's stores write the halo images themselves
    const bool fused_fill = !c->g.has_mask && !c->slab_set;
    if ((rc = do_tracer_step(c, dt, from_cache, fused_fill))) return rc;                 // :25 / :89
    if ((rc = do_thermo(c, dt, from_cache))) return rc;                                  // :28 / :91 thermodynamic_time_step! (the mixed layer: from Psi^-)
    if (c->trc.set && (rc = tracers_second_half(c, dt))) return rc;                      // (advected tracers: the second half)
    return do_update_state(c, true, fused_fill);                                         // :31
}

// An RK3 step of an advection-only model (prescribed velocities: examples/ice_advected_by_anticyclone.jl's family, BASELINE
// config 2) with ONE launch per stage: nothing happens between a stage's tendencies and its tracer update, so the kernel that
// computes G also applies it -- into another copy of (h, a), because its neighbours still read the stage's input: the state
// rotates bound arrays -> copy 1 -> copy 2 -> bound arrays.  The first stage also writes Psi^- (cache_current_fields!).  Same
// arithmetic as the separate kernels, statement for statement: bit-identical (tests/test_gpu_steps.py).
// (A scheme that is unknown or does not fit the halo declines the path: the general stage loop reports it.)
bool advect_stage_supported(const csi_context* c, int scheme) {
    const ImageSpec im = image_spec(c, CSI_F_H);
    for (int side : {im.xlo, im.xhi, im.ylo, im.yhi}) if (side != IMG_WRAP && side != IMG_MIRROR) return false;      // (periodic / no-flux walls)
    if (c->Nx < 2 * c->Hx || c->Ny < 2 * c->Hy) return false;
    // Round 3 cut this path off above 3 M cells (2048^2: 768 -> 794 us per RK3 step with it).  Re-measured in round 6 with two tracers
    // per thread and the round-5 block shapes (scripts/ab_adv_stage.sh, profiles/r06_advection_stage_ab.txt; WENO7, us per RK3 step,
    // separate launches -> one per stage): 1536^2 314 -> 264, 2048^2 538 -> 476, 3072^2 1205 -> 988, 4096^2 2110 -> 1711 -- the
    // separate update streams another 7 arrays per stage, which the fused stage never touches: no cut any more (A/B knob:
    // CSI_ADV_STAGE_MAX_CELLS)
    if ((long)c->Nx * c->Ny > c->tune.adv_stage_max_cells) return false;
    if (c->trc.set) return false;      // (advected tracers take the general stage loop)
    return !has_dynamics(c) && scheme != 0 && c->fusion && !c->slab_set && !c->g.has_mask && !is_tiled(c) &&
           c->f[CSI_F_HS].p == nullptr && c->f[CSI_F_H].ld == c->f[CSI_F_HM].ld && c->f[CSI_F_A].ld == c->f[CSI_F_AM].ld && advect_fits(c, scheme);
}
int32_t rk3_advection_only(csi_context* c, double dt, int scheme) {
    int32_t rc;
    if ((rc = need(c, {CSI_F_U, CSI_F_V, CSI_F_H, CSI_F_A, CSI_F_GH, CSI_F_GA, CSI_F_HM, CSI_F_AM}))) return rc;
    for (ScratchField& s : c->adv_buf) {
        bool fresh;
        HIP_TRY(c, s.ensure(c, nullptr, &fresh));
        // beyond walls the halo holds mirror images the stores rewrite; cells nobody writes (wall corners) start as the state's
        if (fresh) HIP_TRY(c, hipMemcpyAsync(s.get(), c->f[s.fid].p, s.buf.size() * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    const FRef H0 = ref_of(c, CSI_F_H), A0 = ref_of(c, CSI_F_A), H1 = c->adv_buf[0].view(c), A1 = c->adv_buf[1].view(c),
               H2 = c->adv_buf[2].view(c), A2 = c->adv_buf[3].view(c);
    const FRef hin[3] = {H0, H1, H2}, ain[3] = {A0, A1, A2}, hout[3] = {H1, H2, H0}, aout[3] = {A1, A2, A0};
    int stage = 0;
    for (int beta = 3; beta >= 1; --beta, ++stage) {
        AdvDev A = adv_dev(c, scheme, dt / beta, 1);
        A.h = hin[stage]; A.a = ain[stage];
        A.hb = stage == 0 ? H0 : A.hm; A.ab = stage == 0 ? A0 : A.am;
        A.ho = hout[stage]; A.ao = aout[stage];
        A.write_cache = stage == 0;
        A.fill_images = 1;
        c->last_adv = launch_advect_stage(A, c->mode, c->stream);
        c->last_adv_stage = 1;
        HIP_TRY(c, hipGetLastError());
    }
    return CSI_OK;
}

// cache_current_fields! (sea_ice_rk_substep.jl:29-42): Psi^- = the prognostic fields, whole parents, in one launch
int32_t cache_current_fields(csi_context* c) {
    int32_t rc = need(c, {CSI_F_H, CSI_F_A, CSI_F_HM, CSI_F_AM});
    if (rc) return rc;
    CopyBatch B = copy_batch_aligned();
    auto add = [&](int dst, int src) -> int32_t {
        const Bound &d = c->f[dst], &q = c->f[src];
        if (d.ld != q.ld || d.nj != q.nj) return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("parent shape mismatch: ") + slot_name(dst) + " vs " + slot_name(src));
        copy_add(B, q.p, d.p, (long)d.ld * d.nj);
        return CSI_OK;
    };
    if ((rc = add(CSI_F_HM, CSI_F_H))) return rc;
    if ((rc = add(CSI_F_AM, CSI_F_A))) return rc;
    if (c->f[CSI_F_HS].p && c->f[CSI_F_HSM].p && (rc = add(CSI_F_HSM, CSI_F_HS))) return rc;
    if (c->f[CSI_F_U].p && c->f[CSI_F_UM].p) {
        if ((rc = need(c, {CSI_F_V, CSI_F_VM}))) return rc;
        if ((rc = add(CSI_F_UM, CSI_F_U))) return rc;
        if ((rc = add(CSI_F_VM, CSI_F_V))) return rc;
    }
    // (the mixed-layer temperature is a prognostic field of the step like h and aice: the sixth and last entry of the batch)
    if (c->f[CSI_F_ML_TEMPERATURE].p && c->f[CSI_F_ML_TEMPERATURE_M].p && (rc = add(CSI_F_ML_TEMPERATURE_M, CSI_F_ML_TEMPERATURE))) return rc;
    launch_copy_batch(B, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (c->trc.set && (rc = tracers_cache(c))) return rc;      // (advected tracers: c -> c^-, a batch of their own)
    return CSI_OK;
}

}  // namespace csi_host
