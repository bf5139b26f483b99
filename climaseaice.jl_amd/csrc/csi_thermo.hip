// csi_thermo.hip -- the host side of the thermodynamics: the parameter structs as the kernels take them, the choice between the numeric
// kernels (thermo.hip) and the flux-term kernels (thermo_flux.hip) with the binding checks of the latter, the slab-ocean mixed layer's
// launch (mixed_layer.hip), and the entry points that set and step them (include/csi.h).  The time steppers (csi_abi.hip) call
// do_thermo.  See csi_ctx.h.
#include "csi_ctx.h"

namespace csi_host {

static SlabDev slab_dev(const csi_slab_params* p) {
    SlabDev S{};
    S.k = p->conductivity; S.rho_bulk = p->sea_ice_density; S.rho_pure = p->density; S.rho_l = p->liquid_density;
    S.c_l = p->liquid_heat_capacity; S.c_i = p->heat_capacity; S.L0 = p->reference_latent_heat; S.T0 = p->reference_temperature;
    S.liq_slope = p->liquidus_slope; S.liq_T0 = p->freshwater_melting_temperature; S.S = p->bottom_salinity;
    S.hc = p->ice_consolidation_thickness; S.Tu = p->top_temperature; S.Qu = p->top_heat_flux; S.Qb = p->bottom_heat_flux;
    S.top_flux_kind = p->top_flux_kind; S.bot_flux_kind = p->bottom_flux_kind;
    S.top_bc_kind = p->top_bc_kind; S.ice_salinity = p->ice_salinity;
    return S;
}
static SnowDev snow_dev(const csi_snow_params* p) {
    SnowDev W{};
    W.k = p->conductivity; W.rho = p->snow_density; W.snowfall = p->snowfall; W.Tu = p->top_temperature; W.top_bc_kind = p->top_bc_kind;
    return W;
}
// The flux-term path (thermo_flux.hip) runs once a side has terms, the prescribed temperature, the snowfall or the bottom salinity is
// an array, or a used-flux output is bound; its arrays are checked here.  `tu_id`: the surface whose temperature is solved / prescribed (CSI_F_TU bare ice, CSI_F_TUS snow).
static bool flux_path(const csi_context* c, bool snow) {
    const HeatFluxDev& F = c->heat;
    return F.top.n > 0 || F.bot.n > 0 || F.prescribed_array || (snow && F.snowfall_array) || F.bottom_salinity_array ||
           c->f[CSI_F_TOP_HEAT_FLUX_USED].p || c->f[CSI_F_BOTTOM_HEAT_FLUX_USED].p;
}
static bool has_array_term(const FluxTermsDev& t) {
    for (int k = 0; k < t.n; ++k)
        if (t.kind[k] == FLUX_ARRAY) return true;
    return false;
}
// `sw`: the SHORTWAVE term's setting as the kernels take it (mode SW_NONE unless the top's tuple has the term)
static int32_t flux_fields(csi_context* c, const SlabDev& S, int top_bc_kind, int tu_id, bool snow, FluxFields& ff, ShortwaveDev& sw) {
    const HeatFluxDev& F = c->heat;
    if (F.top.n > 0 && S.top_flux_kind != 0)
        return fail(c, CSI_ERR_UNSUPPORTED, "top heat-flux terms replace top_flux_kind 1 (the internal-flux equilibrium): set top_flux_kind 0");
    if (F.bot.n > 0 && S.bot_flux_kind != 0)
        return fail(c, CSI_ERR_UNSUPPORTED, "bottom heat-flux terms replace the frazil bottom_flux_kind 1: set bottom_flux_kind 0");
    if (F.prescribed_array && top_bc_kind != 0)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "csi_surface_solve.prescribed_array needs a PrescribedTemperature top (top_bc_kind 0)");
    ff = FluxFields{};
    std::vector<int> ids;
    if (has_array_term(F.top)) { ids.push_back(CSI_F_TOP_HEAT_FLUX); ff.qtop = ref_of(c, CSI_F_TOP_HEAT_FLUX); }
    if (has_array_term(F.bot)) { ids.push_back(CSI_F_BOTTOM_HEAT_FLUX); ff.qbot = ref_of(c, CSI_F_BOTTOM_HEAT_FLUX); }
    if (snow && F.snowfall_array) { ids.push_back(CSI_F_SNOWFALL); ff.snowfall = ref_of(c, CSI_F_SNOWFALL); }
    if (F.lin == LIN_ARRAYS) {
        ids.push_back(CSI_F_FLUX_COEFFICIENT); ff.lin_k = ref_of(c, CSI_F_FLUX_COEFFICIENT);
        ids.push_back(CSI_F_FLUX_REFERENCE_TEMPERATURE); ff.lin_ta = ref_of(c, CSI_F_FLUX_REFERENCE_TEMPERATURE);
    }
    if (F.bottom_salinity_array) { ids.push_back(CSI_F_BOTTOM_SALINITY); ff.sbot = ref_of(c, CSI_F_BOTTOM_SALINITY); }
    sw = ShortwaveDev{};
    if (c->heat_has_shortwave) {
        if (c->sw.mode == SW_NONE)
            return fail(c, CSI_ERR_INVALID_ARGUMENT, "a SHORTWAVE top heat-flux term needs csi_shortwave_set (the flux, the albedo and the weighting)");
        sw = c->sw;
        if (sw.mode == SW_CELL) { ids.push_back(CSI_F_SHORTWAVE); sw.f = ref_of(c, CSI_F_SHORTWAVE); }
        sw.albedo_used = ref_of(c, CSI_F_ALBEDO_USED);      // (unbound: p == nullptr)
    }
    // the surface temperature: read per cell (prescribed, Tu- of the secant), written by the flux balance
    if (flux_reads_surface_temperature(F, sw.mode, top_bc_kind)) ids.push_back(tu_id);
    for (int id : ids) {
        int32_t rc = need(c, {id});
        if (rc) return rc;
    }
    ff.tu = ref_of(c, tu_id);
    ff.qtop_used = ref_of(c, CSI_F_TOP_HEAT_FLUX_USED); ff.qbot_used = ref_of(c, CSI_F_BOTTOM_HEAT_FLUX_USED);      // (unbound: p == nullptr)
    return CSI_OK;
}
static int32_t do_layered(csi_context* c, const SlabDev& S, const SnowDev& W, double dt) {
    int32_t rc = need(c, {CSI_F_H, CSI_F_A, CSI_F_HS});
    if (rc) return rc;
    if (S.top_flux_kind != 0)
        return fail(c, CSI_ERR_UNSUPPORTED, "the layered (snow) step takes numbers, arrays and RadiativeEmission as top heat flux "
                                            "(top_flux_kind 0, csi_heat_fluxes_set), not the internal-flux equilibrium (top_flux_kind 1)");
    LayeredOut o{};
    o.mf_ice = ref_of(c, CSI_F_MASS_FLUX); o.mf_snow = ref_of(c, CSI_F_MASS_FLUX_SNOW); o.mf_int = ref_of(c, CSI_F_SNOWFALL_INTERCEPTED);
    o.tu_ice = ref_of(c, CSI_F_TU); o.tu_snow = ref_of(c, CSI_F_TUS);
    if (flux_path(c, true)) {
        FluxFields ff;
        ShortwaveDev sw;
        if ((rc = flux_fields(c, S, W.top_bc_kind, CSI_F_TUS, true, ff, sw))) return rc;
        c->last_thermo = launch_layered_flux_step(S, W, c->heat, ff, sw, c->g, ref_of(c, CSI_F_H), ref_of(c, CSI_F_A), ref_of(c, CSI_F_HS), o, dt, c->stream);
    } else {
        c->last_thermo = launch_layered_step(S, W, c->g, ref_of(c, CSI_F_H), ref_of(c, CSI_F_A), ref_of(c, CSI_F_HS), o, dt, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}
// thermodynamic_time_step!(model, ice_thermodynamics, snow_thermodynamics, dt): dispatch on the snow layer
static int32_t do_slab(csi_context* c, const SlabDev& S, double dt) {
    const bool has_mf = c->f[CSI_F_MASS_FLUX].p != nullptr;
    if (S.top_bc_kind == 1 && S.top_flux_kind != 0)
        return fail(c, CSI_ERR_UNSUPPORTED, "MeltingConstrainedFluxBalance takes numbers, arrays and RadiativeEmission as top heat flux "
                                            "(top_flux_kind 0, csi_heat_fluxes_set), not the internal-flux equilibrium (top_flux_kind 1)");
    if (flux_path(c, false)) {
        FluxFields ff;
        ShortwaveDev sw;
        int32_t rc = flux_fields(c, S, S.top_bc_kind, CSI_F_TU, false, ff, sw);
        if (rc) return rc;
        c->last_thermo = launch_slab_flux_step(S, c->heat, ff, sw, c->g, ref_of(c, CSI_F_H), ref_of(c, CSI_F_A), ref_of(c, CSI_F_MASS_FLUX), has_mf, dt, c->stream);
    } else {
        c->last_thermo = launch_slab_step(S, c->g, ref_of(c, CSI_F_H), ref_of(c, CSI_F_A), ref_of(c, CSI_F_MASS_FLUX), has_mf, dt, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}
// The slab-ocean mixed layer (include/csi.h csi_mixed_layer_set): one launch of k_mixed_layer, which writes To' and the bottom
// heat-flux array the ice step reads next.
static int32_t do_mixed_layer(csi_context* c, double dt, int from_cache) {
    if (!c->ml_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_mixed_layer_set has not been called");
    if (!c->slab_set)
        return fail(c, CSI_ERR_NOT_BOUND, "the mixed layer needs csi_slab_params_set (the liquidus and the bottom salinity of the ice thermodynamics)");
    const FluxTermsDev& bot = c->heat.bot;
    if (bot.n != 1 || bot.kind[0] != FLUX_ARRAY)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "the mixed layer needs exactly one ARRAY bottom heat-flux term (csi_heat_fluxes_set): it writes Qb "
                                                 "into the array bound to bottom_heat_flux");
    if (series_drives(c, CSI_F_BOTTOM_HEAT_FLUX))
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series on bottom_heat_flux: the mixed layer (csi_mixed_layer_set) writes that array at every step");
    if (!(dt > 0) || !std::isfinite(dt)) return fail(c, CSI_ERR_INVALID_ARGUMENT, "the mixed layer needs a finite dt > 0");
    const csi_mixed_layer_params& p = c->ml;
    int32_t rc = need(c, {CSI_F_ML_TEMPERATURE, CSI_F_A, CSI_F_BOTTOM_HEAT_FLUX});
    if (rc) return rc;
    if (from_cache && (rc = need(c, {CSI_F_ML_TEMPERATURE_M}))) return rc;
    MixedLayerFields F{};
    F.to_out = ref_of(c, CSI_F_ML_TEMPERATURE);
    F.to_in = from_cache ? ref_of(c, CSI_F_ML_TEMPERATURE_M) : F.to_out;
    F.a = ref_of(c, CSI_F_A);
    F.qb = ref_of(c, CSI_F_BOTTOM_HEAT_FLUX);
    if (p.flags & CSI_ML_SURFACE_ARRAY) {
        if ((rc = need(c, {CSI_F_ML_SURFACE_HEAT_FLUX}))) return rc;
        F.fo = ref_of(c, CSI_F_ML_SURFACE_HEAT_FLUX);
    }
    if (p.flags & CSI_ML_BULK_ARRAYS) {
        if ((rc = need(c, {CSI_F_ML_COEFFICIENT, CSI_F_ML_REFERENCE_TEMPERATURE}))) return rc;
        F.k = ref_of(c, CSI_F_ML_COEFFICIENT); F.ta = ref_of(c, CSI_F_ML_REFERENCE_TEMPERATURE);
    }
    if (p.flags & CSI_ML_DEEP_ARRAY) {
        if ((rc = need(c, {CSI_F_ML_DEEP_HEAT_FLUX}))) return rc;
        F.qd = ref_of(c, CSI_F_ML_DEEP_HEAT_FLUX);
    }
    if (c->heat.bottom_salinity_array) {
        if ((rc = need(c, {CSI_F_BOTTOM_SALINITY}))) return rc;
        F.sb = ref_of(c, CSI_F_BOTTOM_SALINITY);
    }
    F.qow = ref_of(c, CSI_F_ML_SURFACE_FLUX_USED);      // (unbound: p == nullptr)
    MixedLayerDev M{};
    M.rc = p.density * p.heat_capacity;
    M.C = M.rc * p.depth;
    M.grc = p.exchange_velocity * M.rc;
    M.Fo = p.surface_heat_flux; M.K = p.coefficient; M.Ta = p.reference_temperature; M.Qd = p.deep_heat_flux;
    M.liq_T0 = c->slab.liq_T0; M.liq_slope = c->slab.liq_slope; M.S = c->slab.S;
    M.dt = dt;
    M.has_surface = (p.flags & (CSI_ML_HAS_SURFACE | CSI_ML_SURFACE_ARRAY)) != 0;
    M.has_bulk = (p.flags & (CSI_ML_HAS_BULK | CSI_ML_BULK_ARRAYS)) != 0;
    M.nx = c->Nx; M.ny = c->Ny;
    launch_mixed_layer(M, F, c->stream);
    ++c->ml_launches;
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}
int32_t do_thermo(csi_context* c, double dt, int from_cache) {
    if (!c->slab_set) return CSI_OK;                       // thermodynamic_time_step!(model, ::Nothing, ...) = nothing
    int32_t rc;
    if (c->ml_set && (rc = do_mixed_layer(c, dt, from_cache))) return rc;      // the ocean under the ice first: it writes the bottom flux
    return c->snow_set ? do_layered(c, c->slab, c->snow, dt) : do_slab(c, c->slab, dt);
}

}  // namespace csi_host

extern "C" {

int32_t csi_slab_thermo_step(csi_context* c, const csi_slab_params* p, double dt) {
    if (!c || !p) return CSI_ERR_INVALID_ARGUMENT;
    int32_t rc = need(c, {CSI_F_H, CSI_F_A});
    if (rc) return rc;
    return do_slab(c, slab_dev(p), dt);
}

int32_t csi_layered_thermo_step(csi_context* c, const csi_slab_params* p, const csi_snow_params* w, double dt) {
    if (!c || !p || !w) return CSI_ERR_INVALID_ARGUMENT;
    return do_layered(c, slab_dev(p), snow_dev(w), dt);
}

int32_t csi_snow_params_set(csi_context* c, const csi_snow_params* p) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    c->snow_set = p != nullptr;
    if (p) c->snow = snow_dev(p);
    return CSI_OK;
}

int32_t csi_slab_params_set(csi_context* c, const csi_slab_params* p) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    c->slab_set = p != nullptr;
    if (p) c->slab = slab_dev(p);
    return CSI_OK;
}

int32_t csi_last_thermo(csi_context* c, int32_t* step, int32_t* shortwave, int32_t* index) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (step) *step = c->last_thermo.step;
    if (shortwave) *shortwave = c->last_thermo.sw;
    if (index) *index = c->last_thermo.index;
    return CSI_OK;
}

int32_t csi_mixed_layer_set(csi_context* c, const csi_mixed_layer_params* p) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!p) { c->ml_set = false; return CSI_OK; }
    const double values[8] = {p->density, p->heat_capacity, p->depth, p->exchange_velocity, p->surface_heat_flux, p->coefficient,
                              p->reference_temperature, p->deep_heat_flux};
    const char* const names[8] = {"density", "heat_capacity", "depth", "exchange_velocity", "surface_heat_flux", "coefficient",
                                  "reference_temperature", "deep_heat_flux"};
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(values[k])) return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("csi_mixed_layer_params.") + names[k] + " is not finite");
    for (int k = 0; k < 3; ++k)
        if (!(values[k] > 0)) return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("csi_mixed_layer_params.") + names[k] + " must be > 0");
    if (p->exchange_velocity < 0) return fail(c, CSI_ERR_INVALID_ARGUMENT, "csi_mixed_layer_params.exchange_velocity must be >= 0");
    if ((p->flags & ~(CSI_ML_SURFACE_ARRAY | CSI_ML_BULK_ARRAYS | CSI_ML_DEEP_ARRAY | CSI_ML_HAS_SURFACE | CSI_ML_HAS_BULK)) || p->reserved)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "csi_mixed_layer_params.flags: unknown flag bits (reserved must be 0)");
    if (series_drives(c, CSI_F_BOTTOM_HEAT_FLUX))
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "time series on bottom_heat_flux: the mixed layer (csi_mixed_layer_set) writes that array at every step");
    c->ml = *p;
    c->ml_set = true;
    return CSI_OK;
}

int32_t csi_mixed_layer_step(csi_context* c, double dt, int32_t from_cache) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    return do_mixed_layer(c, dt, from_cache != 0);
}

int32_t csi_mixed_layer_stats(csi_context* c, int64_t* launches) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (launches) *launches = c->ml_launches;
    return CSI_OK;
}

int32_t csi_heat_fluxes_set(csi_context* c, int32_t side, const csi_heat_flux_term* terms, int32_t n) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (side != CSI_HEAT_TOP && side != CSI_HEAT_BOTTOM) return fail(c, CSI_ERR_INVALID_ARGUMENT, "side must be CSI_HEAT_TOP or CSI_HEAT_BOTTOM");
    if (!terms) n = 0;
    if (n < 0) return fail(c, CSI_ERR_INVALID_ARGUMENT, "n < 0");
    if (n > CSI_MAX_HEAT_FLUX_TERMS)
        return fail(c, CSI_ERR_UNSUPPORTED, "more than CSI_MAX_HEAT_FLUX_TERMS heat-flux terms on one side");
    FluxTermsDev t{};
    int arrays = 0, lin = LIN_NONE, lin_weight = WEIGHT_NONE, shortwave = 0;
    for (int k = 0; k < n; ++k) {
        const csi_heat_flux_term& q = terms[k];
        if (q.kind != CSI_FLUX_CONSTANT && q.kind != CSI_FLUX_ARRAY && q.kind != CSI_FLUX_RADIATIVE_EMISSION && q.kind != CSI_FLUX_LINEAR &&
            q.kind != CSI_FLUX_SHORTWAVE)
            return fail(c, CSI_ERR_INVALID_ARGUMENT, "unknown heat-flux term kind");
        if (q.kind == CSI_FLUX_SHORTWAVE) {
            if (side != CSI_HEAT_TOP) return fail(c, CSI_ERR_UNSUPPORTED, "ShortwaveRadiation is a top heat flux only");
            if (++shortwave > 1) return fail(c, CSI_ERR_UNSUPPORTED, "at most one ShortwaveRadiation term per model (sum the fluxes into one)");
            if (c->sw.mode == SW_NONE)
                return fail(c, CSI_ERR_INVALID_ARGUMENT, "a SHORTWAVE top heat-flux term needs csi_shortwave_set (the flux, the albedo and the weighting) first");
        }
        if (q.kind == CSI_FLUX_LINEAR) {
            if (side != CSI_HEAT_TOP) return fail(c, CSI_ERR_UNSUPPORTED, "LinearHeatFlux is a top heat flux only");
            if (lin != LIN_NONE) return fail(c, CSI_ERR_UNSUPPORTED, "at most one LinearHeatFlux term per model (sum the coefficients into one)");
            const int per_cell = q.reserved & (CSI_LINEAR_COEFFICIENT_ARRAY | CSI_LINEAR_REFERENCE_ARRAY);
            lin_weight = q.reserved & CSI_LINEAR_WEIGHT_MASK;
            if ((q.reserved & ~(CSI_LINEAR_WEIGHT_MASK | CSI_LINEAR_COEFFICIENT_ARRAY | CSI_LINEAR_REFERENCE_ARRAY)) || lin_weight > CSI_WEIGHT_ICE_PRESENT)
                return fail(c, CSI_ERR_INVALID_ARGUMENT, "LinearHeatFlux: unknown weighting or flag in csi_heat_flux_term.reserved");
            if (per_cell != 0 && per_cell != (CSI_LINEAR_COEFFICIENT_ARRAY | CSI_LINEAR_REFERENCE_ARRAY))
                return fail(c, CSI_ERR_UNSUPPORTED, "LinearHeatFlux: the coefficient and the reference temperature are both numbers or both per cell "
                                                    "(broadcast the number into an array)");
            lin = per_cell ? LIN_ARRAYS : LIN_NUMBERS;
        }
        if (q.kind == CSI_FLUX_ARRAY && ++arrays > 1)
            return fail(c, CSI_ERR_UNSUPPORTED, "at most one ARRAY heat-flux term per side (sum the arrays into one)");
        if (q.kind == CSI_FLUX_RADIATIVE_EMISSION && side != CSI_HEAT_TOP)
            return fail(c, CSI_ERR_UNSUPPORTED, "RadiativeEmission is a top heat flux only");
        t.kind[k] = q.kind == CSI_FLUX_ARRAY ? FLUX_ARRAY : (q.kind == CSI_FLUX_RADIATIVE_EMISSION ? FLUX_EMISSION :
                    (q.kind == CSI_FLUX_LINEAR ? FLUX_LINEAR : (q.kind == CSI_FLUX_SHORTWAVE ? FLUX_SHORTWAVE : FLUX_CONST)));
        t.value[k] = q.value;
        t.eps[k] = q.emissivity; t.sigma[k] = q.stefan_boltzmann_constant; t.Tr[k] = q.reference_temperature;
    }
    t.n = n;
    (side == CSI_HEAT_TOP ? c->heat.top : c->heat.bot) = t;
    if (side == CSI_HEAT_TOP) { c->heat.lin = lin; c->heat.lin_weight = lin_weight; c->heat_has_shortwave = shortwave != 0; }
    return CSI_OK;
}

int32_t csi_shortwave_set(csi_context* c, const csi_shortwave* p) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    if (!p) { c->sw = ShortwaveDev{}; return CSI_OK; }
    const double values[7] = {p->flux, p->cold, p->warm, p->threshold, p->snow_cold, p->snow_warm, p->snow_threshold};
    const char* const names[7] = {"flux", "cold", "warm", "threshold", "snow_cold", "snow_warm", "snow_threshold"};
    for (int k = 0; k < (p->has_snow_pair ? 7 : 4); ++k) {
        if (!std::isfinite(values[k])) return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("csi_shortwave.") + names[k] + " is not finite");
        if (k != 0 && k != 3 && k != 6 && !(values[k] >= 0 && values[k] <= 1))
            return fail(c, CSI_ERR_INVALID_ARGUMENT, std::string("csi_shortwave.") + names[k] + ": an albedo lies in [0, 1]");
    }
    if (p->weighting < CSI_WEIGHT_NONE || p->weighting > CSI_WEIGHT_ICE_PRESENT)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "csi_shortwave.weighting: unknown weighting");
    if ((p->per_cell & ~1) || (p->has_snow_pair & ~1) || p->reserved)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "csi_shortwave: per_cell and has_snow_pair are 0 or 1, reserved must be 0");
    if (p->per_cell && !c->f[CSI_F_SHORTWAVE].p)
        return fail(c, CSI_ERR_INVALID_ARGUMENT, "csi_shortwave.per_cell: no array is bound to CSI_F_SHORTWAVE (csi_field_bind it first)");
    ShortwaveDev w{};
    w.mode = p->per_cell ? SW_CELL : SW_NUMBER;
    w.weight = p->weighting; w.snow_pair = p->has_snow_pair;
    w.F = p->per_cell ? 0.0 : p->flux;
    w.cold = p->cold; w.warm = p->warm; w.thr = p->threshold;
    if (p->has_snow_pair) { w.snow_cold = p->snow_cold; w.snow_warm = p->snow_warm; w.snow_thr = p->snow_threshold; }
    c->sw = w;
    return CSI_OK;
}

int32_t csi_surface_solve_set(csi_context* c, const csi_surface_solve* p) {
    if (!c) return CSI_ERR_INVALID_ARGUMENT;
    const HeatFluxDev defaults{};
    if (!p) {
        c->heat.tol = defaults.tol; c->heat.maxiters = defaults.maxiters;
        c->heat.prescribed_array = 0; c->heat.snowfall_array = 0; c->heat.bottom_salinity_array = 0;
        return CSI_OK;
    }
    if (!(p->tol > 0) || p->maxiters < 1) return fail(c, CSI_ERR_INVALID_ARGUMENT, "the surface solve needs tol > 0 and maxiters >= 1");
    c->heat.tol = p->tol; c->heat.maxiters = p->maxiters;
    if (p->reserved & ~CSI_SOLVE_BOTTOM_SALINITY_ARRAY) return fail(c, CSI_ERR_INVALID_ARGUMENT, "csi_surface_solve.reserved: unknown flag");
    c->heat.prescribed_array = p->prescribed_array != 0; c->heat.snowfall_array = p->snowfall_array != 0;
    c->heat.bottom_salinity_array = (p->reserved & CSI_SOLVE_BOTTOM_SALINITY_ARRAY) != 0;
    return CSI_OK;
}

}  // extern "C"
