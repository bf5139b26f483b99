// thermo.hip -- bare-ice slab thermodynamic step (plumbing: configs 1 and 4 of BASELINE.json).
//
//   k_slab  _ice_thermodynamic_time_step!  SeaIceThermodynamics/thermodynamic_time_step.jl:75-118
//           with thermodynamic_tendency / ice_melt_freeze_tendency
//           (slab_thermodynamics_tendencies.jl:28-135, PrescribedTemperature top BC),
//           ice_volume_update (:304-324), concentration_thermodynamic_step (:358-370),
//           latent_heat (SeaIceThermodynamics.jl:161-170), slab_internal_heat_flux
//           (slab_heat_and_tracer_fluxes.jl:8-19).
//   k_layered  _layered_thermodynamic_time_step!  thermodynamic_time_step.jl:131-298 (snow on ice, resistors in
//           series: ice_snow_conductive_flux / interface_temperature, slab_heat_and_tracer_fluxes.jl:47-84;
//           snow_accumulation, snow_ice_formation :331-353).
// Top boundary conditions: PrescribedTemperature, or MeltingConstrainedFluxBalance with a numeric external flux (the
// secant solve's root in closed form, see include/csi.h).
// Per-cell, no stencil.  Compiled with -ffp-contract=off, oracle expression order.
#include "csi_dev.h"
#include "csi_kernels.h"
#include "thermo_dev.h"

namespace csi {
__global__ void __launch_bounds__(256) k_slab(SlabDev s, GridDev g, FRef h, FRef a, FRef mf, int has_mf, double dt) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const double hn = h(i, j), an = a(i, j), hc = s.hc;
    const bool consolidated = hn >= hc;
    const double Tb = s.liq_T0 - s.liq_slope * s.S;
    double Tu = s.Tu;
    if (s.top_bc_kind == 1) {      // MeltingConstrainedFluxBalance: root of Qx - Qi(T), capped at Tm(S_ice); thin slab: Tb
        const double Tm = s.liq_T0 - s.liq_slope * s.ice_salinity;
        Tu = consolidated ? jmin(Tb - s.Qu * hn / s.k, Tm) : Tb;
    }
    slab_from_surface(s, i, j, h, a, mf, has_mf, hn, an, hc, dt, Tb, Tu, [&](double T) { return s.rho_bulk * latent_heat(s, T); },
                      [&](double) { return s.Qu; }, [&](double) { return (s.bot_flux_kind == 1) ? (-(1 - an)) * s.Qb : s.Qb; });
}

__global__ void __launch_bounds__(256) k_layered(SlabDev s, SnowDev w, GridDev g, FRef h, FRef a, FRef hs, LayeredOut o, double dt) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const double hin = h(i, j), an = a(i, j), hc = s.hc;
    double hsn = hs(i, j);
    const bool consolidated = hin >= hc;
    const double Tb = s.liq_T0 - s.liq_slope * s.S;
    double Tm = s.liq_T0 - s.liq_slope * s.ice_salinity;
    const double ks = w.k, ki = s.k;
    const double Qu = s.Qu;
    Tm = (hsn > 0) ? 0.0 : Tm;
    const double Ri = hin / ki, Rs = hsn / ks, R = Rs + Ri;
    double Tus = w.Tu;
    if (w.top_bc_kind == 1) Tus = consolidated ? jmin(Tb - Qu * R, Tm) : Tb;
    const LayeredNums n{w.rho, s.rho_l, ki, dt, w.snowfall, s.rho_bulk, s.L0, hc};
    layered_from_surface(n, i, j, h, a, hs, o, hin, an, hsn, Tb, Tus, Ri, R, [&](double T) { return latent_heat(s, T); },
                         [&](double) { return Qu; }, [&](double) { return (s.bot_flux_kind == 1) ? (-(1 - an)) * s.Qb : s.Qb; });
}

ThermoLaunch launch_layered_step(const SlabDev& S, const SnowDev& W, const GridDev& g, const FRef& h, const FRef& a, const FRef& hs,
                                 const LayeredOut& o, double dt, hipStream_t s) {
    hipLaunchKernelGGL(k_layered, thermo_grid(g), thermo_block(), 0, s, S, W, g, h, a, hs, o, dt);
    return ThermoLaunch{2, SW_NONE, -1};
}

ThermoLaunch launch_slab_step(const SlabDev& S, const GridDev& g, const FRef& h, const FRef& a, const FRef& mf, int has_mf,
                              double dt, hipStream_t s) {
    hipLaunchKernelGGL(k_slab, thermo_grid(g), thermo_block(), 0, s, S, g, h, a, mf, has_mf, dt);
    return ThermoLaunch{1, SW_NONE, -1};
}

}  // namespace csi
