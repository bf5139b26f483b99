// thermo_dev.h -- what the thermodynamic kernels share (thermo.hip, thermo_flux.hip; mixed_layer.hip takes jmax / jmin): Julia's max / min, the
// latent heat, ice_volume_update, each step from the surface temperature on, and the launch geometry of the four per-cell kernels.
#pragma once
#include "csi_dev.h"
#include "csi_kernels.h"

namespace csi {
// k_slab, k_layered, k_slab_flux, k_layered_flux: one thread per cell (i, j) = 1 + block * blockDim + thread
constexpr int kThermoBlockX = 64, kThermoBlockY = 4;
inline dim3 thermo_block() { return dim3(kThermoBlockX, kThermoBlockY); }
inline dim3 thermo_grid(const GridDev& g) {
    return dim3((unsigned)((g.Nx + kThermoBlockX - 1) / kThermoBlockX), (unsigned)((g.Ny + kThermoBlockY - 1) / kThermoBlockY));
}

// Julia's max(a, b) for floats: NaN if either is NaN
__device__ __forceinline__ double jmax(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? b : a); }
__device__ __forceinline__ double jmin(double a, double b) { return (a != a || b != b) ? a + b : (b < a ? b : a); }


__device__ __forceinline__ double latent_heat(const SlabDev& s, double T) {
    return s.L0 + (s.rho_l * s.c_l / s.rho_pure - s.c_i) * (T - s.T0);
}

// ice_volume_update, thermodynamic_time_step.jl:304-324 (+ concentration_thermodynamic_step :358-370)
__device__ __forceinline__ void ice_volume_update(double dtV, double hn, double an, double hc, double dt, double& h1, double& a1) {
    double V1 = hn * an + dt * dtV;
    V1 = jmax(0.0, V1);
    dtV = (V1 - hn * an) / dt;
    // `x * flag` with a Julia Bool: false is a strong zero (NaN * false == 0, sign kept)
    const bool freezing = (dtV >= 0), melting = (dtV < 0);
    const double xf = (1 - an) / hc * dtV, xm = an / (2 * hn) * dtV;
    const double daf = freezing ? xf : copysign(0.0, xf);
    const double dam = melting ? xm : copysign(0.0, xm);
    double ap = an + dt * (daf + dam);
    ap = jmax(0.0, ap);
    double hp = V1 / ap;
    hp = (ap <= 0) ? 0.0 : hp;
    ap = (dtV == 0) ? an : ap;
    hp = (dtV == 0) ? hn : hp;
    ap = (hp == 0) ? 0.0 : ap;
    hp = (ap == 0) ? 0.0 : hp;
    a1 = (ap > 1) ? 1.0 : ap;
    h1 = (ap > 1) ? hp * ap : hp;
}

// the external fluxes a step used
struct UsedFluxes {
    double top, bottom;
};

// The bare-ice step from the surface temperature Tu on: the tendency, ice_volume_update and the stores of h, aice and the mass flux.
// E(T): rho_bulk * latent_heat at T; Qx(T), Qb_ext(T): the top's and the bottom's external flux -- callables, so that each is evaluated
// where the kernels always evaluated it (the bottom's after the top's): the scalar register allocation of the flux kernels' SW_NONE
// instantiations depends on the place.
template <class EFn, class QxFn, class QbFn>
__device__ __forceinline__ UsedFluxes slab_from_surface(const SlabDev& s, int i, int j, const FRef& h, const FRef& a, const FRef& mf, int has_mf,
                                                        double hn, double an, double hc, double dt, double Tb, double Tu, const EFn& E,
                                                        const QxFn& Qx, const QbFn& Qb_ext) {
    const double Eb = E(Tb);
    const double Eu = E(Tu);
    const double Qi_fun = (hn <= 0) ? 0.0 : -s.k * (Tu - Tb) / hn;
    const double Qu = (s.top_flux_kind == 1) ? Qi_fun : Qx(Tu);
    const double Qb = Qb_ext(Tu);
    const double Qi = (hn >= hc) ? Qi_fun : 0.0;
    const double wu = (Qu - Qi) / Eu;
    const double wb = (Qi - Qb) / Eb;
    double h1, a1;
    ice_volume_update(wu + wb, hn, an, hc, dt, h1, a1);
    a(i, j) = a1;
    h(i, j) = h1;
    if (has_mf) mf(i, j) = s.rho_bulk * (h1 * a1 - hn * an) / dt;
    return UsedFluxes{Qu, Qb};
}

// the numbers the layered step reads from the surface temperature on: the snow's and the liquid's density, the ice's conductivity, dt,
// the cell's snowfall, the ice's bulk density, the reference latent heat and the consolidation thickness
struct LayeredNums {
    double rs, rw, ki, dt, Ps, ri, Ls, hc;
};

// The layered step from the snow's surface temperature Tus on: the interface temperature, snow melt, the implicit concentration estimate,
// ice_volume_update, the snow update, snow-ice formation, the stores of h, aice, hs and of the optional outputs.  Ri = hin / ki and
// R = hs / ks + Ri: the resistances the surface solve used; latent(T): latent_heat at T; Qx(T), Qb_ext(T): as above.
template <class LatentFn, class QxFn, class QbFn>
__device__ __forceinline__ UsedFluxes layered_from_surface(const LayeredNums& n, int i, int j, const FRef& h, const FRef& a, const FRef& hs,
                                                           const LayeredOut& o, double hin, double an, double hsn, double Tb, double Tus,
                                                           double Ri, double R, const LatentFn& latent, const QxFn& Qx, const QbFn& Qb_ext) {
    const double Vin = hin * an, Vsn = hsn * an;
    const bool consolidated = hin >= n.hc;
    const double Tsi = (R <= 0) ? Tb : Tb + (Tus - Tb) * Ri / R;
    const double Qic = (R <= 0) ? 0.0 : (Tb - Tus) / R;
    const double Qis = consolidated ? Qic : 0.0;
    const double Qui = Qx(Tus);
    const double Qui_per_ice = (an > 0) ? Qui / an : 0.0;
    const double dQ = Qui_per_ice - Qis;
    const double melt_energy = jmax(0.0, -dQ);
    const double rs = n.rs, Ls = n.Ls;
    const double cap = rs * Ls * hsn / n.dt;
    const double Qs = jmin(melt_energy, cap);
    const double Gsm = Qs / (rs * Ls);
    const double ri = n.ri, riL = ri * Ls;
    const double Qbi = Qb_ext(Tus);
    const double alpha = (Qui - Qbi) / riL, beta = Qs / riL;
    const double Cm = (hin > 0) ? an / (2 * hin) : 0.0;
    const double Cf = (n.hc > 0) ? (1 - an) / n.hc : 0.0;
    const double Km = n.dt * Cm, Kf = n.dt * Cf;
    const double eps = 2.220446049250313e-16;
    const double Dm = 1 - Km * beta, Df = 1 - Kf * beta;
    const double am = (fabs(Dm) > eps) ? (an + Km * alpha) / Dm : an + Km * alpha;
    const double af = (fabs(Df) > eps) ? (an + Kf * alpha) / Df : an + Kf * alpha;
    const double dtVm = alpha + beta * am;
    const bool melting = dtVm < 0;
    const double atmp = melting ? am : af;
    const double Qeff = Qui + Qs * atmp;
    const double Eb = ri * latent(Tb), Eu = ri * latent(Tsi);
    const double Qii_fun = (hin <= 0) ? 0.0 : -n.ki * (Tsi - Tb) / hin;
    const double Qii = consolidated ? Qii_fun : 0.0;
    const double wu = (Qeff - Qii) / Eu, wb = (Qii - Qbi) / Eb;
    double hi1, a1;
    ice_volume_update(wu + wb, hin, an, n.hc, n.dt, hi1, a1);
    hsn = (a1 > 0) ? hsn * an / a1 : 0.0;
    const double Gsp = (a1 > 0) ? n.Ps / rs : 0.0;
    double hs1 = hsn + n.dt * (Gsp - Gsm);
    hs1 = jmax(0.0, hs1);
    {
        const double rw = n.rw;
        const double hf = hi1 * (1 - ri / rw) - hs1 * rs / rw;
        double dhs = (hf < 0) ? -hf * ri / rs : 0.0;
        const double hsp = jmax(0.0, hs1 - dhs);
        dhs = hs1 - hsp;
        hi1 = hi1 + dhs * rs / ri;
        hs1 = hsp;
    }
    hs1 = (a1 <= 0) ? 0.0 : hs1;
    a(i, j) = a1; h(i, j) = hi1; hs(i, j) = hs1;
    const double Pabs = rs * Gsp * a1;
    if (o.mf_ice.p) o.mf_ice(i, j) = ri * (hi1 * a1 - Vin) / n.dt;
    if (o.mf_snow.p) o.mf_snow(i, j) = rs * (hs1 * a1 - Vsn) / n.dt - Pabs;
    if (o.mf_int.p) o.mf_int(i, j) = Pabs;
    if (o.tu_ice.p) o.tu_ice(i, j) = Tsi;
    if (o.tu_snow.p) o.tu_snow(i, j) = Tus;
    return UsedFluxes{Qui, Qbi};
}

}  // namespace csi
