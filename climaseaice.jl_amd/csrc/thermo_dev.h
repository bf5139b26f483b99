// thermo_dev.h -- device helpers shared by the thermodynamic kernels (thermo.hip, thermo_flux.hip).
#pragma once
#include "csi_dev.h"
#include "csi_kernels.h"

namespace csi {
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

}  // namespace csi
