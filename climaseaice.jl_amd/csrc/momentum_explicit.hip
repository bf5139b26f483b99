// momentum_explicit.hip -- the ExplicitSolver (csi_momentum_solver_set(ctx, CSI_SOLVER_EXPLICIT)), both rheologies.
//
//   k_tendencies   _compute_velocity_tendencies!   SeaIceDynamics/momentum_tendencies_kernel_functions.jl:3-8
//                  (compute_momentum_tendencies!, explicit_momentum_equations.jl:85-113)
//   k_expl_ustep   _step_u_velocity!               explicit_momentum_equations.jl:40-60
//   k_expl_vstep   _step_v_velocity!               :62-82
// The tendency launch writes G^n.u and G^n.v; with ElastoViscoPlasticRheology its divergence reads the STORED sigma11, sigma22,
// sigma12 (compute_stresses! is never called on this path) and sum_of_forcing_* adds (u^n - u) / Delta t / Ixᶠᵃᵃ(alpha) with
// the u^n nothing refreshes.  The steps are separate launches -- with a SemiImplicitStress the v step's drag norm reads the NEW u
// at four points -- and, unlike the split-explicit kernels, have no `* active` factor and no m <= 0 guard on tau_i.  Each writes
// the halo images of its component with its stores: the fill_halo_regions! that follows it (:33, :36).
#include "momentum_dev.h"

namespace csi {
namespace mom {

#define MOM_CELL(r)                                                            \
    const int i = (r).i0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);       \
    const int j = (r).j0 + (int)(blockIdx.y * blockDim.y + threadIdx.y);       \
    if (i > (r).i1 || j > (r).j1) return;

template <bool FAST, bool VISC>
__global__ void __launch_bounds__(256) k_tendencies(MomDev M, Range r) {
    MOM_CELL(r)
    const EvpDev& P = M.P;
    UPoint qu;
    VPoint qv;
    gather_u<VISC>(P, P.u, P.v, i, j, qu);
    gather_v<VISC>(P, P.u, P.v, i, j, qv);
    double mi, ai;
    M.Gu(i, j) = u_tendency<FAST, VISC>(P, M.nu, qu, i, j, P.dt, mi, ai);
    M.Gv(i, j) = v_tendency<FAST, VISC>(P, M.nu, qv, i, j, P.dt, mi, ai);
}

template <bool FAST>
__global__ void __launch_bounds__(256) k_expl_ustep(MomDev M, Range r, ImageSpec im) {
    MOM_CELL(r)
    const EvpDev& P = M.P;
    // gather: h, aice at (i-1, j), (i, j); u^-, G, u at the point; v at the four points of the cross average; stresses; free drift
    const double hw = P.h(i - 1, j), he = P.h(i, j), aw = P.a(i - 1, j), ae = P.a(i, j);
    const double um = M.um(i, j), G = M.Gu(i, j), uc = P.u(i, j);
    double v4[4] = {P.v(i - 1, j), P.v(i, j), P.v(i - 1, j + 1), P.v(i, j + 1)};
    StressPt top, bot;
    gather_stress_u(P.top, P.u, P.v, i, j, top);
    gather_stress_u(P.bot, P.u, P.v, i, j, bot);
    const double fd = ld_sel(P.free_drift, addr(P.ufd, i, j), addr(P.u, i, j), 0.0);
    const double ai = (aw + ae) / 2;
    const double mi = (hw * P.rho * aw + he * P.rho * ae) / 2;
    const double dt = P.dt;
    const double tau_i = implicit_coef<FAST>(P, top, bot, uc, v4, mi, ai);
    const double uD = FAST ? fma(dt, G, um) / fma(dt, tau_i, 1.0) : (um + dt * G) / (1 + dt * tau_i);
    const double uF = P.free_drift ? fd : 0.0;
    const bool marginal = (mi > MOM_EPS64) & (ai > MOM_EPS64);
    const bool active_ice = (mi >= P.min_mass) & (ai >= P.min_conc);
    store_with_images(M.out, P.g, im, i, j, active_ice ? uD : (marginal ? uF : 0.0));
}

template <bool FAST>
__global__ void __launch_bounds__(256) k_expl_vstep(MomDev M, Range r, ImageSpec im) {
    MOM_CELL(r)
    const EvpDev& P = M.P;
    const double hs = P.h(i, j - 1), hn = P.h(i, j), as_ = P.a(i, j - 1), an = P.a(i, j);
    const double vm = M.vm(i, j), G = M.Gv(i, j), vc = P.v(i, j);
    double u4[4] = {P.u(i, j - 1), P.u(i + 1, j - 1), P.u(i, j), P.u(i + 1, j)};
    StressPt top, bot;
    gather_stress_v(P.top, P.u, P.v, i, j, top);
    gather_stress_v(P.bot, P.u, P.v, i, j, bot);
    const double fd = ld_sel(P.free_drift, addr(P.vfd, i, j), addr(P.v, i, j), 0.0);
    const double ai = (as_ + an) / 2;
    const double mi = (hs * P.rho * as_ + hn * P.rho * an) / 2;
    const double dt = P.dt;
    const double tau_i = implicit_coef<FAST>(P, top, bot, vc, u4, mi, ai);
    const double vD = FAST ? fma(dt, G, vm) / fma(dt, tau_i, 1.0) : (vm + dt * G) / (1 + dt * tau_i);
    const double vF = P.free_drift ? fd : 0.0;
    const bool marginal = (mi > MOM_EPS64) & (ai > MOM_EPS64);
    const bool active_ice = (mi >= P.min_mass) & (ai >= P.min_conc);
    store_with_images(M.out, P.g, im, i, j, active_ice ? vD : (marginal ? vF : 0.0));
}

}  // namespace mom

static inline dim3 mom_grid(const Range& r, dim3 b) {
    return dim3((unsigned)((r.i1 - r.i0 + 1 + b.x - 1) / b.x), (unsigned)((r.j1 - r.j0 + 1 + b.y - 1) / b.y), 1);
}

void launch_explicit_tendencies(const MomDev& M, const Range& r, int viscous, int fast, hipStream_t s) {
    const dim3 b(64, 4);
    if (fast) {
        if (viscous) hipLaunchKernelGGL((mom::k_tendencies<true, true>), mom_grid(r, b), b, 0, s, M, r);
        else hipLaunchKernelGGL((mom::k_tendencies<true, false>), mom_grid(r, b), b, 0, s, M, r);
    } else {
        if (viscous) hipLaunchKernelGGL((mom::k_tendencies<false, true>), mom_grid(r, b), b, 0, s, M, r);
        else hipLaunchKernelGGL((mom::k_tendencies<false, false>), mom_grid(r, b), b, 0, s, M, r);
    }
}
void launch_explicit_ustep(const MomDev& M, const Range& r, const ImageSpec& im, int fast, hipStream_t s) {
    const dim3 b(64, 4);
    if (fast) hipLaunchKernelGGL(mom::k_expl_ustep<true>, mom_grid(r, b), b, 0, s, M, r, im);
    else hipLaunchKernelGGL(mom::k_expl_ustep<false>, mom_grid(r, b), b, 0, s, M, r, im);
}
void launch_explicit_vstep(const MomDev& M, const Range& r, const ImageSpec& im, int fast, hipStream_t s) {
    const dim3 b(64, 4);
    if (fast) hipLaunchKernelGGL(mom::k_expl_vstep<true>, mom_grid(r, b), b, 0, s, M, r, im);
    else hipLaunchKernelGGL(mom::k_expl_vstep<false>, mom_grid(r, b), b, 0, s, M, r, im);
}

}  // namespace csi
