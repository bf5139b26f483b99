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
#include "csi_kernels.h"

namespace csi {
namespace mom {

template <bool FAST, bool VISC>
__global__ void __launch_bounds__(256) k_tendencies(MomDev M, Range r) {
    CELL_OF_RANGE(r)
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
    CELL_OF_RANGE(r)
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
    const double tau_i = implicit_coef<FAST>(P, top, bot, uc, v4, mi, ai);
    store_with_images(M.out, P.g, im, i, j, close_substep<FAST, false>(P, um, G, tau_i, P.dt, fd, mi, ai, false));
}

template <bool FAST>
__global__ void __launch_bounds__(256) k_expl_vstep(MomDev M, Range r, ImageSpec im) {
    CELL_OF_RANGE(r)
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
    const double tau_i = implicit_coef<FAST>(P, top, bot, vc, u4, mi, ai);
    store_with_images(M.out, P.g, im, i, j, close_substep<FAST, false>(P, vm, G, tau_i, P.dt, fd, mi, ai, false));
}

}  // namespace mom

void launch_explicit_tendencies(const MomDev& M, const Range& r, int viscous, int fast, hipStream_t s) {
    const dim3 b(64, 4);
    if (fast) {
        if (viscous) hipLaunchKernelGGL((mom::k_tendencies<true, true>), grid_for(r, b), b, 0, s, M, r);
        else hipLaunchKernelGGL((mom::k_tendencies<true, false>), grid_for(r, b), b, 0, s, M, r);
    } else {
        if (viscous) hipLaunchKernelGGL((mom::k_tendencies<false, true>), grid_for(r, b), b, 0, s, M, r);
        else hipLaunchKernelGGL((mom::k_tendencies<false, false>), grid_for(r, b), b, 0, s, M, r);
    }
}
void launch_explicit_ustep(const MomDev& M, const Range& r, const ImageSpec& im, int fast, hipStream_t s) {
    const dim3 b(64, 4);
    if (fast) hipLaunchKernelGGL(mom::k_expl_ustep<true>, grid_for(r, b), b, 0, s, M, r, im);
    else hipLaunchKernelGGL(mom::k_expl_ustep<false>, grid_for(r, b), b, 0, s, M, r, im);
}
void launch_explicit_vstep(const MomDev& M, const Range& r, const ImageSpec& im, int fast, hipStream_t s) {
    const dim3 b(64, 4);
    if (fast) hipLaunchKernelGGL(mom::k_expl_vstep<true>, grid_for(r, b), b, 0, s, M, r, im);
    else hipLaunchKernelGGL(mom::k_expl_vstep<false>, grid_for(r, b), b, 0, s, M, r, im);
}

}  // namespace csi
