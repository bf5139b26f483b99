// momentum_viscous.hip -- the split-explicit sub-step of ViscousRheology (csi_rheology_set(ctx, CSI_RHEOLOGY_VISCOUS, nu)).
//
//   k_visc_ustep   _u_velocity_step!   SeaIceDynamics/split_explicit_momentum_equations.jl:197-229
//   k_visc_vstep   _v_velocity_step!   :231-264
// with ViscousRheology's stresses computed inline from the velocities (Rheologies/viscous_rheology.jl:15-22), the sub-step
// Delta t / substeps and the user forcing alone (Rheologies.jl:42-55).  One launch per component and sub-step; the local halo
// fill that follows each kernel in the reference (:180-187) is fused into the store (store_with_images).
//
// Deliberate departure (include/csi.h): the reference's kernel writes u[i, j] in place while its viscous stencil reads u
// at the neighbouring points, so its result depends on scheduling.  Here a launch reads the OLD values of its own component (M.P.u /
// M.P.v) and writes the new ones into another array (M.out): Jacobi within a component, Gauss-Seidel between the two (the second
// component of a sub-step reads the first one's new values, the order alternating with the parity of the sub-step, :178).
//
// STRICT (FAST = false): the reference's operation order, compiled without contraction: bit-for-bit the test-side restatement
// (tests/momentum_ref.py).  FAST: explicit FMAs, reciprocals of the mass and the metrics; both gather every load of a point first.
#include "momentum_dev.h"
#include "csi_kernels.h"

namespace csi {
namespace mom {

template <bool FAST>
__global__ void __launch_bounds__(256) k_visc_ustep(MomDev M, Range r, ImageSpec im) {
    CELL_OF_RANGE(r)
    const EvpDev& P = M.P;
    UPoint q;
    gather_u<true>(P, P.u, P.v, i, j, q);
    const double dtau = P.dt;                                          // Delta t / substeps (host), Rheologies.jl:49
    double mi, ai;
    const double G = u_tendency<FAST, true>(P, M.nu, q, i, j, 0.0, mi, ai);
    const double tau_i = implicit_coef<FAST>(P, q.top, q.bot, q.uc, q.v4, mi, ai);
    const bool peripheral = q.c.inact[3] | q.c.inact[2];               // peripheral_node (f, c, c): cells (i, j), (i - 1, j)
    store_with_images(M.out, P.g, im, i, j, close_substep<FAST, true>(P, q.uc, G, tau_i, dtau, q.fd, mi, ai, peripheral));
}

template <bool FAST>
__global__ void __launch_bounds__(256) k_visc_vstep(MomDev M, Range r, ImageSpec im) {
    CELL_OF_RANGE(r)
    const EvpDev& P = M.P;
    VPoint q;
    gather_v<true>(P, P.u, P.v, i, j, q);
    const double dtau = P.dt;
    double mi, ai;
    const double G = v_tendency<FAST, true>(P, M.nu, q, i, j, 0.0, mi, ai);
    const double tau_i = implicit_coef<FAST>(P, q.top, q.bot, q.vc, q.u4, mi, ai);
    const bool peripheral = q.c.inact[4] | q.c.inact[1];               // peripheral_node (c, f, c): cells (i, j), (i, j - 1)
    store_with_images(M.out, P.g, im, i, j, close_substep<FAST, true>(P, q.vc, G, tau_i, dtau, q.fd, mi, ai, peripheral));
}

}  // namespace mom

void launch_viscous_ustep(const MomDev& M, const Range& r, const ImageSpec& im, int fast, hipStream_t s) {
    const dim3 b(64, 4);
    if (fast) hipLaunchKernelGGL(mom::k_visc_ustep<true>, grid_for(r, b), b, 0, s, M, r, im);
    else hipLaunchKernelGGL(mom::k_visc_ustep<false>, grid_for(r, b), b, 0, s, M, r, im);
}
void launch_viscous_vstep(const MomDev& M, const Range& r, const ImageSpec& im, int fast, hipStream_t s) {
    const dim3 b(64, 4);
    if (fast) hipLaunchKernelGGL(mom::k_visc_vstep<true>, grid_for(r, b), b, 0, s, M, r, im);
    else hipLaunchKernelGGL(mom::k_visc_vstep<false>, grid_for(r, b), b, 0, s, M, r, im);
}

}  // namespace csi
