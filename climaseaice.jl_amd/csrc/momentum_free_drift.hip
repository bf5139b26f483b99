// momentum_free_drift.hip -- StressBalanceFreeDrift's closed forms (stress_balance_free_drift.jl:61-109), gathered once for both users:
//
//   k_free_drift_step   _free_drift_velocity_step!   SeaIceDynamics/stress_balance_free_drift.jl:145-151: the model's whole dynamics
//                       (csi_dynamics_set(ctx, CSI_DYNAMICS_FREE_DRIFT); time_step_momentum!(model, ::AbstractFreeDriftDynamics, ...), :132-143)
//   k_free_drift        the velocities of marginal ice (:111-129), once per sub-cycle into ufd / vfd: plain stores over the launch's
//                       range, no images
// k_free_drift_step:
// One launch over i = 1 .. Nx, j = 1 .. Ny: u[i, j] = free_drift_u, v[i, j] = free_drift_v at EVERY point -- no mass or concentration
// select, no `* active` factor, nothing read of the current u, v, nothing of dt.  Exactly one stress is a SemiImplicitStress (checked
// on the host: csi_momentum.hip need_free_drift_dynamics); it gives U_e and C = rho_e C_D, the other one the explicit stress tau.  Each
// store also writes the halo images of its component (store_with_images, csi_dev.h: the fill_halo_regions! of update_state!, periodic wrap,
// no-flux mirror, ValueBoundaryCondition, north fold), so no fill launch follows.  No value of u or v enters the result, so the
// images race with nothing that matters: the only load from u is the `safe` address below -- the point's own, interior element,
// loaded where the configuration has a number or nothing and discarded by the select -- and images are stored into halo cells only.  Wall faces and immersed faces are written like any other point, as the ExplicitSolver's velocity launches
// write them: what the local fill and update_state! leave there are recalled fill semantics, not pinned.
//
// A bandwidth kernel: per point pair at most four arrays read (tau_x, tau_y, u_e, v_e; ten loads, eight of them shared with the
// neighbouring lanes and rows through the caches) and two written, 2 sqrt + 1 divide per component; no LDS.  The operands are gathered
// the way momentum_dev.h gathers a point: every load unconditional, from a selected valid address, discarded by a select where the
// configuration has a number or nothing there -- all ten in flight before the first wait (tests/test_free_drift.py gates the
// generated code).  64-lane rows: consecutive lanes read and write consecutive elements.  The arithmetic is csi_dev.h
// stress_balance_velocity: the reference's operation order, compiled without contraction, the same for STRICT and FAST.
#include "momentum_dev.h"
#include "csi_kernels.h"

namespace csi {
namespace mom {

// one point pair: the closed forms of u and v at (i, j).  IMAGES: the destination is u / v with their halo images (the dynamics step);
// otherwise ufd / vfd with plain stores over the launch's range (the marginal-ice velocities of a sub-cycle)
template <bool IMAGES>
__device__ __forceinline__ void free_drift_point(const EvpDev& P, const Range& r, const ImageSpec& imu, const ImageSpec& imv) {
    CELL_OF_RANGE(r)
    // exactly one stress is a SemiImplicitStress and the explicit side never is one: the host refuses anything else before a launch
    // (csi_momentum.hip need_dynamics_common, need_free_drift_dynamics), so the explicit side is numbers, arrays or nothing
    const bool bot_semi = P.bot.kind == 3;
    const StressDev& semi = bot_semi ? P.bot : P.top;
    const StressDev& expl = bot_semi ? P.top : P.bot;
    // ---- gather: tau_x at the u point and at the three other u points around the v point, tau_y at the v point and at the three other
    // v points around the u point, u_e, v_e.  `safe`: the u point itself (a valid address of this launch; the value is discarded)
    const double* safe = addr(P.u, i, j);
    const bool tau_a = expl.kind == 2;                                  // arrays; a number pair (kind 1) or nothing otherwise
    const double cx = expl.kind == 1 ? expl.tau_u : 0.0, cy = expl.kind == 1 ? expl.tau_v : 0.0;
    const double tx_p = ld_sel(tau_a, addr(expl.fu, i, j), safe, cx);
    const double ty_p = ld_sel(tau_a, addr(expl.fv, i, j), safe, cy);
    // u point: tau_y at (i-1, j), (i, j), (i-1, j+1), (i, j+1); v point: tau_x at (i, j-1), (i+1, j-1), (i, j), (i+1, j)
    const double ty4[4] = {ld_sel(tau_a, addr(expl.fv, i - 1, j), safe, cy), ty_p,
                           ld_sel(tau_a, addr(expl.fv, i - 1, j + 1), safe, cy), ld_sel(tau_a, addr(expl.fv, i, j + 1), safe, cy)};
    const double tx4[4] = {ld_sel(tau_a, addr(expl.fu, i, j - 1), safe, cx), ld_sel(tau_a, addr(expl.fu, i + 1, j - 1), safe, cx),
                           tx_p, ld_sel(tau_a, addr(expl.fu, i + 1, j), safe, cx)};
    const double ue = ld_sel(semi.ue_kind == 2, addr(semi.fu, i, j), safe, semi.ue_kind == 1 ? semi.ue : 0.0);
    const double ve = ld_sel(semi.ve_kind == 2, addr(semi.fv, i, j), safe, semi.ve_kind == 1 ? semi.ve : 0.0);
    // ---- arithmetic on registers (:61-109)
    const double C = semi.rho_e * semi.Cd;
    const double uf = stress_balance_velocity(ue, tx_p, tx_p, avg4(ty4), C);
    const double vf = stress_balance_velocity(ve, ty_p, avg4(tx4), ty_p, C);
    if (IMAGES) {
        store_with_images(P.u, P.g, imu, i, j, uf);
        store_with_images(P.v, P.g, imv, i, j, vf);
    } else {
        P.ufd(i, j) = uf;
        P.vfd(i, j) = vf;
    }
}

__global__ void __launch_bounds__(256) k_free_drift_step(EvpDev P, Range r, ImageSpec imu, ImageSpec imv) {
    free_drift_point<true>(P, r, imu, imv);
}
// the free-drift velocities of marginal ice, once per sub-cycle into ufd / vfd (csi_free_drift_set kind 1), both modes
__global__ void __launch_bounds__(256) k_free_drift(EvpDev P, Range r) {
    free_drift_point<false>(P, r, ImageSpec{}, ImageSpec{});
}

}  // namespace mom

void launch_free_drift_step(const EvpDev& P, const Range& r, const ImageSpec& imu, const ImageSpec& imv, hipStream_t s) {
    const dim3 b(64, 4);
    hipLaunchKernelGGL(mom::k_free_drift_step, grid_for(r, b), b, 0, s, P, r, imu, imv);
}
void launch_free_drift(const EvpDev& P, const Range& r, hipStream_t s) {
    const dim3 b(64, 4);
    hipLaunchKernelGGL(mom::k_free_drift, grid_for(r, b), b, 0, s, P, r);
}

}  // namespace csi
