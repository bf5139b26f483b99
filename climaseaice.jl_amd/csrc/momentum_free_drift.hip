// momentum_free_drift.hip -- StressBalanceFreeDrift as the model's whole dynamics (csi_dynamics_set(ctx, CSI_DYNAMICS_FREE_DRIFT)).
//
//   k_free_drift_step   _free_drift_velocity_step!   SeaIceDynamics/stress_balance_free_drift.jl:145-151
//                       (time_step_momentum!(model, ::AbstractFreeDriftDynamics, ...), :132-143; closed forms :61-109)
// One launch over i = 1 .. Nx, j = 1 .. Ny: u[i, j] = free_drift_u, v[i, j] = free_drift_v at EVERY point -- no mass or concentration
// select, no `* active` factor, nothing read of the current u, v, nothing of dt.  Exactly one stress is a SemiImplicitStress (checked
// on the host: csi_momentum.hip need_free_drift_dynamics); it gives U_e and C = rho_e C_D, the other one the explicit stress tau.  Each
// store also writes the halo images of its component (store_point_and_images below, store_with_images' stores: the fill_halo_regions! of update_state!, periodic wrap,
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
// stress_balance_velocity, shared with k_free_drift (evp_strict.hip): the reference's operation order, compiled without contraction,
// the same for STRICT and FAST.
#include "momentum_dev.h"
#include "csi_kernels.h"

namespace csi {
namespace mom {

// store_with_images (csi_dev.h) restated -- KEEP THE TWO IN STEP: a change of the image semantics there has to be made here too
// (rewriting store_with_images itself in this form would change the code of every velocity kernel and is left for a change of its
// own).  The same stores: the point, its north-fold image, its x images, its y images and their corners, a
// ValueBoundaryCondition side reflected about twice its value, x before y -- with the images in fixed slots (low side, high side)
// instead of lists that are indexed at run time: those lists live in scratch memory, which this kernel then does not need at all
__device__ __forceinline__ void store_point_and_images(const FRef& f, const GridDev& g, const ImageSpec& im, int i, int j, double val) {
    f(i, j) = val;
    const bool in_x = (i >= 1) & (i <= g.Nx), in_y = (j >= 1) & (j <= g.Ny);
    const bool near_x = in_x & ((i <= g.Hx) | (i > g.Nx - g.Hx));
    const bool fold = im.yhi == IMG_FOLD;
    const bool near_y = in_y & ((j <= g.Hy) | (j > g.Ny - g.Hy - (fold ? 1 : 0)));
    if (!(near_x | near_y)) return;
    if (fold & in_x & in_y) {
        const int jt = im.fold_fy ? 2 * g.Ny + 1 - j : 2 * g.Ny - j;
        if ((jt > g.Ny) & (jt <= g.Ny + g.Hy)) {
            int it = im.fold_fx ? g.Nx - i + 2 : g.Nx - i + 1;
            double w = (double)im.fold_sign * val;
            if (it > g.Nx) { it -= g.Nx; w = fabs((double)im.fold_sign) * val; }
            f(it, jt) = w;
            if (it <= g.Hx) f(it + g.Nx, jt) = w;
            if (it > g.Nx - g.Hx) f(it - g.Nx, jt) = w;
        }
    }
    bool hx[2], hy[2];
    const int xi[2] = {image_lo(im.xlo, i, g.Nx, g.Hx, hx[0]), image_hi(im.xhi, i, g.Nx, g.Hx, hx[1])};
    const int yj[2] = {image_lo(im.ylo, j, g.Ny, g.Hy, hy[0]), image_hi(im.yhi, j, g.Ny, g.Hy, hy[1])};
    const bool rx[2] = {im.xlo == IMG_VALUE, im.xhi == IMG_VALUE}, ry[2] = {im.ylo == IMG_VALUE, im.yhi == IMG_VALUE};
    const double cx[2] = {2 * im.vxlo, 2 * im.vxhi}, cy[2] = {2 * im.vylo, 2 * im.vyhi};
#pragma unroll
    for (int a = 0; a < 2; ++a)
        if (in_x & hx[a]) f(xi[a], j) = rx[a] ? cx[a] - val : val;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (!(in_y & hy[b])) continue;
        f(i, yj[b]) = ry[b] ? cy[b] - val : val;
#pragma unroll
        for (int a = 0; a < 2; ++a)
            if (in_x & hx[a]) {
                const double w = rx[a] ? cx[a] - val : val;
                f(xi[a], yj[b]) = ry[b] ? cy[b] - w : w;
            }
    }
}

__global__ void __launch_bounds__(256) k_free_drift_step(EvpDev P, Range r, ImageSpec imu, ImageSpec imv) {
    const int i = r.i0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int j = r.j0 + (int)(blockIdx.y * blockDim.y + threadIdx.y);
    if (i > r.i1 || j > r.j1) return;
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
    store_point_and_images(P.u, P.g, imu, i, j, uf);
    store_point_and_images(P.v, P.g, imv, i, j, vf);
}

}  // namespace mom

void launch_free_drift_step(const EvpDev& P, const Range& r, const ImageSpec& imu, const ImageSpec& imv, hipStream_t s) {
    const dim3 b(64, 4);
    const dim3 g((unsigned)((r.i1 - r.i0 + 1 + b.x - 1) / b.x), (unsigned)((r.j1 - r.j0 + 1 + b.y - 1) / b.y), 1);
    hipLaunchKernelGGL(mom::k_free_drift_step, g, b, 0, s, P, r, imu, imv);
}

}  // namespace csi
