// evp_strict.hip -- STRICT-mode EVP kernels (CSI_MODE_STRICT).
//
// One HIP kernel per reference @kernel, the reference's operation order in every expression,
// compiled with -ffp-contract=off: results are bit-for-bit those of the CPU oracle, which is
// what anchors the parity of the optimised FAST kernels (evp_fast.hip).
//
//   k_init      _initialize_evp_rhology!   Rheologies/elasto_visco_plastic_rheology.jl:211-219
//   k_visc      _compute_evp_viscosities!  :236-273 (+ strain rates :360-375)
//   k_stress    _compute_evp_stresses!     :294-354 (+ ice_pressure :282-289)
//   k_ustep     _u_velocity_step!          SeaIceDynamics/split_explicit_momentum_equations.jl:197-229
//   k_vstep     _v_velocity_step!          :231-264
// The strain rates and the four-point interpolations of k_visc / k_stress are derived_dev.h's, with the metric kind decided at run
// time (dv::MK_RUNTIME).  The velocity steps are momentum_dev.h's point-wise sub-step -- gather, u/v_velocity_tendency
// (momentum_tendencies_kernel_functions.jl:11-74) on the stored stresses, implicit coefficient, closing part -- instantiated with
// strict arithmetic; the local halo fill that follows each of them in the reference (:180-187) is fused into the store
// (store_with_images).  The free-drift velocities of marginal ice are momentum_free_drift.hip's.
#include "csi_kernels.h"
#include "momentum_dev.h"

namespace csi {
namespace strict {

using namespace dv;
constexpr int MK = MK_RUNTIME;      // dxm / dym / azm (csi_dev.h) at every access: the same calls as oracle/csi_oracle.c
#define F_ LOC_F
#define C_ LOC_C

// Julia's max(a, b) for floats: NaN if either is NaN (fmax would drop the NaN)
__device__ __forceinline__ double jmax(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? b : a); }

__device__ __forceinline__ double ice_mass(const EvpDev& P, int i, int j) {   // ClimaSeaIce.jl:42
    return P.h(i, j) * P.rho * P.a(i, j);
}

// derived_dev.h's strain rates on this model's velocities
__device__ __forceinline__ double exx(const EvpDev& P, int i, int j) { return e_xx<MK>(P.g, P.u, P.v, i, j); }
__device__ __forceinline__ double eyy(const EvpDev& P, int i, int j) { return e_yy<MK>(P.g, P.u, P.v, i, j); }
__device__ __forceinline__ double exy(const EvpDev& P, int i, int j) { return e_xy<MK>(P.g, P.u, P.v, i, j); }

__global__ void k_init(EvpDev P, Range r, FRef un, FRef vn) {
    CELL_OF_RANGE(r)
    P.P(i, j) = P.P_star * P.h(i, j) * exp(-P.C_star * (1 - P.a(i, j)));   // ice_strength :219
    un(i, j) = P.u(i, j);
    vn(i, j) = P.v(i, j);
}

__global__ void k_visc(EvpDev P, Range r) {
    CELL_OF_RANGE(r)
    const double ie = 1.0 / P.ecc;
    const double em2 = ie * ie;
    const double Dm = P.Dmin;
    double e11c = exx(P, i, j);
    double e22c = eyy(P, i, j);
    double e12f = exy(P, i, j);
    double e11f = avg4(exx(P, i - 1, j - 1), exx(P, i, j - 1), exx(P, i - 1, j), exx(P, i, j));           // to (f, f)
    double e22f = avg4(eyy(P, i - 1, j - 1), eyy(P, i, j - 1), eyy(P, i - 1, j), eyy(P, i, j));
    double e12c = avg4(exy(P, i, j), exy(P, i + 1, j), exy(P, i, j + 1), exy(P, i + 1, j + 1));           // to (c, c)
    double dc = e11c + e22c;
    double df = e11f + e22f;
    double sc = sqrt((e11c - e22c) * (e11c - e22c) + 4 * (e12c * e12c));
    double sf = sqrt((e11f - e22f) * (e11f - e22f) + 4 * (e12f * e12f));
    double Dc = jmax(sqrt(dc * dc + (sc * sc) * em2), Dm);
    double Df = jmax(sqrt(df * df + (sf * sf) * em2), Dm);
    double Pc = P.P(i, j);
    double Pf = avg4_ff(P.P, i, j);
    P.zf(i, j) = Pf / (2 * Df);
    P.zc(i, j) = Pc / (2 * Dc);
    P.Dl(i, j) = Dc;
}

__device__ __forceinline__ double clampd(double x, double lo, double hi) { return x > hi ? hi : (x < lo ? lo : x); }

__global__ void k_stress(EvpDev P, Range r) {
    CELL_OF_RANGE(r)
    const GridDev& g = P.g;
    const double ie = 1.0 / P.ecc;
    const double em2 = ie * ie;
    const double ap = P.amax, am = P.amin, ca = P.ca, dt = P.dt;
    double e11 = exx(P, i, j);
    double e22 = eyy(P, i, j);
    double e12 = exy(P, i, j);
    double zc = P.zc(i, j);
    double zf = P.zf(i, j);
    double Pr;
    if (P.pressure_kind == 0) {
        double Pc = P.P(i, j), Dc = P.Dl(i, j);
        Pr = Pc * Dc / (Dc + P.Dmin);
    } else {
        Pr = P.P(i, j);
    }
    double etac = zc * em2;
    double etaf = zf * em2;
    double s11n = 2 * etac * e11 + ((zc - etac) * (e11 + e22) - Pr / 2);
    double s22n = 2 * etac * e22 + ((zc - etac) * (e11 + e22) - Pr / 2);
    double s12n = 2 * etaf * e12;
    double mc = ice_mass(P, i, j);
    double mf = avg4_ff([&](int ii, int jj) { return ice_mass(P, ii, jj); }, i, j);
    double g2c = zc * ca * dt / mc / azm(g, C_, C_, i, j);
    g2c = isnan(g2c) ? ap * ap : g2c;
    double gc = clampd(sqrt(g2c), am, ap);
    double g2f = zf * ca * dt / mf / azm(g, F_, F_, i, j);
    g2f = isnan(g2f) ? ap * ap : g2f;
    double gf = clampd(sqrt(g2f), am, ap);
    double s11s = (s11n - P.s11(i, j)) / gc;
    double s22s = (s22n - P.s22(i, j)) / gc;
    double s12s = (s12n - P.s12(i, j)) / gf;
    P.s11(i, j) += (mc > 0) ? s11s : 0.0;
    P.s22(i, j) += (mc > 0) ? s22s : 0.0;
    P.s12(i, j) += (mf > 0) ? s12s : 0.0;
    P.al(i, j) = gc;
}

// ---- the velocity steps: momentum_dev.h's point-wise sub-step with strict arithmetic on the stored stresses (FAST = false,
// VISC = false), stored in place.  dtau = dt / Ix(alpha), also the Delta t of sum_of_forcing (evp:391-401)
__global__ void __launch_bounds__(256) k_ustep(EvpDev P, Range r, ImageSpec im) {
    CELL_OF_RANGE(r)
    mom::UPoint q;
    mom::gather_u<false>(P, P.u, P.v, i, j, q);
    const double dtau = P.dt / ((q.alw + q.ale) / 2);
    double mi, ai;
    const double G = mom::u_tendency<false, false>(P, 0.0, q, i, j, dtau, mi, ai);
    const double tau_i = mom::implicit_coef<false>(P, q.top, q.bot, q.uc, q.v4, mi, ai);
    const bool peripheral = q.c.inact[3] | q.c.inact[2];               // peripheral_node (f, c, c): cells (i, j), (i - 1, j)
    store_with_images(P.u, P.g, im, i, j, mom::close_substep<false, true>(P, q.uc, G, tau_i, dtau, q.fd, mi, ai, peripheral));
}

__global__ void __launch_bounds__(256) k_vstep(EvpDev P, Range r, ImageSpec im) {
    CELL_OF_RANGE(r)
    mom::VPoint q;
    mom::gather_v<false>(P, P.u, P.v, i, j, q);
    const double dtau = P.dt / ((q.als + q.aln) / 2);
    double mi, ai;
    const double G = mom::v_tendency<false, false>(P, 0.0, q, i, j, dtau, mi, ai);
    const double tau_i = mom::implicit_coef<false>(P, q.top, q.bot, q.vc, q.u4, mi, ai);
    const bool peripheral = q.c.inact[4] | q.c.inact[1];               // peripheral_node (c, f, c): cells (i, j), (i, j - 1)
    store_with_images(P.v, P.g, im, i, j, mom::close_substep<false, true>(P, q.vc, G, tau_i, dtau, q.fd, mi, ai, peripheral));
}

}  // namespace strict

void launch_strict_init(const EvpDev& P, const Range& r, hipStream_t s) {
    dim3 b(64, 4);
    hipLaunchKernelGGL(strict::k_init, grid_for(r, b), b, 0, s, P, r, P.un, P.vn);
}
void launch_strict_visc(const EvpDev& P, const Range& r, hipStream_t s) {
    dim3 b(64, 4);
    hipLaunchKernelGGL(strict::k_visc, grid_for(r, b), b, 0, s, P, r);
}
void launch_strict_stress(const EvpDev& P, const Range& r, hipStream_t s) {
    dim3 b(64, 4);
    hipLaunchKernelGGL(strict::k_stress, grid_for(r, b), b, 0, s, P, r);
}
void launch_strict_ustep(const EvpDev& P, const Range& r, const ImageSpec& im, hipStream_t s) {
    dim3 b(64, 4);
    hipLaunchKernelGGL(strict::k_ustep, grid_for(r, b), b, 0, s, P, r, im);
}
void launch_strict_vstep(const EvpDev& P, const Range& r, const ImageSpec& im, hipStream_t s) {
    dim3 b(64, 4);
    hipLaunchKernelGGL(strict::k_vstep, grid_for(r, b), b, 0, s, P, r, im);
}

}  // namespace csi
