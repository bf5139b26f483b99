// derived_dev.h -- the reference's strict-order operators, stated ONCE for every kernel that evaluates them on fields: the strain rates
// (elasto_visco_plastic_rheology.jl:360-375), the four-point interpolations, the masked stress accessors and the stress divergence
// (ice_stress_divergence.jl:16-51).  Users: the STRICT viscosity and stress kernels (evp_strict.hip k_visc, k_stress), the derived-field and
// energy-budget kernels (derived.hip, budget.hip) and, for the divergence arithmetic on gathered values, momentum_dev.h div1 / div2
// (every point-wise velocity step, the STRICT EVP ones included).
//
// Every operator takes the bare grid and field references and the metric kind as a template parameter: MK = 0 uniform (two numbers),
// 1 per row (vectors indexed by j), 2 per point (twelve planes) -- decided when the kernel is chosen (derived.hip, budget.hip) -- or
// MK_RUNTIME: decided per access by csi_dev.h dxm / dym / azm (evp_strict.hip).  The reference's operation order in every expression;
// units that include this header are compiled without contraction.
#pragma once
#include "csi_dev.h"

namespace csi {
namespace dv {

constexpr int MK_RUNTIME = -1;
template <int MK> __device__ __forceinline__ double dx_(const GridDev& g, int lx, int ly, int i, int j) {
    if (MK == MK_RUNTIME) return dxm(g, lx, ly, i, j);
    if (MK == 0) return g.dx;
    if (MK == 1) return ly == LOC_C ? g.dxc[j] : g.dxf[j];
    return metric2(g, 0, lx, ly, i, j);
}
template <int MK> __device__ __forceinline__ double dy_(const GridDev& g, int lx, int ly, int i, int j) {
    if (MK == MK_RUNTIME) return dym(g, lx, ly, i, j);
    if (MK != 2) return g.dy;
    return metric2(g, 1, lx, ly, i, j);
}
template <int MK> __device__ __forceinline__ double az_(const GridDev& g, int lx, int ly, int i, int j) {
    if (MK == MK_RUNTIME) return azm(g, lx, ly, i, j);
    if (MK == 0) return g.dx * g.dy;
    if (MK == 1) return ly == LOC_C ? g.azc[j] : g.azf[j];
    return metric2(g, 2, lx, ly, i, j);
}

#define F_ LOC_F
#define C_ LOC_C
// ---- strain rates, elasto_visco_plastic_rheology.jl:360-375 ------------------------------------------------------------------------
template <int MK> __device__ __forceinline__ double eps_D(const GridDev& g, const FRef& u, const FRef& v, int i, int j) {
    double a = dy_<MK>(g, F_, C_, i + 1, j) * u.ld_(i + 1, j) - dy_<MK>(g, F_, C_, i, j) * u.ld_(i, j);
    double b = dx_<MK>(g, C_, F_, i, j + 1) * v.ld_(i, j + 1) - dx_<MK>(g, C_, F_, i, j) * v.ld_(i, j);
    return (a + b) / az_<MK>(g, C_, C_, i, j);
}
template <int MK> __device__ __forceinline__ double eps_T(const GridDev& g, const FRef& u, const FRef& v, int i, int j) {
    double dycc = dy_<MK>(g, C_, C_, i, j), dxcc = dx_<MK>(g, C_, C_, i, j);
    double a = u.ld_(i + 1, j) / dy_<MK>(g, F_, C_, i + 1, j) - u.ld_(i, j) / dy_<MK>(g, F_, C_, i, j);
    double b = v.ld_(i, j + 1) / dx_<MK>(g, C_, F_, i, j + 1) - v.ld_(i, j) / dx_<MK>(g, C_, F_, i, j);
    return ((dycc * dycc) * a - (dxcc * dxcc) * b) / az_<MK>(g, C_, C_, i, j);
}
template <int MK> __device__ __forceinline__ double eps_S(const GridDev& g, const FRef& u, const FRef& v, int i, int j) {
    double dxff = dx_<MK>(g, F_, F_, i, j), dyff = dy_<MK>(g, F_, F_, i, j);
    double a = u.ld_(i, j) / dx_<MK>(g, F_, C_, i, j) - u.ld_(i, j - 1) / dx_<MK>(g, F_, C_, i, j - 1);
    double b = v.ld_(i, j) / dy_<MK>(g, C_, F_, i, j) - v.ld_(i - 1, j) / dy_<MK>(g, C_, F_, i - 1, j);
    return ((dxff * dxff) * a + (dyff * dyff) * b) / az_<MK>(g, F_, F_, i, j);
}
template <int MK> __device__ __forceinline__ double e_xx(const GridDev& g, const FRef& u, const FRef& v, int i, int j) {
    return (eps_D<MK>(g, u, v, i, j) + eps_T<MK>(g, u, v, i, j)) / 2;
}
template <int MK> __device__ __forceinline__ double e_yy(const GridDev& g, const FRef& u, const FRef& v, int i, int j) {
    return (eps_D<MK>(g, u, v, i, j) - eps_T<MK>(g, u, v, i, j)) / 2;
}
template <int MK> __device__ __forceinline__ double e_xy(const GridDev& g, const FRef& u, const FRef& v, int i, int j) {
    return eps_S<MK>(g, u, v, i, j) / 2;
}
// ---- four-point interpolations of f(i, j) (csi_dev.h avg4) to the point (i, j) of the named location -------------------------------
template <class F> __device__ __forceinline__ double avg4_ff(F f, int i, int j) { return avg4(f(i - 1, j - 1), f(i, j - 1), f(i - 1, j), f(i, j)); }   // from (c, c)
template <class F> __device__ __forceinline__ double avg4_cc(F f, int i, int j) { return avg4(f(i, j), f(i + 1, j), f(i, j + 1), f(i + 1, j + 1)); }   // from (f, f)
template <class F> __device__ __forceinline__ double avg4_fc(F f, int i, int j) { return avg4(f(i - 1, j), f(i, j), f(i - 1, j + 1), f(i, j + 1)); }   // from (c, f)
template <class F> __device__ __forceinline__ double avg4_cf(F f, int i, int j) { return avg4(f(i, j - 1), f(i + 1, j - 1), f(i, j), f(i + 1, j)); }   // from (f, c)

// ---- stress divergence, ice_stress_divergence.jl:16-51 -----------------------------------------------------------------------------
struct Sigma { FRef s11, s22, s12; };
__device__ __forceinline__ double sig11(const GridDev& g, const Sigma& S, int i, int j) { return immersed_peripheral_cc(g, i, j) ? 0.0 : S.s11.ld_(i, j); }
__device__ __forceinline__ double sig22(const GridDev& g, const Sigma& S, int i, int j) { return immersed_peripheral_cc(g, i, j) ? 0.0 : S.s22.ld_(i, j); }
__device__ __forceinline__ double sig12(const GridDev& g, const Sigma& S, int i, int j) { return immersed_peripheral_ff(g, i, j) ? 0.0 : S.s12.ld_(i, j); }
__device__ __forceinline__ double sigD(const GridDev& g, const Sigma& S, int i, int j) { return sig11(g, S, i, j) + sig22(g, S, i, j); }
__device__ __forceinline__ double sigT(const GridDev& g, const Sigma& S, int i, int j) { return sig11(g, S, i, j) - sig22(g, S, i, j); }

// the arithmetic on gathered values: the invariants sigma_11 +- sigma_22 at the two cells (0: the point's own index, m: one below) and
// the shear stress at the two corners (hi: one above, lo: the point's own index)
// u point, m: dy(f,c)(i,j), dy(c,c)(i,j), dy(c,c)(i-1,j), dx(f,f)(i,j+1), dx(f,f)(i,j), dx(f,c)(i,j), Az(f,c)(i,j)                  :39-44
__device__ __forceinline__ double div1_strict(const double* m, double sD0, double sDm, double sT0, double sTm, double sN, double sS) {
    const double dyfc = m[0], dyc = m[1], dycm = m[2], dxfn = m[3], dxf = m[4], dxfc = m[5], az = m[6];
    const double d = dyfc * (sD0 - sDm) / 2;
    const double T = ((dyc * dyc) * sT0 - (dycm * dycm) * sTm) / dyfc / 2;
    const double S = ((dxfn * dxfn) * sN - (dxf * dxf) * sS) / dxfc;
    return (d + T + S) / az;
}
// v point, m: dx(c,f)(i,j), dx(c,c)(i,j), dx(c,c)(i,j-1), dy(f,f)(i+1,j), dy(f,f)(i,j), dy(c,f)(i,j), Az(c,f)(i,j)                  :46-51
__device__ __forceinline__ double div2_strict(const double* m, double sD0, double sDm, double sT0, double sTm, double sE, double sW) {
    const double dxcf = m[0], dxc = m[1], dxcm = m[2], dyfn = m[3], dyf = m[4], dycf = m[5], az = m[6];
    const double d = dxcf * (sD0 - sDm) / 2;
    const double T = -((dxc * dxc) * sT0 - (dxcm * dxcm) * sTm) / dxcf / 2;
    const double S = ((dyfn * dyfn) * sE - (dyf * dyf) * sW) / dycf;
    return (d + T + S) / az;
}
// on fields, spelled out (the same operations in the same order as div1_strict / div2_strict: gathering the metrics into an array first
// costs the per-point instantiations registers)
template <int MK> __device__ __forceinline__ double div_sigma_1(const GridDev& g, const Sigma& P, int i, int j) {   // :39-44
    double dyfc = dy_<MK>(g, F_, C_, i, j);
    double d = dyfc * (sigD(g, P, i, j) - sigD(g, P, i - 1, j)) / 2;
    double dyc = dy_<MK>(g, C_, C_, i, j), dycm = dy_<MK>(g, C_, C_, i - 1, j);
    double T = ((dyc * dyc) * sigT(g, P, i, j) - (dycm * dycm) * sigT(g, P, i - 1, j)) / dyfc / 2;
    double dxfn = dx_<MK>(g, F_, F_, i, j + 1), dxf = dx_<MK>(g, F_, F_, i, j);
    double S = ((dxfn * dxfn) * sig12(g, P, i, j + 1) - (dxf * dxf) * sig12(g, P, i, j)) / dx_<MK>(g, F_, C_, i, j);
    return (d + T + S) / az_<MK>(g, F_, C_, i, j);
}
template <int MK> __device__ __forceinline__ double div_sigma_2(const GridDev& g, const Sigma& P, int i, int j) {   // :46-51
    double dxcf = dx_<MK>(g, C_, F_, i, j);
    double d = dxcf * (sigD(g, P, i, j) - sigD(g, P, i, j - 1)) / 2;
    double dxc = dx_<MK>(g, C_, C_, i, j), dxcm = dx_<MK>(g, C_, C_, i, j - 1);
    double T = -((dxc * dxc) * sigT(g, P, i, j) - (dxcm * dxcm) * sigT(g, P, i, j - 1)) / dxcf / 2;
    double dyfn = dy_<MK>(g, F_, F_, i + 1, j), dyf = dy_<MK>(g, F_, F_, i, j);
    double S = ((dyfn * dyfn) * sig12(g, P, i + 1, j) - (dyf * dyf) * sig12(g, P, i, j)) / dy_<MK>(g, C_, F_, i, j);
    return (d + T + S) / az_<MK>(g, C_, F_, i, j);
}
#undef F_
#undef C_

}  // namespace dv
}  // namespace csi
