// derived_dev.h -- the reference's strain rates and stress divergence for the derived-field and energy-budget kernels (derived.hip,
// budget.hip; include/csi.h "derived fields and energy budget integrals").
//
// The same expressions, in the same operation order, as evp_strict.hip eps_D / eps_T / eps_S and div_sigma_1 / div_sigma_2 (which stay
// where they are: the objects of the stepping kernels do not change), restated on bare field references instead of an EvpDev and with
// the metric kind as a template parameter: MK = 0 uniform (two numbers), 1 per row (vectors indexed by j), 2 per point (twelve planes).
// Units that include this header are compiled without contraction.
#pragma once
#include "csi_dev.h"

namespace csi {
namespace dv {

template <int MK> __device__ __forceinline__ double dx_(const GridDev& g, int lx, int ly, int i, int j) {
    if (MK == 0) return g.dx;
    if (MK == 1) return ly == LOC_C ? g.dxc[j] : g.dxf[j];
    return metric2(g, 0, lx, ly, i, j);
}
template <int MK> __device__ __forceinline__ double dy_(const GridDev& g, int lx, int ly, int i, int j) {
    if (MK != 2) return g.dy;
    return metric2(g, 1, lx, ly, i, j);
}
template <int MK> __device__ __forceinline__ double az_(const GridDev& g, int lx, int ly, int i, int j) {
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
// Ixy of four corner values: ((f(i, j) + f(i + 1, j)) / 2 + (f(i, j + 1) + f(i + 1, j + 1)) / 2) / 2
__device__ __forceinline__ double avg4(double f00, double f10, double f01, double f11) { return ((f00 + f10) / 2 + (f01 + f11) / 2) / 2; }

// ---- stress divergence, ice_stress_divergence.jl:16-51 -----------------------------------------------------------------------------
struct Sigma { FRef s11, s22, s12; };
__device__ __forceinline__ double sig11(const GridDev& g, const Sigma& S, int i, int j) { return immersed_peripheral_cc(g, i, j) ? 0.0 : S.s11.ld_(i, j); }
__device__ __forceinline__ double sig22(const GridDev& g, const Sigma& S, int i, int j) { return immersed_peripheral_cc(g, i, j) ? 0.0 : S.s22.ld_(i, j); }
__device__ __forceinline__ double sig12(const GridDev& g, const Sigma& S, int i, int j) { return immersed_peripheral_ff(g, i, j) ? 0.0 : S.s12.ld_(i, j); }
__device__ __forceinline__ double sigD(const GridDev& g, const Sigma& S, int i, int j) { return sig11(g, S, i, j) + sig22(g, S, i, j); }
__device__ __forceinline__ double sigT(const GridDev& g, const Sigma& S, int i, int j) { return sig11(g, S, i, j) - sig22(g, S, i, j); }

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
