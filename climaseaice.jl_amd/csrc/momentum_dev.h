// momentum_dev.h -- the point-wise velocity sub-step: the tendencies and the closing part.  Users: the STRICT EVP velocity steps
// (evp_strict.hip, FAST = false, VISC = false), ViscousRheology (momentum_viscous.hip), the ExplicitSolver (momentum_explicit.hip),
// the momentum balance terms (momentum_terms.hip, the front half) and, for the gather helpers, momentum_free_drift.hip.  gfx950 only.
//
//   u_velocity_tendency / v_velocity_tendency   SeaIceDynamics/momentum_tendencies_kernel_functions.jl:11-74
//   ViscousRheology stresses                    Rheologies/viscous_rheology.jl:15-22 (nu a Number)
//   stress divergence, conditional fluxes       Rheologies/ice_stress_divergence.jl:16-51
//   immersed flux term                          :65-123
//   sum_of_forcing_* / sub-step                 Rheologies/Rheologies.jl:42-55 (viscous), elasto_visco_plastic_rheology.jl:391-401 (EVP)
//
// One function per velocity point, templated on the arithmetic (STRICT: the reference's operation order, no contraction;
// FAST: explicit FMAs, reciprocals hoisted) and on the stresses (VISC: nu * delta u inline; otherwise the stored sigma fields).
// Both issue every load of the point before the first value is used (the lesson of profiles/r06_band.md): the velocities, h,
// aice, the stored stresses, the metrics, the mask bytes and the optional operands (Coriolis parameter, stress arrays, forcing,
// free drift) are gathered first with UNCONDITIONAL loads -- an operand the configuration does not have is loaded from a valid
// address the point reads anyway and discarded by a select (a load inside a branch is waited for where the branch joins) --, the
// arithmetic follows on registers.  tests/test_momentum_variants.py gates the generated code.
#pragma once
#include "csi_dev.h"
#include "derived_dev.h"

namespace csi {

enum : int { RHEO_EVP = 0, RHEO_VISCOUS = 1 };

struct MomDev {
    EvpDev P;          // grid, state (P.u / P.v: the arrays the launch reads), stresses, Coriolis, forcing, free drift, dt
    FRef out;          // the component the launch writes, with its halo images (viscous sub-step, explicit step)
    FRef Gu, Gv;       // explicit solver: timestepper.G^n.u / .v
    FRef um, vm;       // explicit solver: u^- / v^- (RK3: Psi^-; FE: the velocities themselves)
    double nu;         // ViscousRheology(nu::Number)
};

void launch_viscous_ustep(const MomDev& M, const Range& r, const ImageSpec& im, int fast, hipStream_t s);
void launch_viscous_vstep(const MomDev& M, const Range& r, const ImageSpec& im, int fast, hipStream_t s);
void launch_explicit_tendencies(const MomDev& M, const Range& r, int viscous, int fast, hipStream_t s);
void launch_explicit_ustep(const MomDev& M, const Range& r, const ImageSpec& im, int fast, hipStream_t s);
void launch_explicit_vstep(const MomDev& M, const Range& r, const ImageSpec& im, int fast, hipStream_t s);

namespace mom {

#define MOM_EPS64 2.220446049250313e-16

// ---- the cells a velocity point's predicates look at: 2 x 3 (u point: i-1..i, j-1..j+1) or 3 x 2 (v point: i-1..i+1, j-1..j) ----
// the mask byte of every cell is loaded from a clamped index without a branch per cell (csi_dev.h inactive_cell), all six before any test
struct Cells {
    uint8_t byte[6];
    bool inact[6], under[6];
};
// cell (i0 + a, j0 + b), a < NA, b < NB, stored at [a + NA * b].  gather_cells only issues the loads; resolve_cells, called once
// everything of the point is in flight, evaluates the predicates
// (without a mask the bytes come from `safe`, a valid address, and are never looked at)
template <int NA, int NB>
__device__ __forceinline__ void gather_cells(const GridDev& g, int i0, int j0, const void* safe, Cells& c) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const int i = i0 + a, j = j0 + b;
            const int ic = min(max(i, 1 - g.Hx), g.Nx + g.Hx), jc = min(max(j, 1 - g.Hy), g.Ny + g.Hy);
            const uint8_t* m = g.has_mask ? g.mask + (ic + (long)jc * g.mask_ld) : (const uint8_t*)safe;
            c.byte[a + NA * b] = *m;
        }
}
template <int NA, int NB>
__device__ __forceinline__ void resolve_cells(const GridDev& g, int i0, int j0, Cells& c) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const int i = i0 + a, j = j0 + b, k = a + NA * b;
            c.under[k] = inactive_cell_underlying(g, i, j);
            bool out = c.under[k];
            if (g.has_mask) {
                const bool beyond = (i < 1 - g.Hx) | (i > g.Nx + g.Hx) | (j < 1 - g.Hy) | (j > g.Ny + g.Hy);
                out |= beyond | (c.byte[k] == 0);
            }
            c.inact[k] = out;
        }
}
// immersed_peripheral_node at (c, c, c) of cell k / at (f, f, c) of the corner whose four cells are k, k + 1, k + na, k + na + 1
__device__ __forceinline__ bool ipcc(const GridDev& g, const Cells& c, int k) { return g.has_mask && c.inact[k] && !c.under[k]; }
template <int NA>
__device__ __forceinline__ bool ipff(const GridDev& g, const Cells& c, int k) {
    const bool p = c.inact[k] | c.inact[k + 1] | c.inact[k + NA] | c.inact[k + NA + 1];
    const bool pu = c.under[k] | c.under[k + 1] | c.under[k + NA] | c.under[k + NA + 1];
    return g.has_mask && p && !pu;
}

// ---- unconditional loads ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ const double* addr(const FRef& f, int i, int j) { return f.p + (i + (long)j * f.ld); }
// `use` ? *p : otherwise, with ONE load from a selected address (safe: any valid address) and no branch around it
__device__ __forceinline__ double ld_sel(bool use, const double* p, const double* safe, double otherwise) {
    const double x = *(use ? p : safe);
    return use ? x : otherwise;
}
// dxm / dym / azm (csi_dev.h) as an unconditional load: which 0 dx, 1 dy, 2 Az.  Same values, same arithmetic (Az = dx * dy on
// uniform metrics)
__device__ __forceinline__ double met(const GridDev& g, int which, int lx, int ly, int i, int j, const double* safe) {
    // both candidate addresses computed without a branch (only the selected one is dereferenced)
    const double* p2 = g.m2 + ((4 * which + (lx == LOC_F ? 1 : 0) + (ly == LOC_F ? 2 : 0)) * g.m2_plane + i + (long)j * g.m2_ld);
    const double* p1 = (which == 0 ? (ly == LOC_C ? g.dxc : g.dxf) : (ly == LOC_C ? g.azc : g.azf)) + j;
    const bool use2 = g.metric_kind == 2, use1 = (g.metric_kind == 1) & (which != 1);
    const double x = *(use2 ? p2 : (use1 ? p1 : safe));
    const double c = which == 0 ? g.dx : (which == 1 ? g.dy : g.dx * g.dy);
    return (use2 | use1) ? x : c;
}

// ---- arithmetic: STRICT spells the reference's expression, FAST the same terms with FMAs and reciprocals ---------------------
// a * x - b * y
template <bool FAST> __device__ __forceinline__ double msub(double a, double x, double b, double y) {
    return FAST ? fma(a, x, -(b * y)) : a * x - b * y;
}

// the divergence of (sigma_11, sigma_12) at a u point (ice_stress_divergence.jl:36-44) from the invariants at the cells i, i - 1
// and the shear stress at the corners j + 1 (N), j (S); STRICT: derived_dev.h div1_strict, which also names the seven metrics of m
template <bool FAST>
__device__ __forceinline__ double div1(const double* m, double sD0, double sDm, double sT0, double sTm, double sN, double sS) {
    if (!FAST) return dv::div1_strict(m, sD0, sDm, sT0, sTm, sN, sS);
    const double dyfc = m[0], dyc = m[1], dycm = m[2], dxfn = m[3], dxf = m[4], dxfc = m[5], az = m[6];
    const double rdy = 1.0 / dyfc;
    const double T = msub<true>(dyc * dyc, sT0, dycm * dycm, sTm) * (0.5 * rdy);
    const double S = msub<true>(dxfn * dxfn, sN, dxf * dxf, sS) * (1.0 / dxfc);
    return fma(0.5 * dyfc, sD0 - sDm, T + S) * (1.0 / az);
}
// ... of (sigma_21, sigma_22) at a v point (:46-51): invariants at the cells j, j - 1, shear stress at the corners i + 1 (E), i (W)
template <bool FAST>
__device__ __forceinline__ double div2(const double* m, double sD0, double sDm, double sT0, double sTm, double sE, double sW) {
    if (!FAST) return dv::div2_strict(m, sD0, sDm, sT0, sTm, sE, sW);
    const double dxcf = m[0], dxc = m[1], dxcm = m[2], dyfn = m[3], dyf = m[4], dycf = m[5], az = m[6];
    const double rdx = 1.0 / dxcf;
    const double T = msub<true>(dxc * dxc, sT0, dxcm * dxcm, sTm) * (-0.5 * rdx);
    const double S = msub<true>(dyfn * dyfn, sE, dyf * dyf, sW) * (1.0 / dycf);
    return fma(0.5 * dxcf, sD0 - sDm, T + S) * (1.0 / az);
}

// ---- external stresses (sea_ice_external_stress.jl:8-27,176-202) on gathered values -----------------------------------------
// what a stress needs at a point: its own component there (tau array / external velocity) and the other component at the four
// points of the cross average
struct StressPt {
    double own, x4[4];
};
// (kind 2: tau array at the point; kind 3: the external velocity, an array (kind 2), a number (1) or zero (0); other kinds: nothing.
//  safe_own / safe_x: valid addresses of the point and of the four cross points)
__device__ __forceinline__ void gather_stress(const StressDev& s, const FRef& own_arr, int own_kind, double own_num, const FRef& x_arr, int x_kind,
                                              double x_num, int i, int j, const int (*xp)[2], const double* safe_own, const double* const* safe_x,
                                              StressPt& p) {
    const bool own_a = (s.kind == 2) | ((s.kind == 3) & (own_kind == 2));
    p.own = ld_sel(own_a, addr(own_arr, i, j), safe_own, ((s.kind == 3) & (own_kind == 1)) ? own_num : 0.0);
    const bool x_a = (s.kind == 3) & (x_kind == 2);
    const double x_c = ((s.kind == 3) & (x_kind == 1)) ? x_num : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) p.x4[k] = ld_sel(x_a, addr(x_arr, xp[k][0], xp[k][1]), safe_x[k], x_c);
}
// u point: own = tau_x / u_e at (i, j); x4 = v_e at (i-1, j), (i, j), (i-1, j+1), (i, j+1)
__device__ __forceinline__ void gather_stress_u(const StressDev& s, const FRef& U, const FRef& V, int i, int j, StressPt& p) {
    const int xp[4][2] = {{i - 1, j}, {i, j}, {i - 1, j + 1}, {i, j + 1}};
    const double* sx[4] = {addr(V, i - 1, j), addr(V, i, j), addr(V, i - 1, j + 1), addr(V, i, j + 1)};
    gather_stress(s, s.fu, s.ue_kind, s.ue, s.fv, s.ve_kind, s.ve, i, j, xp, addr(U, i, j), sx, p);
}
// v point: own = tau_y / v_e at (i, j); x4 = u_e at (i, j-1), (i+1, j-1), (i, j), (i+1, j)
__device__ __forceinline__ void gather_stress_v(const StressDev& s, const FRef& U, const FRef& V, int i, int j, StressPt& p) {
    const int xp[4][2] = {{i, j - 1}, {i + 1, j - 1}, {i, j}, {i + 1, j}};
    const double* sx[4] = {addr(U, i, j - 1), addr(U, i + 1, j - 1), addr(U, i, j), addr(U, i + 1, j)};
    gather_stress(s, s.fv, s.ve_kind, s.ve, s.fu, s.ue_kind, s.ue, i, j, xp, addr(V, i, j), sx, p);
}
// |U_e - U| at the point: own component difference and the cross average
__device__ __forceinline__ double drag_norm(const StressPt& p, double own_vel, const double* x_vel4) {
    const double d1 = p.own - own_vel;
    const double d2 = avg4(p.x4) - avg4(x_vel4);
    return sqrt(d1 * d1 + d2 * d2);
}
__device__ __forceinline__ double explicit_tau(const StressDev& s, const StressPt& p, const double* tau_const, double own_vel, const double* x_vel4) {
    switch (s.kind) {
        case 1: return *tau_const;
        case 2: return p.own;
        case 3: return s.rho_e * s.Cd * drag_norm(p, own_vel, x_vel4) * p.own;
        default: return 0.0;
    }
}
__device__ __forceinline__ double implicit_tau(const StressDev& s, const StressPt& p, double own_vel, const double* x_vel4) {
    return s.kind == 3 ? s.rho_e * s.Cd * drag_norm(p, own_vel, x_vel4) : 0.0;
}

// ---- everything a u point reads (gathered first) ----------------------------------------------------------------------------
struct UPoint {
    double uc, uw, ue, us, un;          // u at (i, j), (i -+ 1, j), (i, j -+ 1)
    double v4[4];                       // v at (i-1, j), (i, j), (i-1, j+1), (i, j+1)
    double hw, he, aw, ae;              // h, aice at (i-1, j), (i, j)
    double s11w, s11e, s22w, s22e, s12s, s12n;   // stored stresses (EVP): cells i-1, i; corners j, j+1
    double unn, alw, ale;               // EVP: u^n at the point, alpha at the cells
    double f, user, fd;                 // Coriolis parameter, model.forcing.u, free-drift velocity
    double m[7];                        // metrics of div1 (and of the immersed flux term)
    StressPt top, bot;
    Cells c;                            // cells (i-1..i) x (j-1..j+1)
};
struct VPoint {
    double vc, vs, vn, vw, ve;          // v at (i, j), (i, j -+ 1), (i -+ 1, j)
    double u4[4];                       // u at (i, j-1), (i+1, j-1), (i, j), (i+1, j)
    double hs, hn, as_, an;             // h, aice at (i, j-1), (i, j)
    double s11s, s11n, s22s, s22n, s12w, s12e;   // cells j-1, j; corners i, i+1
    double vnn, als, aln;
    double f, user, fd;
    double m[7];                        // metrics of div2 (and of the immersed flux term)
    StressPt top, bot;
    Cells c;                            // cells (i-1..i+1) x (j-1..j)
};

// U: the u array the point reads (the launch's input), V: the current v.  Only the viscous stencil reads the own component at the
// four neighbours: the EVP steps store in place, and those are cells that other threads are writing
template <bool VISC>
__device__ __forceinline__ void gather_u(const EvpDev& P, const FRef& U, const FRef& V, int i, int j, UPoint& q) {
    q.uc = U(i, j);
    if (VISC) { q.uw = U(i - 1, j); q.ue = U(i + 1, j); q.us = U(i, j - 1); q.un = U(i, j + 1); }
    q.v4[0] = V(i - 1, j); q.v4[1] = V(i, j); q.v4[2] = V(i - 1, j + 1); q.v4[3] = V(i, j + 1);
    q.hw = P.h(i - 1, j); q.he = P.h(i, j); q.aw = P.a(i - 1, j); q.ae = P.a(i, j);
    if (!VISC) {
        q.s11w = P.s11(i - 1, j); q.s11e = P.s11(i, j); q.s22w = P.s22(i - 1, j); q.s22e = P.s22(i, j);
        q.s12s = P.s12(i, j); q.s12n = P.s12(i, j + 1);
        q.unn = P.un(i, j); q.alw = P.al(i - 1, j); q.ale = P.al(i, j);
    }
    const double* safe = addr(U, i, j);
    const GridDev& g = P.g;
    q.m[0] = met(g, 1, LOC_F, LOC_C, i, j, safe); q.m[1] = met(g, 1, LOC_C, LOC_C, i, j, safe); q.m[2] = met(g, 1, LOC_C, LOC_C, i - 1, j, safe);
    q.m[3] = met(g, 0, LOC_F, LOC_F, i, j + 1, safe); q.m[4] = met(g, 0, LOC_F, LOC_F, i, j, safe); q.m[5] = met(g, 0, LOC_F, LOC_C, i, j, safe);
    q.m[6] = met(g, 2, LOC_F, LOC_C, i, j, safe);
    // fcor_at_u (csi_dev.h): per point, per row or the number
    const double* pc = P.fcor2_u ? P.fcor2_u + (i + (long)j * P.fcor2_ld) : (P.fcor_u ? P.fcor_u + j : nullptr);
    q.f = ld_sel(P.has_cor && pc, pc, safe, P.has_cor ? P.fcor : 0.0);
    q.user = ld_sel(P.has_forcing, addr(P.forcing_u, i, j), safe, 0.0);
    q.fd = ld_sel(P.free_drift, addr(P.ufd, i, j), safe, 0.0);
    gather_stress_u(P.top, U, V, i, j, q.top);
    gather_stress_u(P.bot, U, V, i, j, q.bot);
    gather_cells<2, 3>(g, i - 1, j - 1, safe, q.c);
}
template <bool VISC>
__device__ __forceinline__ void gather_v(const EvpDev& P, const FRef& U, const FRef& V, int i, int j, VPoint& q) {
    q.vc = V(i, j);
    if (VISC) { q.vs = V(i, j - 1); q.vn = V(i, j + 1); q.vw = V(i - 1, j); q.ve = V(i + 1, j); }
    q.u4[0] = U(i, j - 1); q.u4[1] = U(i + 1, j - 1); q.u4[2] = U(i, j); q.u4[3] = U(i + 1, j);
    q.hs = P.h(i, j - 1); q.hn = P.h(i, j); q.as_ = P.a(i, j - 1); q.an = P.a(i, j);
    if (!VISC) {
        q.s11s = P.s11(i, j - 1); q.s11n = P.s11(i, j); q.s22s = P.s22(i, j - 1); q.s22n = P.s22(i, j);
        q.s12w = P.s12(i, j); q.s12e = P.s12(i + 1, j);
        q.vnn = P.vn(i, j); q.als = P.al(i, j - 1); q.aln = P.al(i, j);
    }
    const double* safe = addr(V, i, j);
    const GridDev& g = P.g;
    q.m[0] = met(g, 0, LOC_C, LOC_F, i, j, safe); q.m[1] = met(g, 0, LOC_C, LOC_C, i, j, safe); q.m[2] = met(g, 0, LOC_C, LOC_C, i, j - 1, safe);
    q.m[3] = met(g, 1, LOC_F, LOC_F, i + 1, j, safe); q.m[4] = met(g, 1, LOC_F, LOC_F, i, j, safe); q.m[5] = met(g, 1, LOC_C, LOC_F, i, j, safe);
    q.m[6] = met(g, 2, LOC_C, LOC_F, i, j, safe);
    const double* pc = P.fcor2_v ? P.fcor2_v + (i + (long)j * P.fcor2_ld) : (P.fcor_v ? P.fcor_v + j : nullptr);
    q.f = ld_sel(P.has_cor && pc, pc, safe, P.has_cor ? P.fcor : 0.0);
    q.user = ld_sel(P.has_forcing, addr(P.forcing_v, i, j), safe, 0.0);
    q.fd = ld_sel(P.free_drift, addr(P.vfd, i, j), safe, 0.0);
    gather_stress_v(P.top, U, V, i, j, q.top);
    gather_stress_v(P.bot, U, V, i, j, q.bot);
    gather_cells<3, 2>(g, i - 1, j - 1, safe, q.c);
}

// ---- the front half of a tendency: everything up to the stress divergence, shared by the stepping kernels (u_tendency / v_tendency)
// and by the kernels that keep the terms apart (momentum_terms.hip, with FAST = false) ------------------------------------------------
// mi, ai: the interpolated ice mass (ClimaSeaIce.jl:42) and concentration; c0, c1 / f0, f1: the immersed-peripheral predicates of the
// point's two cells / two corners (lower index first); div: the stress divergence with the conditional fluxes; imm: the immersed
// flux term -- both per unit area, not yet divided by mi
struct Front {
    double mi, ai, div, imm;
    bool c0, c1, f0, f1;
};
template <bool FAST, bool VISC>
__device__ __forceinline__ Front u_front(const EvpDev& P, double nu, UPoint& q, int i, int j) {
    const GridDev& g = P.g;
    Front r;
    resolve_cells<2, 3>(g, i - 1, j - 1, q.c);
    r.mi = (q.hw * P.rho * q.aw + q.he * P.rho * q.ae) / 2;        // Ixᶠᵃᵃ
    r.ai = (q.aw + q.ae) / 2;
    // corners: (i, j) = cells 0, 1, 2, 3; (i, j + 1) = cells 2, 3, 4, 5.  Cells (i-1, j) = 2, (i, j) = 3
    const bool cw = ipcc(g, q.c, 2), ce = ipcc(g, q.c, 3), fs = ipff<2>(g, q.c, 0), fn = ipff<2>(g, q.c, 2);
    double s11w, s11e, s22w, s22e, s12s, s12n;
    if (VISC) {                                                     // viscous_rheology.jl:15-22: nu * delta
        s11w = nu * (q.uc - q.uw); s11e = nu * (q.ue - q.uc);        // ux at cells i - 1, i
        s22w = nu * (q.v4[2] - q.v4[0]); s22e = nu * (q.v4[3] - q.v4[1]);   // vy
        s12s = nu * (q.uc - q.us); s12n = nu * (q.un - q.uc);        // uy at corners (i, j), (i, j + 1)
    } else {
        s11w = q.s11w; s11e = q.s11e; s22w = q.s22w; s22e = q.s22e; s12s = q.s12s; s12n = q.s12n;
    }
    // conditional_flux_ccc / _ffc (ice_stress_divergence.jl:21-24)
    s11w = cw ? 0.0 : s11w; s22w = cw ? 0.0 : s22w;
    s11e = ce ? 0.0 : s11e; s22e = ce ? 0.0 : s22e;
    s12s = fs ? 0.0 : s12s; s12n = fn ? 0.0 : s12n;
    r.div = div1<FAST>(q.m, s11e + s22e, s11w + s22w, s11e - s22e, s11w - s22w, s12n, s12s);
    // immersed_dj_sigma_1j (:65-92): west / east faces are the cells i - 1, i; south / north the corners j, j + 1
    r.imm = 0.0;
    if (g.has_mask) {
        const double qW = (cw ? -P.ibc_u[0] : 0.0) * q.m[2];          // dy(c,c)(i-1, j)
        const double qE = (ce ? P.ibc_u[1] : 0.0) * q.m[1];           // dy(c,c)(i, j)
        const double qS = (fs ? -P.ibc_u[2] : 0.0) * q.m[4];          // dx(f,f)(i, j)
        const double qN = (fn ? P.ibc_u[3] : 0.0) * q.m[3];           // dx(f,f)(i, j + 1)
        r.imm = (qE - qW + qN - qS) / q.m[6];
    }
    r.c0 = cw; r.c1 = ce; r.f0 = fs; r.f1 = fn;
    return r;
}
template <bool FAST, bool VISC>
__device__ __forceinline__ Front v_front(const EvpDev& P, double nu, VPoint& q, int i, int j) {
    const GridDev& g = P.g;
    Front r;
    resolve_cells<3, 2>(g, i - 1, j - 1, q.c);
    r.mi = (q.hs * P.rho * q.as_ + q.hn * P.rho * q.an) / 2;
    r.ai = (q.as_ + q.an) / 2;
    // cells (i-1..i+1) x (j-1..j): (i, j-1) = 1, (i, j) = 4; corners (i, j) = cells 0, 1, 3, 4; (i + 1, j) = cells 1, 2, 4, 5
    const bool cs = ipcc(g, q.c, 1), cn = ipcc(g, q.c, 4), fw = ipff<3>(g, q.c, 0), fe = ipff<3>(g, q.c, 1);
    double s11s, s11n, s22s, s22n, s12w, s12e;
    if (VISC) {
        s11s = nu * (q.u4[1] - q.u4[0]); s11n = nu * (q.u4[3] - q.u4[2]);   // ux at cells j - 1, j
        s22s = nu * (q.vc - q.vs); s22n = nu * (q.vn - q.vc);                // vy
        s12w = nu * (q.vc - q.vw); s12e = nu * (q.ve - q.vc);                // vx at corners (i, j), (i + 1, j)
    } else {
        s11s = q.s11s; s11n = q.s11n; s22s = q.s22s; s22n = q.s22n; s12w = q.s12w; s12e = q.s12e;
    }
    s11s = cs ? 0.0 : s11s; s22s = cs ? 0.0 : s22s;
    s11n = cn ? 0.0 : s11n; s22n = cn ? 0.0 : s22n;
    s12w = fw ? 0.0 : s12w; s12e = fe ? 0.0 : s12e;
    r.div = div2<FAST>(q.m, s11n + s22n, s11s + s22s, s11n - s22n, s11s - s22s, s12e, s12w);
    r.imm = 0.0;
    if (g.has_mask) {                                                // immersed_dj_sigma_2j (:94-123)
        const double qW = (fw ? -P.ibc_v[0] : 0.0) * q.m[4];          // dy(f,f)(i, j)
        const double qE = (fe ? P.ibc_v[1] : 0.0) * q.m[3];           // dy(f,f)(i + 1, j)
        const double qS = (cs ? -P.ibc_v[2] : 0.0) * q.m[2];          // dx(c,c)(i, j - 1)
        const double qN = (cn ? P.ibc_v[3] : 0.0) * q.m[1];           // dx(c,c)(i, j)
        r.imm = (qE - qW + qN - qS) / q.m[6];
    }
    r.c0 = cs; r.c1 = cn; r.f0 = fw; r.f1 = fe;
    return r;
}

// ---- the tendency at a u point (u_velocity_tendency, :11-41) ----------------------------------------------------------------
// dt_forcing: the Delta t of sum_of_forcing_u (EVP only).  Returns G; mi, ai: the interpolated mass and concentration
template <bool FAST, bool VISC>
__device__ __forceinline__ double u_tendency(const EvpDev& P, double nu, UPoint& q, int i, int j, double dt_forcing, double& mi, double& ai) {
    const Front fr = u_front<FAST, VISC>(P, nu, q, i, j);
    mi = fr.mi; ai = fr.ai;
    const double div = fr.div, imm = fr.imm;
    const double cor = P.has_cor ? -q.f * avg4(q.v4) : 0.0;          // x_f_cross_U
    double forcing = q.user;                                          // sum_of_forcing_u: viscous = the user forcing alone
    if (!VISC) forcing = q.user + (q.unn - q.uc) / dt_forcing / ((q.alw + q.ale) / 2);
    const double ttop = explicit_tau(P.top, q.top, &P.top.tau_u, q.uc, q.v4);
    const double tbot = explicit_tau(P.bot, q.bot, &P.bot.tau_u, q.uc, q.v4);
    double G;
    if (FAST) {
        const double rmi = 1.0 / mi;
        G = -cor + (tbot - ttop) * (rmi * ai) + (div + imm) * rmi + forcing;
    } else {
        G = (-cor - ttop / mi * ai + tbot / mi * ai + div / mi + imm / mi + forcing);
    }
    return (mi <= 0) ? 0.0 : G;
}
template <bool FAST, bool VISC>
__device__ __forceinline__ double v_tendency(const EvpDev& P, double nu, VPoint& q, int i, int j, double dt_forcing, double& mi, double& ai) {
    const Front fr = v_front<FAST, VISC>(P, nu, q, i, j);
    mi = fr.mi; ai = fr.ai;
    const double div = fr.div, imm = fr.imm;
    const double cor = P.has_cor ? q.f * avg4(q.u4) : 0.0;            // y_f_cross_U
    double forcing = q.user;
    if (!VISC) forcing = q.user + (q.vnn - q.vc) / dt_forcing / ((q.als + q.aln) / 2);
    const double ttop = explicit_tau(P.top, q.top, &P.top.tau_v, q.vc, q.u4);
    const double tbot = explicit_tau(P.bot, q.bot, &P.bot.tau_v, q.vc, q.u4);
    double G;
    if (FAST) {
        const double rmi = 1.0 / mi;
        G = -cor + (tbot - ttop) * (rmi * ai) + (div + imm) * rmi + forcing;
    } else {
        G = (-cor - ttop / mi * ai + tbot / mi * ai + div / mi + imm / mi + forcing);
    }
    return (mi <= 0) ? 0.0 : G;
}

// (implicit_bot - implicit_top) / m * aice at the point
template <bool FAST>
__device__ __forceinline__ double implicit_coef(const EvpDev& P, const StressPt& top, const StressPt& bot, double own, const double* x4, double mi, double ai) {
    const double d = implicit_tau(P.bot, bot, own, x4) - implicit_tau(P.top, top, own, x4);
    return FAST ? d * ((1.0 / mi) * ai) : d / mi * ai;
}

// ---- the closing part of a sub-step, once for both components and every stepping kernel (split_explicit_momentum_equations.jl:215-228,
// :249-263; explicit_momentum_equations.jl:40-82) ----------------------------------------------------------------------------------
// x: the velocity the step starts from (the point's own; u^- / v^- for the ExplicitSolver), G its tendency, tau_i the implicit
// coefficient, fd the free-drift value, mi / ai the interpolated mass and concentration.  The semi-implicit solve, then the select:
// active ice takes the solve, marginal ice the free drift, the rest zero.
// SPLIT: the split-explicit kernels guard tau_i where m <= 0 and multiply by `active` -- a Julia Bool, so a peripheral point gets a
// strong zero that keeps the sign (:228).  The ExplicitSolver's steps have neither (momentum_explicit.hip's header): SPLIT = false
template <bool FAST, bool SPLIT>
__device__ __forceinline__ double close_substep(const EvpDev& P, double x, double G, double tau_i, double dtau, double fd, double mi, double ai,
                                                bool peripheral) {
    if (SPLIT) tau_i = (mi <= 0) ? 0.0 : tau_i;
    const double xD = FAST ? fma(dtau, G, x) / fma(dtau, tau_i, 1.0) : (x + dtau * G) / (1 + dtau * tau_i);
    const double xF = P.free_drift ? fd : 0.0;
    const bool marginal = (mi > MOM_EPS64) & (ai > MOM_EPS64);
    const bool active_ice = (mi >= P.min_mass) & (ai >= P.min_conc);
    const double sel = active_ice ? xD : (marginal ? xF : 0.0);
    return (SPLIT && peripheral) ? copysign(0.0, sel) : sel;
}

}  // namespace mom
}  // namespace csi
