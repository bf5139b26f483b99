// momentum_terms.hip -- the terms of the velocity tendencies kept apart, and their power (include/csi.h: csi_momentum_terms_compute,
// csi_momentum_budget_compute).  gfx950 only.
//
//   k_momentum_terms<VISC>   one thread per index (i, j): the u point and the v point there; blocks of 64 x 4 threads, consecutive lanes
//                            on consecutive columns; the grid rounds up over i = 1 .. Nx + exu, j = 1 .. Ny + eyv, so the last face
//                            column / row of a Bounded side is covered; a thread beyond a field's own extent stores nothing for that
//                            component (its loads come from indices clamped into the extent)
//   k_momentum_power<VISC>   one pass over i = 1 .. Nx, j = 1 .. Ny; each block of 64 x 64 cells writes one record of MQ_COUNT sums
//   k_momentum_power_finish  ONE block folds the records
// The arithmetic is momentum_dev.h's, included unchanged: gather_u / gather_v issue every load of a point before the first value is
// used, resolve_cells evaluates the predicates, div1 / div2 (strict order), explicit_tau, drag_norm and the immersed flux term form what
// u_tendency / v_tendency (momentum_tendencies_kernel_functions.jl:11-74) add up and throw away.  Here the pieces are kept, each scaled
// to a force per unit area as include/csi.h states.  The stores are the last statements; output arrays never alias inputs.
// ONE code path for STRICT and FAST: compiled without contraction, IEEE division and square root.  No atomics, no flags; the field
// kernel uses no LDS.  The power sums follow the two-launch scheme and the SUMMATION ORDER of diagnostics.hip / budget.hip: thread
// (tx, ty) adds the cells of column tx in rows ty, ty + 4, ..., ty + 60 of the block's tile from +0.0, the wave combines over lane offsets
// 32 .. 1 (xor butterfly), the block adds its four waves in wave order, the finishing block's thread t adds records t, t + 256, ... and
// folds the same way.  A lane or row beyond the grid contributes +0.0; its loads come from indices clamped into the interior.
#include "csi_kernels.h"
#include "momentum_dev.h"

namespace csi {
namespace mt {
using namespace mom;

// x_momentum_stress / y_momentum_stress (sea_ice_external_stress.jl:33-37, 162-174): explicit - implicit * u; for a SemiImplicitStress
// the one product ((rho_e * C_D) * |dU|) * du
__device__ __forceinline__ double total_tau(const StressDev& s, const StressPt& p, const double* tau_const, double own_vel, const double* x_vel4) {
    if (s.kind == 3) return s.rho_e * s.Cd * drag_norm(p, own_vel, x_vel4) * (p.own - own_vel);
    return explicit_tau(s, p, tau_const, own_vel, x_vel4);
}

// the five terms at a u point, F[MQ_*], from the gathered point
template <bool VISC>
__device__ __forceinline__ void u_terms(const MomTermsDev& T, UPoint& q, int i, int j, double (&F)[MQ_COUNT]) {
    const EvpDev& P = T.P;
    const GridDev& g = P.g;
    resolve_cells<2, 3>(g, i - 1, j - 1, q.c);
    const double mi = (q.hw * P.rho * q.aw + q.he * P.rho * q.ae) / 2;
    const double ai = (q.aw + q.ae) / 2;
    // corners: (i, j) = cells 0, 1, 2, 3; (i, j + 1) = cells 2, 3, 4, 5.  Cells (i-1, j) = 2, (i, j) = 3
    const bool cw = ipcc(g, q.c, 2), ce = ipcc(g, q.c, 3), fs = ipff<2>(g, q.c, 0), fn = ipff<2>(g, q.c, 2);
    double s11w, s11e, s22w, s22e, s12s, s12n;
    if (VISC) {
        s11w = T.nu * (q.uc - q.uw); s11e = T.nu * (q.ue - q.uc);
        s22w = T.nu * (q.v4[2] - q.v4[0]); s22e = T.nu * (q.v4[3] - q.v4[1]);
        s12s = T.nu * (q.uc - q.us); s12n = T.nu * (q.un - q.uc);
    } else {
        s11w = q.s11w; s11e = q.s11e; s22w = q.s22w; s22e = q.s22e; s12s = q.s12s; s12n = q.s12n;
    }
    s11w = cw ? 0.0 : s11w; s22w = cw ? 0.0 : s22w;
    s11e = ce ? 0.0 : s11e; s22e = ce ? 0.0 : s22e;
    s12s = fs ? 0.0 : s12s; s12n = fn ? 0.0 : s12n;
    const double div = div1<false>(q.m, s11e + s22e, s11w + s22w, s11e - s22e, s11w - s22w, s12n, s12s);
    double imm = 0.0;
    if (g.has_mask) {
        const double qW = (cw ? -P.ibc_u[0] : 0.0) * q.m[2];
        const double qE = (ce ? P.ibc_u[1] : 0.0) * q.m[1];
        const double qS = (fs ? -P.ibc_u[2] : 0.0) * q.m[4];
        const double qN = (fn ? P.ibc_u[3] : 0.0) * q.m[3];
        imm = (qE - qW + qN - qS) / q.m[6];
    }
    const double cor = -q.f * avg4(q.v4);                            // x_f_cross_U
    const double ttop = total_tau(P.top, q.top, &P.top.tau_u, q.uc, q.v4);
    const double tbot = total_tau(P.bot, q.bot, &P.bot.tau_u, q.uc, q.v4);
    const bool zero = (mi <= 0) | q.c.inact[2] | q.c.inact[3];     // no mass / peripheral node: cell (i - 1, j) or (i, j) inactive
    F[MQ_CORIOLIS] = (zero | !P.has_cor) ? 0.0 : mi * (-cor);
    F[MQ_TOP] = zero ? 0.0 : (T.raw_stress ? ttop : -(ai * ttop));
    F[MQ_BOTTOM] = zero ? 0.0 : (T.raw_stress ? tbot : ai * tbot);
    F[MQ_INTERNAL] = (zero | (T.no_internal != 0)) ? 0.0 : div + imm;
    F[MQ_FORCING] = (zero | !P.has_forcing) ? 0.0 : mi * q.user;
}
template <bool VISC>
__device__ __forceinline__ void v_terms(const MomTermsDev& T, VPoint& q, int i, int j, double (&F)[MQ_COUNT]) {
    const EvpDev& P = T.P;
    const GridDev& g = P.g;
    resolve_cells<3, 2>(g, i - 1, j - 1, q.c);
    const double mi = (q.hs * P.rho * q.as_ + q.hn * P.rho * q.an) / 2;
    const double ai = (q.as_ + q.an) / 2;
    // cells (i-1..i+1) x (j-1..j): (i, j-1) = 1, (i, j) = 4; corners (i, j) = cells 0, 1, 3, 4; (i + 1, j) = cells 1, 2, 4, 5
    const bool cs = ipcc(g, q.c, 1), cn = ipcc(g, q.c, 4), fw = ipff<3>(g, q.c, 0), fe = ipff<3>(g, q.c, 1);
    double s11s, s11n, s22s, s22n, s12w, s12e;
    if (VISC) {
        s11s = T.nu * (q.u4[1] - q.u4[0]); s11n = T.nu * (q.u4[3] - q.u4[2]);
        s22s = T.nu * (q.vc - q.vs); s22n = T.nu * (q.vn - q.vc);
        s12w = T.nu * (q.vc - q.vw); s12e = T.nu * (q.ve - q.vc);
    } else {
        s11s = q.s11s; s11n = q.s11n; s22s = q.s22s; s22n = q.s22n; s12w = q.s12w; s12e = q.s12e;
    }
    s11s = cs ? 0.0 : s11s; s22s = cs ? 0.0 : s22s;
    s11n = cn ? 0.0 : s11n; s22n = cn ? 0.0 : s22n;
    s12w = fw ? 0.0 : s12w; s12e = fe ? 0.0 : s12e;
    const double div = div2<false>(q.m, s11n + s22n, s11s + s22s, s11n - s22n, s11s - s22s, s12e, s12w);
    double imm = 0.0;
    if (g.has_mask) {
        const double qW = (fw ? -P.ibc_v[0] : 0.0) * q.m[4];
        const double qE = (fe ? P.ibc_v[1] : 0.0) * q.m[3];
        const double qS = (cs ? -P.ibc_v[2] : 0.0) * q.m[2];
        const double qN = (cn ? P.ibc_v[3] : 0.0) * q.m[1];
        imm = (qE - qW + qN - qS) / q.m[6];
    }
    const double cor = q.f * avg4(q.u4);                             // y_f_cross_U
    const double ttop = total_tau(P.top, q.top, &P.top.tau_v, q.vc, q.u4);
    const double tbot = total_tau(P.bot, q.bot, &P.bot.tau_v, q.vc, q.u4);
    const bool zero = (mi <= 0) | q.c.inact[1] | q.c.inact[4];     // cell (i, j - 1) or (i, j) inactive
    F[MQ_CORIOLIS] = (zero | !P.has_cor) ? 0.0 : mi * (-cor);
    F[MQ_TOP] = zero ? 0.0 : (T.raw_stress ? ttop : -(ai * ttop));
    F[MQ_BOTTOM] = zero ? 0.0 : (T.raw_stress ? tbot : ai * tbot);
    F[MQ_INTERNAL] = (zero | (T.no_internal != 0)) ? 0.0 : div + imm;
    F[MQ_FORCING] = (zero | !P.has_forcing) ? 0.0 : mi * q.user;
}

template <bool VISC>
__global__ void __launch_bounds__(256) k_momentum_terms(MomTermsDev T) {
    const EvpDev& P = T.P;
    const GridDev& g = P.g;
    const int i = 1 + (int)(blockIdx.x * 64 + threadIdx.x), j = 1 + (int)(blockIdx.y * 4 + threadIdx.y);
    const int nxu = g.Nx + T.exu, nyv = g.Ny + T.eyv;
    const bool do_u = (i <= nxu) & (j <= g.Ny), do_v = (i <= g.Nx) & (j <= nyv);
    if (!(do_u | do_v)) return;
    // (a component this thread does not own is gathered at the nearest point of its extent and never stored)
    const int iu = min(i, nxu), ju = min(j, g.Ny), iv = min(i, g.Nx), jv = min(j, nyv);
    UPoint qu;
    VPoint qv;
    gather_u<VISC>(P, P.u, P.v, iu, ju, qu);
    gather_v<VISC>(P, P.u, P.v, iv, jv, qv);
    double Fu[MQ_COUNT], Fv[MQ_COUNT];
    u_terms<VISC>(T, qu, iu, ju, Fu);
    v_terms<VISC>(T, qv, iv, jv, Fv);
#pragma unroll
    for (int t = 0; t < MQ_COUNT; ++t) {
        if (T.out[2 * t].p && do_u) T.out[2 * t](i, j) = Fu[t];
        if (T.out[2 * t + 1].p && do_v) T.out[2 * t + 1](i, j) = Fv[t];
    }
}

constexpr int kRows = 64;

__device__ __forceinline__ void block_fold(double (&acc)[MQ_COUNT], int lane, int wave, int tid, double* dst, long stride) {
    __shared__ double sm[4][MQ_COUNT];
#pragma unroll
    for (int q = 0; q < MQ_COUNT; ++q) {
        double x = acc[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off);
        if (lane == 0) sm[wave][q] = x;
    }
    __syncthreads();
    if (tid < MQ_COUNT) {
        double x = sm[0][tid];
        for (int w = 1; w < 4; ++w) x = x + sm[w][tid];
        dst[(long)tid * stride] = x;
    }
}

template <bool VISC>
__global__ void __launch_bounds__(256) k_momentum_power(MomTermsDev T) {
    const EvpDev& P = T.P;
    const GridDev& g = P.g;
    const int i = 1 + (int)blockIdx.x * 64 + (int)threadIdx.x;
    const int ic = min(i, g.Nx);
    double acc[MQ_COUNT];
#pragma unroll
    for (int q = 0; q < MQ_COUNT; ++q) acc[q] = 0.0;
#pragma unroll 1
    for (int r = 0; r < kRows / 4; ++r) {
        const int j = 1 + (int)blockIdx.y * kRows + 4 * r + (int)threadIdx.y;
        const int jc = min(j, g.Ny);
        const bool in = (i <= g.Nx) & (j <= g.Ny);
        UPoint qu;
        VPoint qv;
        gather_u<VISC>(P, P.u, P.v, ic, jc, qu);
        gather_v<VISC>(P, P.u, P.v, ic, jc, qv);
        double Fu[MQ_COUNT], Fv[MQ_COUNT];
        u_terms<VISC>(T, qu, ic, jc, Fu);
        v_terms<VISC>(T, qv, ic, jc, Fv);
#pragma unroll
        for (int q = 0; q < MQ_COUNT; ++q) {
            const double w = (qu.uc * Fu[q]) * qu.m[6] + (qv.vc * Fv[q]) * qv.m[6];      // Az^fc(i, j), Az^cf(i, j)
            acc[q] = acc[q] + (in ? w : 0.0);
        }
    }
    const long rec = (long)blockIdx.y * gridDim.x + blockIdx.x;
    block_fold(acc, (int)threadIdx.x, (int)threadIdx.y, (int)(threadIdx.y * 64 + threadIdx.x), T.part + rec, T.nrec);
}

__global__ void __launch_bounds__(256) k_momentum_power_finish(const double* __restrict__ part, long nrec, double* __restrict__ out) {
    const int t = (int)threadIdx.x;
    double acc[MQ_COUNT];
#pragma unroll
    for (int q = 0; q < MQ_COUNT; ++q) acc[q] = 0.0;
    for (long r = t; r < nrec; r += 256) {
#pragma unroll
        for (int q = 0; q < MQ_COUNT; ++q) acc[q] = acc[q] + part[(long)q * nrec + r];
    }
    block_fold(acc, t & 63, t >> 6, t, out, 1);
}

}  // namespace mt

void launch_momentum_terms(const MomTermsDev& T, bool visc, hipStream_t s) {
    const dim3 b(64, 4), g((unsigned)((T.P.g.Nx + T.exu + 63) / 64), (unsigned)((T.P.g.Ny + T.eyv + 3) / 4), 1);
    if (visc) hipLaunchKernelGGL(mt::k_momentum_terms<true>, g, b, 0, s, T);
    else hipLaunchKernelGGL(mt::k_momentum_terms<false>, g, b, 0, s, T);
}

void launch_momentum_power(const MomTermsDev& T, bool visc, double* out, hipStream_t s) {
    int nbx, nby;
    diag_geometry(T.P.g.Nx, T.P.g.Ny, &nbx, &nby);
    const dim3 b(64, 4), g((unsigned)nbx, (unsigned)nby, 1);
    if (visc) hipLaunchKernelGGL(mt::k_momentum_power<true>, g, b, 0, s, T);
    else hipLaunchKernelGGL(mt::k_momentum_power<false>, g, b, 0, s, T);
    hipLaunchKernelGGL(mt::k_momentum_power_finish, dim3(1), dim3(256), 0, s, T.part, T.nrec, out);
}

}  // namespace csi
