// momentum_terms.hip -- the terms of the velocity tendencies kept apart, and their power (include/csi.h: csi_momentum_terms_compute,
// csi_momentum_budget_compute).  gfx950 only.
//
//   k_momentum_terms<VISC>   one thread per index (i, j): the u point and the v point there; blocks of 64 x 4 threads, consecutive lanes
//                            on consecutive columns; the grid rounds up over i = 1 .. Nx + exu, j = 1 .. Ny + eyv, so the last face
//                            column / row of a Bounded side is covered; a thread beyond a field's own extent stores nothing for that
//                            component (its loads come from indices clamped into the extent)
//   k_momentum_power<VISC>   one pass over i = 1 .. Nx, j = 1 .. Ny; each block of 64 x 64 cells writes one record of MQ_COUNT sums
//   red::finish_records      ONE block folds the records
// The arithmetic is momentum_dev.h's: gather_u / gather_v issue every load of a point before the first value is used, u_front / v_front
// (strict order) give the mass, the concentration, the stress divergence and the immersed flux term exactly as u_tendency / v_tendency
// (momentum_tendencies_kernel_functions.jl:11-74) form them, and explicit_tau / drag_norm the stresses those add up and throw away.  Here the pieces are kept, each scaled
// to a force per unit area as include/csi.h states.  The stores are the last statements; output arrays never alias inputs.
// ONE code path for STRICT and FAST: compiled without contraction, IEEE division and square root.  No atomics, no flags; the field
// kernel uses no LDS.  The power sums follow the two-launch scheme, the tile walk, the fold and the SUMMATION ORDER of ordered_reduce.h
// (every slot a sum).  A lane or row beyond the grid contributes +0.0; its loads come from indices clamped into the interior.
#include "csi_kernels.h"
#include "momentum_dev.h"
#include "ordered_reduce.h"

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
    const Front fr = u_front<false, VISC>(P, T.nu, q, i, j);
    const double mi = fr.mi, ai = fr.ai, div = fr.div, imm = fr.imm;
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
    const Front fr = v_front<false, VISC>(P, T.nu, q, i, j);
    const double mi = fr.mi, ai = fr.ai, div = fr.div, imm = fr.imm;
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

template <bool VISC>
__global__ void __launch_bounds__(256) k_momentum_power(MomTermsDev T) {
    const EvpDev& P = T.P;
    const GridDev& g = P.g;
    const int i = red::tile_col();
    const int ic = min(i, g.Nx);
    double acc[MQ_COUNT];
    red::set_identity<MQ_COUNT, red::AllSums>(acc);
#pragma unroll 1
    for (int r = 0; r < red::kRowsPerThread; ++r) {
        const int j = red::tile_row(r);
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
    const long rec = red::tile_record();
    red::block_fold<MQ_COUNT, 0, MQ_COUNT, red::AllSums>(acc, (int)threadIdx.x, (int)threadIdx.y, (int)(threadIdx.y * red::kTileCols + threadIdx.x), T.part + rec, T.nrec);
}

}  // namespace mt

void launch_momentum_terms(const MomTermsDev& T, bool visc, hipStream_t s) {
    const dim3 b(64, 4), g((unsigned)((T.P.g.Nx + T.exu + 63) / 64), (unsigned)((T.P.g.Ny + T.eyv + 3) / 4), 1);
    if (visc) hipLaunchKernelGGL(mt::k_momentum_terms<true>, g, b, 0, s, T);
    else hipLaunchKernelGGL(mt::k_momentum_terms<false>, g, b, 0, s, T);
}

void launch_momentum_power(const MomTermsDev& T, bool visc, double* out, hipStream_t s) {
    const dim3 b = red::tile_threads(), g = red::tile_blocks(T.P.g.Nx, T.P.g.Ny);
    if (visc) hipLaunchKernelGGL(mt::k_momentum_power<true>, g, b, 0, s, T);
    else hipLaunchKernelGGL(mt::k_momentum_power<false>, g, b, 0, s, T);
    red::launch_finish<MQ_COUNT, 0, MQ_COUNT, red::AllSums, 0>(T.part, T.nrec, out, s);
}

}  // namespace csi
