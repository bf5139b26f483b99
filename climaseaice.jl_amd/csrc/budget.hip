// budget.hip -- energy budget integrals of the bound state (include/csi.h: csi_budget_compute).
//
//   k_budget_partial<MK, STRESS, KIN>   one pass over i = 1 .. Nx, j = 1 .. Ny; each block of 64 x 64 cells writes one record of BQ_COUNT sums
//   red::finish_records                 ONE block folds the records
// The two-launch scheme, the tile walk, the fold and the SUMMATION ORDER: ordered_reduce.h (every slot a sum).  A lane or row beyond the
// grid contributes +0.0; its loads come from indices clamped into the interior (the stencils then stay inside the elements
// include/csi.h names).  One term per cell and sum, formed in the order of test/test_rheology_energy_budget.jl:77-88 from the strict
// operators of derived_dev.h.  Compiled without contraction.
#include "csi_kernels.h"
#include "derived_dev.h"
#include "ordered_reduce.h"

namespace csi {
namespace bq {
using namespace dv;

using namespace red;

template <int MK, bool STRESS, bool KIN>
__global__ void __launch_bounds__(256) k_budget_partial(BudgetDev D) {
    constexpr int Q0 = STRESS ? 0 : BQ_KINETIC, Q1 = KIN ? BQ_COUNT : BQ_KINETIC;
    const GridDev& g = D.g;
    const int i = tile_col();
    const int ic = min(i, g.Nx);
    const Sigma S{D.s11, D.s22, D.s12};
    double acc[BQ_COUNT];
    set_identity<BQ_COUNT, AllSums>(acc);
#pragma unroll 1
    for (int r = 0; r < kRowsPerThread; ++r) {      // (not unrolled: the per-point instantiation's stencil holds some forty metric elements per row)
        const int j = tile_row(r);
        const int jc = min(j, g.Ny);
        const bool in = (i <= g.Nx) & (j <= g.Ny);
        const double u = D.u.ld_(ic, jc), v = D.v.ld_(ic, jc);
        const double azfc = az_<MK>(g, LOC_F, LOC_C, ic, jc), azcf = az_<MK>(g, LOC_C, LOC_F, ic, jc);
        if (STRESS) {
            const double d1 = div_sigma_1<MK>(g, S, ic, jc), d2 = div_sigma_2<MK>(g, S, ic, jc);
            const double w = (u * d1) * azfc + (v * d2) * azcf;
            const double e11 = e_xx<MK>(g, D.u, D.v, ic, jc), e22 = e_yy<MK>(g, D.u, D.v, ic, jc), e12 = e_xy<MK>(g, D.u, D.v, ic, jc);
            const double azcc = az_<MK>(g, LOC_C, LOC_C, ic, jc), azff = az_<MK>(g, LOC_F, LOC_F, ic, jc);
            const double p = ((D.s11.ld_(ic, jc) * e11) * azcc + (D.s22.ld_(ic, jc) * e22) * azcc) + ((2 * D.s12.ld_(ic, jc)) * e12) * azff;
            acc[BQ_WORK] = acc[BQ_WORK] + (in ? w : 0.0);
            acc[BQ_POWER] = acc[BQ_POWER] + (in ? p : 0.0);
        }
        if (KIN) {
            const double m = D.h.ld_(ic, jc) * D.rho * D.a.ld_(ic, jc);
            const double mw = D.h.ld_(ic - 1, jc) * D.rho * D.a.ld_(ic - 1, jc), ms = D.h.ld_(ic, jc - 1) * D.rho * D.a.ld_(ic, jc - 1);
            const double mu = (mw + m) / 2, mv = (ms + m) / 2;
            const double k = ((0.5 * mu) * (u * u)) * azfc + ((0.5 * mv) * (v * v)) * azcf;
            acc[BQ_KINETIC] = acc[BQ_KINETIC] + (in ? k : 0.0);
        }
    }
    const long rec = tile_record();
    block_fold<BQ_COUNT, Q0, Q1, AllSums>(acc, (int)threadIdx.x, (int)threadIdx.y, (int)(threadIdx.y * kTileCols + threadIdx.x), D.part + rec, D.nrec);
}

template <int Q0, int Q1> static void finish(const BudgetDev& D, double* out, hipStream_t s) { launch_finish<BQ_COUNT, Q0, Q1, AllSums, 0>(D.part, D.nrec, out, s); }

template <int MK>
static void launch_mk(const BudgetDev& D, bool stress, bool kin, double* out, dim3 g, dim3 b, hipStream_t s) {
    if (stress && kin) {
        hipLaunchKernelGGL((k_budget_partial<MK, true, true>), g, b, 0, s, D);
        finish<0, BQ_COUNT>(D, out, s);
    } else if (stress) {
        hipLaunchKernelGGL((k_budget_partial<MK, true, false>), g, b, 0, s, D);
        finish<0, BQ_KINETIC>(D, out, s);
    } else {
        hipLaunchKernelGGL((k_budget_partial<MK, false, true>), g, b, 0, s, D);
        finish<BQ_KINETIC, BQ_COUNT>(D, out, s);
    }
}

}  // namespace bq

void launch_budget(const BudgetDev& D, bool stress, bool kin, double* out, hipStream_t s) {
    const dim3 b = red::tile_threads(), g = red::tile_blocks(D.g.Nx, D.g.Ny);
    if (D.g.metric_kind == 0) bq::launch_mk<0>(D, stress, kin, out, g, b, s);
    else if (D.g.metric_kind == 1) bq::launch_mk<1>(D, stress, kin, out, g, b, s);
    else bq::launch_mk<2>(D, stress, kin, out, g, b, s);
}

}  // namespace csi
