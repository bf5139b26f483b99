// budget.hip -- energy budget integrals of the bound state (include/csi.h: csi_budget_compute).
//
//   k_budget_partial<MK, STRESS, KIN>   one pass over i = 1 .. Nx, j = 1 .. Ny; each block of 64 x 64 cells writes one record of BQ_COUNT sums
//   k_budget_finish                     ONE block folds the records
// The two-launch scheme and the SUMMATION ORDER of the device diagnostics (diagnostics.hip; stated once, in include/csi.h): thread
// (tx, ty) adds the cells of column tx in rows ty, ty + 4, ..., ty + 60 of the block's tile from +0.0, the wave combines over lane offsets
// 32 .. 1 (xor butterfly), the block adds its four waves in wave order, the finishing block's thread t adds records t, t + 256, ... and
// folds the same way.  No atomics, no flags: the launch boundary is the only hand-off.  A lane or row beyond the grid contributes +0.0;
// its loads come from indices clamped into the interior (the stencils then stay inside the elements include/csi.h names).
// One term per cell and sum, formed in the order of test/test_rheology_energy_budget.jl:77-88.  Compiled without contraction.
#include "csi_kernels.h"
#include "derived_dev.h"

namespace csi {
namespace bq {
using namespace dv;

constexpr int kRows = 64;

template <int Q0, int Q1>
__device__ __forceinline__ void block_fold(double (&acc)[BQ_COUNT], int lane, int wave, int tid, double* dst, long stride) {
    __shared__ double sm[4][BQ_COUNT];
#pragma unroll
    for (int q = Q0; q < Q1; ++q) {
        double x = acc[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off);
        if (lane == 0) sm[wave][q] = x;
    }
    __syncthreads();
    const int q = Q0 + tid;
    if (q < Q1) {
        double x = sm[0][q];
        for (int w = 1; w < 4; ++w) x = x + sm[w][q];
        dst[(long)q * stride] = x;
    }
}

template <int MK, bool STRESS, bool KIN>
__global__ void __launch_bounds__(256) k_budget_partial(BudgetDev D) {
    constexpr int Q0 = STRESS ? 0 : BQ_KINETIC, Q1 = KIN ? BQ_COUNT : BQ_KINETIC;
    const GridDev& g = D.g;
    const int i = 1 + (int)blockIdx.x * 64 + (int)threadIdx.x;
    const int ic = min(i, g.Nx);
    const Sigma S{D.s11, D.s22, D.s12};
    double acc[BQ_COUNT];
#pragma unroll
    for (int q = 0; q < BQ_COUNT; ++q) acc[q] = 0.0;
#pragma unroll 1
    for (int r = 0; r < kRows / 4; ++r) {      // (not unrolled: the per-point instantiation's stencil holds some forty metric elements per row)
        const int j = 1 + (int)blockIdx.y * kRows + 4 * r + (int)threadIdx.y;
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
    const long rec = (long)blockIdx.y * gridDim.x + blockIdx.x;
    block_fold<Q0, Q1>(acc, (int)threadIdx.x, (int)threadIdx.y, (int)(threadIdx.y * 64 + threadIdx.x), D.part + rec, D.nrec);
}

template <int Q0, int Q1>
__global__ void __launch_bounds__(256) k_budget_finish(const double* __restrict__ part, long nrec, double* __restrict__ out) {
    const int t = (int)threadIdx.x;
    double acc[BQ_COUNT];
#pragma unroll
    for (int q = 0; q < BQ_COUNT; ++q) acc[q] = 0.0;
    for (long r = t; r < nrec; r += 256) {
#pragma unroll
        for (int q = Q0; q < Q1; ++q) acc[q] = acc[q] + part[(long)q * nrec + r];
    }
    block_fold<Q0, Q1>(acc, t & 63, t >> 6, t, out, 1);
}

template <int MK>
static void launch_mk(const BudgetDev& D, bool stress, bool kin, double* out, dim3 g, dim3 b, hipStream_t s) {
    if (stress && kin) {
        hipLaunchKernelGGL((k_budget_partial<MK, true, true>), g, b, 0, s, D);
        hipLaunchKernelGGL((k_budget_finish<0, BQ_COUNT>), dim3(1), dim3(256), 0, s, D.part, D.nrec, out);
    } else if (stress) {
        hipLaunchKernelGGL((k_budget_partial<MK, true, false>), g, b, 0, s, D);
        hipLaunchKernelGGL((k_budget_finish<0, BQ_KINETIC>), dim3(1), dim3(256), 0, s, D.part, D.nrec, out);
    } else {
        hipLaunchKernelGGL((k_budget_partial<MK, false, true>), g, b, 0, s, D);
        hipLaunchKernelGGL((k_budget_finish<BQ_KINETIC, BQ_COUNT>), dim3(1), dim3(256), 0, s, D.part, D.nrec, out);
    }
}

}  // namespace bq

void launch_budget(const BudgetDev& D, bool stress, bool kin, double* out, hipStream_t s) {
    int nbx, nby;
    diag_geometry(D.g.Nx, D.g.Ny, &nbx, &nby);
    const dim3 b(64, 4), g((unsigned)nbx, (unsigned)nby, 1);
    if (D.g.metric_kind == 0) bq::launch_mk<0>(D, stress, kin, out, g, b, s);
    else if (D.g.metric_kind == 1) bq::launch_mk<1>(D, stress, kin, out, g, b, s);
    else bq::launch_mk<2>(D, stress, kin, out, g, b, s);
}

}  // namespace csi
