// diagnostics.hip -- scalars computed from the model's fields on the device (include/csi.h: csi_diagnostics_compute).
//
//   k_diag_partial   one pass over the interior i = 1 .. Nx, j = 1 .. Ny: every requested array is read once, each block of 64 x 64
//                    cells writes one partial record (plain stores, one slot per quantity)
//   red::finish_records   ONE block folds the records into the result
// The two-launch scheme, the tile walk, the fold and the SUMMATION ORDER: ordered_reduce.h (defined for users in include/csi.h).  Here:
// what a cell contributes to each of the 21 slots (which slots are sums, maxima, minima and counts: csi_kernels.h DiagKinds).
//
// A bandwidth kernel: 16 B per cell for the velocity group (u, v), 16 or 24 B + the mask byte for the tracer group, plus the metric
// planes on CSI_METRIC_FULL grids.  64-lane rows: consecutive lanes read consecutive elements; a thread walks sixteen rows, four of
// them in flight.  (Sixteen rows per thread, not four: the fold of 21 quantities -- six dependent cross-lane steps each -- is a latency
// chain that a block of 64 x 16 cells could not hide; measured both ways, profiles/r15_diagnostics.md.)
// Every load is unconditional and from an address clamped into the field's interior (the value is discarded by a select where the
// lane is outside the grid); the mask byte likewise (csi_dev.h inactive_cell).  Halo elements are never read.  The two extra loads of
// a Bounded direction's last faces (u[Nx + 1, j], v[i, Ny + 1]) are made by the blocks of the last block column / row only: a
// block-uniform test.  Compiled without contraction; STRICT and FAST run the same code.
#include "csi_dev.h"
#include "csi_kernels.h"
#include "ordered_reduce.h"

namespace csi {
namespace diag {

using namespace red;

using Kinds = DiagKinds;      // csi_kernels.h
__device__ __forceinline__ bool nonfinite(double x) { return !(fabs(x) <= 1.7976931348623157e308); }

template <bool VEL, bool TRC>
__global__ void __launch_bounds__(256) k_diag_partial(DiagDev D) {
    constexpr int Q0 = VEL ? 0 : DQ_VOLUME, Q1 = TRC ? DQ_COUNT : DQ_VOLUME;
    const GridDev& g = D.g;
    const int i = tile_col();
    const int ic = min(i, g.Nx);
    double acc[DQ_COUNT];
    set_identity<DQ_COUNT, Kinds>(acc);
    const bool last_bx = blockIdx.x == gridDim.x - 1, last_by = blockIdx.y == gridDim.y - 1;
#pragma unroll 4
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int j = tile_row(r);
        const int jc = min(j, g.Ny);
        const bool in = (i <= g.Nx) & (j <= g.Ny);
        if (VEL) {
            const double u = D.u.ld_(ic, jc), v = D.v.ld_(ic, jc);
            const double dx = dxm(g, LOC_F, LOC_C, ic, jc), dy = dym(g, LOC_C, LOC_F, ic, jc);
            const double au = fabs(u), av = fabs(v);
            const double inv = (au / dx) + (av / dy);
            acc[DQ_INV_TIMESCALE] = fmax(acc[DQ_INV_TIMESCALE], in ? inv : -INFINITY);
            acc[DQ_MAX_ABS_U] = fmax(acc[DQ_MAX_ABS_U], in ? au : -INFINITY);
            acc[DQ_MAX_ABS_V] = fmax(acc[DQ_MAX_ABS_V], in ? av : -INFINITY);
            long long nfu = in & nonfinite(u), nfv = in & nonfinite(v), nnu = in & (u != u), nnv = in & (v != v);
            if (D.exu && last_bx) {         // the faces i = Nx + 1 of a Bounded x direction: the thread of column Nx reads them
                const bool mine = (i == g.Nx) & (j <= g.Ny);
                const double ue = D.u.ld_(i == g.Nx ? g.Nx + 1 : ic, jc);
                acc[DQ_MAX_ABS_U] = fmax(acc[DQ_MAX_ABS_U], mine ? fabs(ue) : -INFINITY);
                nfu += mine & nonfinite(ue); nnu += mine & (ue != ue);
            }
            if (D.eyv && last_by) {         // the faces j = Ny + 1 of a Bounded y direction: the thread of row Ny reads them
                const bool mine = (j == g.Ny) & (i <= g.Nx);
                const double ve = D.v.ld_(ic, j == g.Ny ? g.Ny + 1 : jc);
                acc[DQ_MAX_ABS_V] = fmax(acc[DQ_MAX_ABS_V], mine ? fabs(ve) : -INFINITY);
                nfv += mine & nonfinite(ve); nnv += mine & (ve != ve);
            }
            acc[DQ_NONFINITE_U] = cnt(__double_as_longlong(acc[DQ_NONFINITE_U]) + nfu);
            acc[DQ_NONFINITE_V] = cnt(__double_as_longlong(acc[DQ_NONFINITE_V]) + nfv);
            acc[DQ_NAN_U] = cnt(__double_as_longlong(acc[DQ_NAN_U]) + nnu);
            acc[DQ_NAN_V] = cnt(__double_as_longlong(acc[DQ_NAN_V]) + nnv);
        }
        if (TRC) {
            const double h = D.h.ld_(ic, jc), a = D.a.ld_(ic, jc);
            const double hs_raw = (D.has_hs ? D.hs : D.h).ld_(ic, jc);      // (no snow layer: h's element, discarded)
            const double hs = D.has_hs ? hs_raw : 0.0;
            const double az = azm(g, LOC_C, LOC_C, ic, jc);
            const bool act = in & !inactive_cell(g, ic, jc);
            acc[DQ_VOLUME] = acc[DQ_VOLUME] + (act ? (h * a) * az : 0.0);
            acc[DQ_AREA] = acc[DQ_AREA] + (act ? a * az : 0.0);
            acc[DQ_EXTENT] = acc[DQ_EXTENT] + ((act & (a >= D.threshold)) ? az : 0.0);
            acc[DQ_SNOW_VOLUME] = acc[DQ_SNOW_VOLUME] + (act ? (hs * a) * az : 0.0);
            acc[DQ_ACTIVE_AREA] = acc[DQ_ACTIVE_AREA] + (act ? az : 0.0);
            acc[DQ_MIN_H] = fmin(acc[DQ_MIN_H], act ? h : INFINITY);
            acc[DQ_MAX_H] = fmax(acc[DQ_MAX_H], act ? h : -INFINITY);
            acc[DQ_MIN_AICE] = fmin(acc[DQ_MIN_AICE], act ? a : INFINITY);
            acc[DQ_MAX_AICE] = fmax(acc[DQ_MAX_AICE], act ? a : -INFINITY);
            acc[DQ_MAX_HS] = fmax(acc[DQ_MAX_HS], act ? hs : -INFINITY);
            acc[DQ_NONFINITE_H] = cnt(__double_as_longlong(acc[DQ_NONFINITE_H]) + (long long)(in & nonfinite(h)));
            acc[DQ_NONFINITE_AICE] = cnt(__double_as_longlong(acc[DQ_NONFINITE_AICE]) + (long long)(in & nonfinite(a)));
            acc[DQ_NONFINITE_HS] = cnt(__double_as_longlong(acc[DQ_NONFINITE_HS]) + (long long)(in & nonfinite(hs)));
            acc[DQ_ACTIVE_CELLS] = cnt(__double_as_longlong(acc[DQ_ACTIVE_CELLS]) + (long long)act);
        }
    }
    const long rec = tile_record();
    block_fold<DQ_COUNT, Q0, Q1, Kinds>(acc, (int)threadIdx.x, (int)threadIdx.y, (int)(threadIdx.y * kTileCols + threadIdx.x), D.part + rec, D.nrec);
}

template <int Q0, int Q1> static void finish(const DiagDev& D, double* out, hipStream_t s) { launch_finish<DQ_COUNT, Q0, Q1, Kinds, 2>(D.part, D.nrec, out, s); }

}  // namespace diag

void launch_diagnostics(const DiagDev& D, bool vel, bool trc, double* out, hipStream_t s) {
    const dim3 b = red::tile_threads(), g = red::tile_blocks(D.g.Nx, D.g.Ny);
    if (vel && trc) {
        hipLaunchKernelGGL((diag::k_diag_partial<true, true>), g, b, 0, s, D);
        diag::finish<0, DQ_COUNT>(D, out, s);
    } else if (vel) {
        hipLaunchKernelGGL((diag::k_diag_partial<true, false>), g, b, 0, s, D);
        diag::finish<0, DQ_VOLUME>(D, out, s);
    } else {
        hipLaunchKernelGGL((diag::k_diag_partial<false, true>), g, b, 0, s, D);
        diag::finish<DQ_VOLUME, DQ_COUNT>(D, out, s);
    }
}

}  // namespace csi
