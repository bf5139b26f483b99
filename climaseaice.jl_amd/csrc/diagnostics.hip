// diagnostics.hip -- scalars computed from the model's fields on the device (include/csi.h: csi_diagnostics_compute).
//
//   k_diag_partial   one pass over the interior i = 1 .. Nx, j = 1 .. Ny: every requested array is read once, each block of 64 x 64
//                    cells writes one partial record (plain stores, one slot per quantity)
//   k_diag_finish    ONE block folds the records into the result
// Two launches on one stream: the launch boundary is the only hand-off between workgroups -- no atomics, no flags, no workgroup
// waits for another.  Every combine has a fixed place in a fixed tree, so the sums are reproducible bit for bit; the order is part of
// the interface and is stated in include/csi.h (tests/diagnostics_ref.py restates it in NumPy):
//   thread (tx, ty) of a block adds the cells of column tx in rows ty, ty + 4, ..., ty + 60 of the block's tile, ascending, from +0.0;
//   the wave (one 64-lane row of threads) combines over lane offsets 32, 16, 8, 4, 2, 1 (xor butterfly: a + b in both partners, so
//   every lane ends with the same bits); the block adds its four waves' values in wave order; the finishing block's thread t adds
//   records t, t + 256, ... ascending, from +0.0, then the same butterfly and the same wave order.
// Lanes and rows outside the grid contribute +0.0 to sums, -Inf to maxima, +Inf to minima and 0 to counts.
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
#include <math.h>

namespace csi {
namespace diag {

constexpr int kDiagRows = 64;      // rows of a block's tile (64 columns wide): sixteen per thread
enum : int { K_SUM = 0, K_MAX = 1, K_MIN = 2, K_CNT = 3 };

__host__ __device__ constexpr int kind_of(int q) {
    return (q == DQ_INV_TIMESCALE || q == DQ_MAX_ABS_U || q == DQ_MAX_ABS_V || q == DQ_MAX_H || q == DQ_MAX_AICE || q == DQ_MAX_HS) ? K_MAX
         : (q == DQ_MIN_H || q == DQ_MIN_AICE) ? K_MIN
         : (q >= DQ_VOLUME && q <= DQ_ACTIVE_AREA) ? K_SUM
         : K_CNT;
}
// counts travel through the double slots as bit patterns (moves only, never arithmetic)
__device__ __forceinline__ double cnt(long long n) { return __longlong_as_double(n); }
__device__ __forceinline__ double combine(int kind, double a, double b) {
    if (kind == K_SUM) return a + b;
    if (kind == K_MAX) return fmax(a, b);
    if (kind == K_MIN) return fmin(a, b);
    return cnt(__double_as_longlong(a) + __double_as_longlong(b));
}
__device__ __forceinline__ double identity(int kind) {
    return kind == K_SUM ? 0.0 : kind == K_MAX ? -INFINITY : kind == K_MIN ? INFINITY : cnt(0);
}
__device__ __forceinline__ bool nonfinite(double x) { return !(fabs(x) <= 1.7976931348623157e308); }

// wave butterfly, then the block's waves in wave order; thread q - Q0 of the block ends with quantity q and stores it
template <int Q0, int Q1>
__device__ __forceinline__ void block_fold(double (&acc)[DQ_COUNT], int lane, int wave, int tid, double* dst, long stride) {
    __shared__ double sm[4][DQ_COUNT];
#pragma unroll
    for (int q = Q0; q < Q1; ++q) {
        double x = acc[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x = combine(kind_of(q), x, __shfl_xor(x, off));
        if (lane == 0) sm[wave][q] = x;
    }
    __syncthreads();
    const int q = Q0 + tid;
    if (q < Q1) {
        const int kind = kind_of(q);
        double x = sm[0][q];
        for (int w = 1; w < 4; ++w) x = combine(kind, x, sm[w][q]);
        dst[(long)q * stride] = x;
    }
}

template <bool VEL, bool TRC>
__global__ void __launch_bounds__(256) k_diag_partial(DiagDev D) {
    constexpr int Q0 = VEL ? 0 : DQ_VOLUME, Q1 = TRC ? DQ_COUNT : DQ_VOLUME;
    const GridDev& g = D.g;
    const int i = 1 + (int)blockIdx.x * 64 + (int)threadIdx.x;
    const int ic = min(i, g.Nx);
    double acc[DQ_COUNT];
#pragma unroll
    for (int q = 0; q < DQ_COUNT; ++q) acc[q] = identity(kind_of(q));
    const bool last_bx = blockIdx.x == gridDim.x - 1, last_by = blockIdx.y == gridDim.y - 1;
#pragma unroll 4
    for (int r = 0; r < kDiagRows / 4; ++r) {
        const int j = 1 + (int)blockIdx.y * kDiagRows + 4 * r + (int)threadIdx.y;
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
    const long rec = (long)blockIdx.y * gridDim.x + blockIdx.x;
    block_fold<Q0, Q1>(acc, (int)threadIdx.x, (int)threadIdx.y, (int)(threadIdx.y * 64 + threadIdx.x), D.part + rec, D.nrec);
}

template <int Q0, int Q1>
__global__ void __launch_bounds__(256) k_diag_finish(const double* __restrict__ part, long nrec, double* __restrict__ out) {
    const int t = (int)threadIdx.x;
    double acc[DQ_COUNT];
#pragma unroll
    for (int q = 0; q < DQ_COUNT; ++q) acc[q] = identity(kind_of(q));
#pragma unroll 2
    for (long r = t; r < nrec; r += 256) {
#pragma unroll
        for (int q = Q0; q < Q1; ++q) acc[q] = combine(kind_of(q), acc[q], part[(long)q * nrec + r]);
    }
    block_fold<Q0, Q1>(acc, t & 63, t >> 6, t, out, 1);
}

}  // namespace diag

void diag_geometry(int Nx, int Ny, int* nbx, int* nby) { *nbx = (Nx + 63) / 64; *nby = (Ny + diag::kDiagRows - 1) / diag::kDiagRows; }

void launch_diagnostics(const DiagDev& D, bool vel, bool trc, double* out, hipStream_t s) {
    int nbx, nby;
    diag_geometry(D.g.Nx, D.g.Ny, &nbx, &nby);
    const dim3 b(64, 4), g((unsigned)nbx, (unsigned)nby, 1);
    if (vel && trc) {
        hipLaunchKernelGGL((diag::k_diag_partial<true, true>), g, b, 0, s, D);
        hipLaunchKernelGGL((diag::k_diag_finish<0, DQ_COUNT>), dim3(1), dim3(256), 0, s, D.part, D.nrec, out);
    } else if (vel) {
        hipLaunchKernelGGL((diag::k_diag_partial<true, false>), g, b, 0, s, D);
        hipLaunchKernelGGL((diag::k_diag_finish<0, DQ_VOLUME>), dim3(1), dim3(256), 0, s, D.part, D.nrec, out);
    } else {
        hipLaunchKernelGGL((diag::k_diag_partial<false, true>), g, b, 0, s, D);
        hipLaunchKernelGGL((diag::k_diag_finish<DQ_VOLUME, DQ_COUNT>), dim3(1), dim3(256), 0, s, D.part, D.nrec, out);
    }
}

}  // namespace csi
