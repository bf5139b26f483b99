// ordered_reduce.h -- the ONE device-side statement of the ordered reduction that csi_diagnostics_compute, csi_budget_compute and
// csi_momentum_budget_compute share (diagnostics.hip, budget.hip, momentum_terms.hip), and csi_regions_compute with one record per region
// and block (regions.hip).  gfx950 only.
//
// Two launches on one stream: a partial kernel of 64 x 4 threads per block of 64 x 64 cells writes one record per block (plain stores,
// one slot per quantity: slot q of record r at part[q * nrec + r]); ONE block (finish_records) folds the records into the result.  The
// launch boundary is the only hand-off between workgroups -- no atomics, no flags, no workgroup waits for another.  Every combine has
// a fixed place in a fixed tree, so the results are reproducible bit for bit.  THE ORDER (part of the interface: include/csi.h defines
// it for users, tests/diagnostics_ref.py ordered_sum restates it in NumPy):
//   thread (tx, ty) of a block combines the cells of column tx in rows ty, ty + 4, ..., ty + 60 of the block's tile, ascending, from
//   the identity; the wave (one 64-lane row of threads) combines over lane offsets 32, 16, 8, 4, 2, 1 (xor butterfly: both partners
//   form a + b, so every lane ends with the same bits); the block combines its four waves' values in wave order; the finishing
//   block's thread t combines records t, t + 256, ... ascending, from the identity, then the same butterfly and the same wave order.
// Lanes and rows outside the grid contribute the identity: +0.0 to sums, -Inf to maxima, +Inf to minima and 0 to counts.
// The partial kernels keep their own loop bodies (what they load and how far they unroll differs on purpose); the tile walk, the fold
// and the finishing kernel are here.  Units that include this header are compiled without contraction.
#pragma once
#include "csi_dev.h"
#include "csi_kernels.h"
#include <math.h>

namespace csi {
namespace red {

// ---- the block shape: 64 columns x 64 rows, sixteen rows per thread; a function of (Nx, Ny) alone -- the order depends on nothing else
constexpr int kTileCols = 64, kTileRows = 64, kRowsPerThread = kTileRows / 4, kFinishThreads = 256;
inline void diag_geometry(int Nx, int Ny, int* nbx, int* nby) { *nbx = (Nx + kTileCols - 1) / kTileCols; *nby = (Ny + kTileRows - 1) / kTileRows; }
inline dim3 tile_blocks(int Nx, int Ny) {
    int nbx, nby;
    diag_geometry(Nx, Ny, &nbx, &nby);
    return dim3((unsigned)nbx, (unsigned)nby, 1);
}
inline dim3 tile_threads() { return dim3(kTileCols, 4); }
// this thread's column, its r-th row (r < kRowsPerThread) and the block's record
__device__ __forceinline__ int tile_col() { return 1 + (int)blockIdx.x * kTileCols + (int)threadIdx.x; }
__device__ __forceinline__ int tile_row(int r) { return 1 + (int)blockIdx.y * kTileRows + 4 * r + (int)threadIdx.y; }
__device__ __forceinline__ long tile_record() { return (long)blockIdx.y * gridDim.x + blockIdx.x; }

// ---- what a slot holds (K_SUM .. K_CNT: csi_kernels.h).  A kind map is a type with `static constexpr int kind(int q)`; AllSums: every
// slot is a sum, so combine is a + b and the identity +0.0 once the compiler has folded the constant
struct AllSums { __host__ __device__ static constexpr int kind(int) { return K_SUM; } };
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
template <int N, class Kinds> __device__ __forceinline__ void set_identity(double (&acc)[N]) {
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] = identity(Kinds::kind(q));
}

// wave butterfly, then the block's waves in wave order; thread q - Q0 of the block ends with quantity q and stores it.  A partial kernel
// ends with block_fold(acc, threadIdx.x, threadIdx.y, threadIdx.y * kTileCols + threadIdx.x, part + tile_record(), nrec)
template <int N, int Q0, int Q1, class Kinds>
__device__ __forceinline__ void block_fold(double (&acc)[N], int lane, int wave, int tid, double* dst, long stride) {
    __shared__ double sm[4][N];
#pragma unroll
    for (int q = Q0; q < Q1; ++q) {
        double x = acc[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x = combine(Kinds::kind(q), x, __shfl_xor(x, off));
        if (lane == 0) sm[wave][q] = x;
    }
    __syncthreads();
    const int q = Q0 + tid;
    if (q < Q1) {
        const int kind = Kinds::kind(q);
        double x = sm[0][q];
        for (int w = 1; w < 4; ++w) x = combine(kind, x, sm[w][q]);
        dst[(long)q * stride] = x;
    }
}
// the finishing kernel: one block of kFinishThreads per SEGMENT -- block b folds the records at part + b * N * nrec into out + b * N.
// The diagnostics and the budgets launch one block (their one segment: b = 0, the pointers as given); csi_regions_compute one per region
// (regions.hip), each in the order stated above.  UNROLL: the record loop's unroll count (0: the compiler's choice).  The loop is
// written out under both branches: behind a helper function the compiler unrolls it differently (more loads in flight than the
// registers of the 21-slot instantiations hold at their occupancy).  The two loops are ONE statement: an edit to one is an edit to both
template <int N, int Q0, int Q1, class Kinds, int UNROLL>
__global__ void __launch_bounds__(kFinishThreads) finish_records(const double* __restrict__ part, long nrec, double* __restrict__ out) {
    const int t = (int)threadIdx.x;
    part += (long)blockIdx.x * N * nrec;
    out += (long)blockIdx.x * N;
    double acc[N];
    set_identity<N, Kinds>(acc);
    if constexpr (UNROLL > 0) {
#pragma unroll UNROLL
        for (long r = t; r < nrec; r += kFinishThreads) {
#pragma unroll
            for (int q = Q0; q < Q1; ++q) acc[q] = combine(Kinds::kind(q), acc[q], part[(long)q * nrec + r]);
        }
    } else {
        for (long r = t; r < nrec; r += kFinishThreads) {
#pragma unroll
            for (int q = Q0; q < Q1; ++q) acc[q] = combine(Kinds::kind(q), acc[q], part[(long)q * nrec + r]);
        }
    }
    block_fold<N, Q0, Q1, Kinds>(acc, t & 63, t >> 6, t, out, 1);
}
template <int N, int Q0, int Q1, class Kinds, int UNROLL>
inline void launch_finish(const double* part, long nrec, double* out, hipStream_t s, int segments = 1) {
    hipLaunchKernelGGL((finish_records<N, Q0, Q1, Kinds, UNROLL>), dim3((unsigned)segments), dim3(kFinishThreads), 0, s, part, nrec, out);
}

}  // namespace red
}  // namespace csi
