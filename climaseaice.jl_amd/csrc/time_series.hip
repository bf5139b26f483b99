// time_series.hip -- forcing time series interpolated at the model clock (include/csi.h csi_time_series_update).
//
//   k_time_series   psi = (n1 == n2) ? psi_1 : psi_2 * n~ + psi_1 * (1 - n~)
//                   (the reference reads a FieldTimeSeries as fts[i, j, 1, Time(clock.time)], e.g. the snowfall of
//                   SeaIceThermodynamics/thermodynamic_time_step.jl:326-329; the formula is RECALLED from the un-vendored
//                   Oceananigans: include/csi.h states it, tests/time_series_ref.py pins it)
// ONE launch for every series-driven slot: the table of descriptors (at most kMaxSeries, nineteen) travels by value as the kernel argument, the grid
// runs over (column block, row block, slot).  Writes the INTERIOR of the bound array only; the halos of the velocity-point slots stay
// update_external_stress' to fill.
//
// A bandwidth kernel: per point two loads and one store, 24 B, two products and one sum.  A thread owns two consecutive points in each
// of kRows rows, four rows apart; the pair starts at an even element of the DESTINATION row counted from a 16-byte boundary, so the
// store is one 16-byte access, and so is each load whose source row has the destination row's alignment (the library's own ring
// slices always have: csi_time_series.hip; a caller's device array has where its row stride and base allow it) -- the first / last
// point of a row that starts / ends odd is a lone 8-byte access.  All 2 * kRows operand pairs are loaded before the first one is
// used.  No LDS, no scratch.  The arithmetic is compiled without contraction (the unit is a STRICT one) and is the same in both
// modes: two products, one sum, in this order.
#include "csi_dev.h"
#include "csi_kernels.h"
#include <cstdint>

namespace csi {

namespace {

constexpr int kRows = 2;                 // rows per thread
constexpr int kBx = 64, kBy = 4;         // threads of a block: 128 columns x (4 * kRows) rows

typedef double pair_t __attribute__((ext_vector_type(2)));      // (a native vector: ONE 16-byte access, which the compiler cannot split)

// elements [e0, e0 + 1] of a row (lo / hi: which of the two exist); one 16-byte load where the address allows it
__device__ __forceinline__ pair_t load_pair(const double* row, int e0, bool lo, bool hi) {
    const double* p = row + e0;
    pair_t v = {0.0, 0.0};
    if (lo & hi & ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) {
        v = *reinterpret_cast<const pair_t*>(p);
    } else {
        if (lo) v.x = p[0];
        if (hi) v.y = p[1];
    }
    return v;
}

}  // namespace

__global__ void __launch_bounds__(kBx * kBy) k_time_series(SeriesTable T) {
    const SeriesDesc& D = T.d[blockIdx.z];
    const int pair = (int)(blockIdx.x * kBx + threadIdx.x);
    const int jb = (int)(blockIdx.y * (kBy * kRows) + threadIdx.y);
    if (2 * pair - 1 >= D.nx || jb >= D.ny) return;
    pair_t a[kRows], b[kRows];
    int e0[kRows];
    bool lo[kRows], hi[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int j = jb + r * kBy;
        const bool row = j < D.ny;
        const long jj = row ? j : 0;
        // the pair's first element: even counted from the 16-byte boundary at or below the destination row's start
        const int head = (int)((reinterpret_cast<uintptr_t>(D.dst + jj * D.ldd) >> 3) & 1);
        e0[r] = 2 * pair - head;
        lo[r] = row & (e0[r] >= 0) & (e0[r] < D.nx);
        hi[r] = row & (e0[r] + 1 < D.nx);
        a[r] = load_pair(D.a + jj * D.lda, e0[r], lo[r], hi[r]);
        b[r] = load_pair(D.b + jj * D.ldb, e0[r], lo[r], hi[r]);
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const long jj = jb + r * kBy;
        pair_t o;
        o.x = D.same ? a[r].x : b[r].x * D.w2 + a[r].x * D.w1;
        o.y = D.same ? a[r].y : b[r].y * D.w2 + a[r].y * D.w1;
        double* p = D.dst + jj * D.ldd + e0[r];
        if (lo[r] & hi[r]) {
            *reinterpret_cast<pair_t*>(p) = o;          // (16-byte aligned by the choice of e0)
        } else {
            if (lo[r]) p[0] = o.x;
            if (hi[r]) p[1] = o.y;
        }
    }
}

void launch_time_series(const SeriesTable& T, hipStream_t s) {
    if (T.n <= 0) return;
    int nx = 0, ny = 0;
    for (int k = 0; k < T.n; ++k) {
        nx = T.d[k].nx > nx ? T.d[k].nx : nx;
        ny = T.d[k].ny > ny ? T.d[k].ny : ny;
    }
    const int pairs = nx / 2 + 1;                        // a row that starts odd has one pair more
    const dim3 b(kBx, kBy);
    const dim3 g((unsigned)((pairs + kBx - 1) / kBx), (unsigned)((ny + kBy * kRows - 1) / (kBy * kRows)), (unsigned)T.n);
    hipLaunchKernelGGL(k_time_series, g, b, 0, s, T);
}

}  // namespace csi
