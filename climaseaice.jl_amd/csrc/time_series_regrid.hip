// time_series_regrid.hip -- forcing time series given on a rectilinear source grid of their own, regridded at the model clock
// (include/csi.h csi_time_series_set_regridded / csi_time_series_update; the definition of every line below is there).
//
//   k_time_series_regrid   c_k = same_t ? a_k : b_k * w2 + a_k * w1      (the four corners, the time formula of k_time_series)
//                          lo  = c10 * wx + c00 * (1 - wx),  hi = c11 * wx + c01 * (1 - wx),  val = hi * wy + lo * (1 - wy)
//                          a component of a vector pair:  x = val_E * cos + val_N * sin   /   y = val_N * cos - val_E * sin
// ONE launch for every regridded slot: the table of descriptors travels by value as the kernel argument, the grid runs over (column
// block, row block, slot).  Writes the INTERIOR of the bound array only, like k_time_series, whose design this follows: a thread owns
// two consecutive points in each of kRows rows, four rows apart; the pair starts at an even element of the DESTINATION row counted
// from a 16-byte boundary, so the store is one 16-byte access -- and so is every load of the map, whose rows the library lays out with
// the destination row's alignment (csi_kernels.h RegridDesc: pair p of a row sits at entries 2p, 2p + 1 of every plane; padding
// entries are zero, so a point that does not exist gathers source element (0, 0) and is never stored).  Per thread: first every map
// entry (3 or 5 16-byte loads per row), then every gather (8 per scalar point, 16 per point of a pair; 8-byte loads from a source
// slice that is small and shared by all workgroups), all issued before the first one is used.  No LDS, no scratch, no atomics.
// Compulsory HBM traffic per point: the map (24 B, with rotation 40 B) plus the store (8 B).  Compiled without contraction; the
// arithmetic is the same in both modes.
#include "csi_dev.h"
#include "csi_kernels.h"
#include <cstdint>

namespace csi {

namespace {

constexpr int kRows = 2;                 // rows per thread
constexpr int kBx = 64, kBy = 4;         // threads of a block: 128 columns x (4 * kRows) rows

typedef double pair_t __attribute__((ext_vector_type(2)));
typedef unsigned long long upair_t __attribute__((ext_vector_type(2)));

// the four gather offsets (doubles) of a point from its packed uint16 indices {i0, i1, j0, j1}
struct Corners { unsigned o00, o10, o01, o11; };
__device__ __forceinline__ Corners corners(unsigned long long idx, unsigned ld) {
    const unsigned i0 = (unsigned)(idx & 0xffffu), i1 = (unsigned)((idx >> 16) & 0xffffu);
    const unsigned r0 = (unsigned)((idx >> 32) & 0xffffu) * ld, r1 = (unsigned)(idx >> 48) * ld;
    return Corners{r0 + i0, r0 + i1, r1 + i0, r1 + i1};
}

struct Quad { double c00, c10, c01, c11; };
__device__ __forceinline__ Quad gather(const double* s, const Corners& o) { return Quad{s[o.o00], s[o.o10], s[o.o01], s[o.o11]}; }

// time, then x, then y: two products and one sum per line
__device__ __forceinline__ double blend(const Quad& a, const Quad& b, int same, double w1, double w2, double wx, double wy) {
    const double c00 = same ? a.c00 : b.c00 * w2 + a.c00 * w1;
    const double c10 = same ? a.c10 : b.c10 * w2 + a.c10 * w1;
    const double c01 = same ? a.c01 : b.c01 * w2 + a.c01 * w1;
    const double c11 = same ? a.c11 : b.c11 * w2 + a.c11 * w1;
    const double ux = 1.0 - wx, uy = 1.0 - wy;
    const double lo = c10 * wx + c00 * ux;
    const double hi = c11 * wx + c01 * ux;
    return hi * wy + lo * uy;
}

template <bool kPair>
__device__ __forceinline__ void regrid_rows(const RegridDesc& D) {
    constexpr int kParts = kPair ? 2 : 1;
    const int pair = (int)(blockIdx.x * kBx + threadIdx.x);
    const int jb = (int)(blockIdx.y * (kBy * kRows) + threadIdx.y);
    if (2 * pair - 1 >= D.nx || jb >= D.ny) return;
    upair_t idx[kRows];
    pair_t wx[kRows], wy[kRows], cs[kRows], sn[kRows];
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
        const unsigned long long* m = D.map + jj * D.mld + 2 * pair;      // (16-byte aligned: mld, plane even, the base aligned)
        idx[r] = *reinterpret_cast<const upair_t*>(m);
        wx[r] = *reinterpret_cast<const pair_t*>(m + D.plane);
        wy[r] = *reinterpret_cast<const pair_t*>(m + 2 * D.plane);
        if (kPair) {
            cs[r] = *reinterpret_cast<const pair_t*>(m + 3 * D.plane);
            sn[r] = *reinterpret_cast<const pair_t*>(m + 4 * D.plane);
        }
    }
    Quad a[kRows][2][kParts], b[kRows][2][kParts];
#pragma unroll
    for (int r = 0; r < kRows; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int s = 0; s < kParts; ++s) {
                const Corners o = corners(q ? idx[r].y : idx[r].x, (unsigned)D.lds[s]);
                a[r][q][s] = gather(D.a[s], o);
                b[r][q][s] = gather(D.b[s], o);
            }
    __builtin_amdgcn_sched_barrier(0);       // (no blend moves up between the gathers: all of them are in flight before the first is used)
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const long jj = jb + r * kBy;
        double v[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const double x = q ? wx[r].y : wx[r].x, y = q ? wy[r].y : wy[r].x;
            const double e = blend(a[r][q][0], b[r][q][0], D.same[0], D.w1[0], D.w2[0], x, y);
            if (kPair) {
                const double n = blend(a[r][q][kParts - 1], b[r][q][kParts - 1], D.same[1], D.w1[1], D.w2[1], x, y);
                const double c = q ? cs[r].y : cs[r].x, s = q ? sn[r].y : sn[r].x;
                v[q] = D.component ? n * c - e * s : e * c + n * s;
            } else {
                v[q] = e;
            }
        }
        double* p = D.dst + jj * D.ldd + e0[r];
        if (lo[r] & hi[r]) {
            pair_t o = {v[0], v[1]};
            *reinterpret_cast<pair_t*>(p) = o;          // (16-byte aligned by the choice of e0)
        } else {
            if (lo[r]) p[0] = v[0];
            if (hi[r]) p[1] = v[1];
        }
    }
}

}  // namespace

__global__ void __launch_bounds__(kBx * kBy) k_time_series_regrid(RegridTable T) {
    const RegridDesc& D = T.d[blockIdx.z];
    if (D.pair) regrid_rows<true>(D);
    else regrid_rows<false>(D);
}

void launch_time_series_regrid(const RegridTable& T, hipStream_t s) {
    if (T.n <= 0) return;
    int nx = 0, ny = 0;
    for (int k = 0; k < T.n; ++k) {
        nx = T.d[k].nx > nx ? T.d[k].nx : nx;
        ny = T.d[k].ny > ny ? T.d[k].ny : ny;
    }
    const int pairs = nx / 2 + 1;                        // a row that starts odd has one pair more
    const dim3 b(kBx, kBy);
    const dim3 g((unsigned)((pairs + kBx - 1) / kBx), (unsigned)((ny + kBy * kRows - 1) / (kBy * kRows)), (unsigned)T.n);
    hipLaunchKernelGGL(k_time_series_regrid, g, b, 0, s, T);
}

}  // namespace csi
