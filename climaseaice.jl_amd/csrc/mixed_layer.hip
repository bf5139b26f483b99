// mixed_layer.hip -- the slab-ocean mixed layer under the ice (include/csi.h csi_mixed_layer_set): frazil growth and basal melt.
//
//   k_mixed_layer   the fixed form of the closure of examples/freezing_of_a_lake.jl:91-120, as data; per interior cell
//                       C   = (rho * c) * depth                                  (formed once, on the host)
//                       Qs  = Fo + (K * (To - Ta))                               absent terms are not added
//                       Qow = Qs * (1 - a)
//                       dT  = To - Tf                                            Tf = liq_T0 - liq_slope * Sb
//                       Qio = dT > 0 ? min(((gamma * (rho * c)) * dT) * a, (C * dT) / dt) : 0
//                       T1  = To + (dt * ((Qd - Qow) - Qio)) / C
//                       Qfr = T1 < Tf ? (C * (T1 - Tf)) / dt : 0
//                       To' = T1 < Tf ? Tf : T1
//                       Qb  = Qio + Qfr
// ONE point-wise launch: reads To (or its Psi^- copy), aice and the arrays the configuration has, writes To', Qb into the interior of
// the bottom heat-flux array and, where bound, Qow.  Every interior cell is computed, land included, as the thermodynamic kernels do;
// no halo element is read or written.  Compiled with -ffp-contract=off, in exactly this order, STRICT and FAST alike.
//
// A bandwidth kernel, laid out like k_time_series: a thread owns two consecutive points in each of kRows rows, four rows apart; the
// pair starts at an even element of the To' row counted from a 16-byte boundary, so every access whose row has that row's alignment
// is one 16-byte access (arrays of one parent shape and 16-byte-aligned bases always have) and the first / last point of a row that
// starts / ends odd is a lone 8-byte access.  Every load of a thread is issued before the first use; the template flags select which
// loads exist, so a configuration pays only for the arrays it reads.  No LDS, no scratch.
#include <utility>

#include "csi_dev.h"
#include "csi_kernels.h"
#include "thermo_dev.h"
#include <cstdint>

namespace csi {

namespace {

constexpr int kRows = 2;                 // rows per thread
constexpr int kBx = 64, kBy = 4;         // threads of a block: 128 columns x (4 * kRows) rows

typedef double pair_t __attribute__((ext_vector_type(2)));      // (a native vector: ONE 16-byte access, which the compiler cannot split)

// interior elements [e0, e0 + 1] (0-based) of row j of a field (lo / hi: which of the two exist); one 16-byte load where the address allows
__device__ __forceinline__ pair_t load_pair(const FRef& f, long j, int e0, bool lo, bool hi) {
    const double* p = f.p + 1 + j * f.ld + e0;
    pair_t v = {0.0, 0.0};
    if (lo & hi & ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) {
        v = *reinterpret_cast<const pair_t*>(p);
    } else {
        if (lo) v.x = p[0];
        if (hi) v.y = p[1];
    }
    return v;
}

__device__ __forceinline__ void store_pair(const FRef& f, long j, int e0, bool lo, bool hi, pair_t v) {
    double* p = f.p + 1 + j * f.ld + e0;
    if (lo & hi & ((reinterpret_cast<uintptr_t>(p) & 15) == 0)) {
        *reinterpret_cast<pair_t*>(p) = v;
    } else {
        if (lo) p[0] = v.x;
        if (hi) p[1] = v.y;
    }
}

struct CellOut { double to, qb, qow; };

// one cell, statement for statement as the header defines it
template <bool FS, bool FB>
__device__ __forceinline__ CellOut cell(const MixedLayerDev& M, double To, double a, double fo, double K, double Ta, double Qd, double Sb) {
    const double Tf = M.liq_T0 - M.liq_slope * Sb;
    const bool surface = FS || M.has_surface, bulk = FB || M.has_bulk;
    double Qs = 0.0;
    if (bulk) {
        const double qk = K * (To - Ta);
        Qs = surface ? fo + qk : qk;
    } else if (surface) {
        Qs = fo;
    }
    const double Qow = Qs * (1 - a);
    const double dT = To - Tf;
    const double Qio = (dT > 0) ? jmin((M.grc * dT) * a, (M.C * dT) / M.dt) : 0.0;
    const double T1 = To + (M.dt * ((Qd - Qow) - Qio)) / M.C;
    const bool frazil = T1 < Tf;
    const double Qfr = frazil ? (M.C * (T1 - Tf)) / M.dt : 0.0;
    return CellOut{frazil ? Tf : T1, Qio + Qfr, Qow};
}

}  // namespace

// FS / FB / FD / SB: the surface flux Fo / the bulk pair K, Ta (both or neither) / the deep flux Qd / the bottom salinity is read per cell
template <bool FS, bool FB, bool FD, bool SB>
__global__ void __launch_bounds__(kBx * kBy) k_mixed_layer(MixedLayerDev M, MixedLayerFields F) {
    const int pair = (int)(blockIdx.x * kBx + threadIdx.x);
    const int jb = (int)(blockIdx.y * (kBy * kRows) + threadIdx.y);
    if (2 * pair - 1 >= M.nx || jb >= M.ny) return;
    pair_t to[kRows], a[kRows], fo[kRows], k[kRows], ta[kRows], qd[kRows], sb[kRows];
    int e0[kRows];
    bool lo[kRows], hi[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int j0 = jb + r * kBy;
        const bool row = j0 < M.ny;
        const long j = row ? j0 + 1 : 1;         // the reference's 1-based row
        // the pair's first element: even counted from the 16-byte boundary at or below the start of To's interior row
        const int head = (int)((reinterpret_cast<uintptr_t>(F.to_out.p + 1 + j * F.to_out.ld) >> 3) & 1);
        e0[r] = 2 * pair - head;
        lo[r] = row & (e0[r] >= 0) & (e0[r] < M.nx);
        hi[r] = row & (e0[r] + 1 < M.nx);
        to[r] = load_pair(F.to_in, j, e0[r], lo[r], hi[r]);
        a[r] = load_pair(F.a, j, e0[r], lo[r], hi[r]);
        if (FS) fo[r] = load_pair(F.fo, j, e0[r], lo[r], hi[r]);
        if (FB) {
            k[r] = load_pair(F.k, j, e0[r], lo[r], hi[r]);
            ta[r] = load_pair(F.ta, j, e0[r], lo[r], hi[r]);
        }
        if (FD) qd[r] = load_pair(F.qd, j, e0[r], lo[r], hi[r]);
        if (SB) sb[r] = load_pair(F.sb, j, e0[r], lo[r], hi[r]);
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const long j = jb + r * kBy + 1;
        const CellOut x = cell<FS, FB>(M, to[r].x, a[r].x, FS ? fo[r].x : M.Fo, FB ? k[r].x : M.K, FB ? ta[r].x : M.Ta, FD ? qd[r].x : M.Qd,
                                       SB ? sb[r].x : M.S);
        const CellOut y = cell<FS, FB>(M, to[r].y, a[r].y, FS ? fo[r].y : M.Fo, FB ? k[r].y : M.K, FB ? ta[r].y : M.Ta,
                                       FD ? qd[r].y : M.Qd, SB ? sb[r].y : M.S);
        store_pair(F.to_out, j, e0[r], lo[r], hi[r], pair_t{x.to, y.to});
        store_pair(F.qb, j, e0[r], lo[r], hi[r], pair_t{x.qb, y.qb});
        if (F.qow.p) store_pair(F.qow, j, e0[r], lo[r], hi[r], pair_t{x.qow, y.qow});
    }
}

namespace {
using MlFn = void (*)(const MixedLayerDev&, const MixedLayerFields&, dim3, hipStream_t);
template <int B>
void ml_inst(const MixedLayerDev& M, const MixedLayerFields& F, dim3 g, hipStream_t st) {
    hipLaunchKernelGGL((k_mixed_layer<(B & 1) != 0, (B & 2) != 0, (B & 4) != 0, (B & 8) != 0>), g, dim3(kBx, kBy), 0, st, M, F);
}
template <int... B>
constexpr MlFn ml_table_entry(int b, std::integer_sequence<int, B...>) {
    constexpr MlFn t[] = {&ml_inst<B>...};
    return t[b];
}
}  // namespace

void launch_mixed_layer(const MixedLayerDev& M, const MixedLayerFields& F, hipStream_t s) {
    if (M.nx <= 0 || M.ny <= 0) return;
    const int pairs = M.nx / 2 + 1;                      // a row that starts odd has one pair more
    const dim3 g((unsigned)((pairs + kBx - 1) / kBx), (unsigned)((M.ny + kBy * kRows - 1) / (kBy * kRows)));
    const int b = (F.fo.p ? 1 : 0) | (F.k.p ? 2 : 0) | (F.qd.p ? 4 : 0) | (F.sb.p ? 8 : 0);
    ml_table_entry(b, std::make_integer_sequence<int, 16>{})(M, F, g, s);
}

}  // namespace csi
