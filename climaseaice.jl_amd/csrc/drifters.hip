// drifters.hip -- Lagrangian ice drifters advected and sampled on the device (include/csi.h: csi_drifters_advance, csi_drifters_sample).
//
//   k_drifters_advance<MK, MASK>   one thread per drifter, blocks of 256; all m sub-steps of the midpoint rule in ONE launch: position and
//                                  status are read once and stored once, the intermediate positions live in registers.  MK: metric
//                                  kind (uniform / per row / per point), MASK: a land mask is set.
//   k_drifters_sample              one thread per drifter; the requested columns at the current positions, column-major: consecutive
//                                  lanes store consecutive elements of a column.
// GATHER kernels, the first of the library: the state is a list, not a grid, and what a drifter costs is the element-granular read of
// the velocity planes around its position -- 2 x 2 elements of u, of v and (MK = 1, 2) of their metrics per rate evaluation, two
// evaluations per sub-step.  Neighbouring lanes share lines only where neighbouring drifters share cells, so the ORDER of the list
// decides how much of that L2 and the Infinity Cache absorb (profiles/r28_drifters.md measures grid order against a shuffled list).
// The rule itself is drifters_dev.h; DevSource hands it the fields: every load of one rate evaluation is issued before the first value
// is used (sixteen independent loads, eight with MK = 0, then the divisions), the idiom of momentum_dev.h.  No LDS (nothing is shared
// between drifters), no atomics, no flags.  Compiled without contraction: STRICT and FAST run this code.
// Addresses: locate() clamps every index as a double before the conversion (columns 0 .. Nx + 1, rows 0 .. Ny + 1 -- the one ring the
// header names -- whatever the position holds, NaN and +-Inf included); threads beyond n leave at once.
#include "../../include/csi.h"
#include "csi_kernels.h"
#include "derived_dev.h"
#include "drifters_dev.h"

namespace csi {
namespace drift {

template <int MK, bool MASK>
struct DevSource {
    const GridDev& g;
    const FRef& u;
    const FRef& v;
    __device__ __forceinline__ void load_u(int i, int j, double* num, double* den) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) num[k] = u.ld_(i + (k & 1), j + (k >> 1));
#pragma unroll
        for (int k = 0; k < 4; ++k) den[k] = dv::dx_<MK>(g, LOC_F, LOC_C, i + (k & 1), j + (k >> 1));
    }
    __device__ __forceinline__ void load_v(int i, int j, double* num, double* den) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) num[k] = v.ld_(i + (k & 1), j + (k >> 1));
#pragma unroll
        for (int k = 0; k < 4; ++k) den[k] = dv::dy_<MK>(g, LOC_C, LOC_F, i + (k & 1), j + (k >> 1));
    }
    __device__ __forceinline__ bool land(int i, int j) const { return MASK && g.mask[i + (long)j * g.mask_ld] == 0; }
};

template <int MK, bool MASK>
__global__ void __launch_bounds__(256) k_drifters_advance(DriftersDev D, double tau, int m) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= D.n) return;
    double xi = D.xi[q], eta = D.eta[q];
    if (!(finite_(xi) && finite_(eta))) {      // inactive: nothing is read for it, its position stays as it is
        D.status[q] = INACTIVE;
        return;
    }
    const DevSource<MK, MASK> src{D.g, D.u, D.v};
    const Dom dom{D.g.Nx, D.g.Ny, D.g.xlo == SIDE_PERIODIC, D.g.ylo == SIDE_PERIODIC};
    int status = 0;
    for (int s = 0; s < m; ++s)
        if (!substep(src, dom, tau, xi, eta, status)) break;
    D.xi[q] = xi;
    D.eta[q] = eta;
    D.status[q] = status;
}

__global__ void __launch_bounds__(256) k_drifters_sample(DriftersDev D, int columns, double* out, long ld) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= D.n) return;
    const double xi = D.xi[q], eta = D.eta[q];
    const bool active = finite_(xi) && finite_(eta);
    const Stencil s = locate(D.g.Nx, D.g.Ny, xi, eta);      // (inside the ring for every input: the loads below need no test)
    double val[7] = {xi, eta, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (columns & CSI_DRIFTER_COL_U)
        val[2] = bilinear(s.sx, s.sy, D.u.ld_(s.ia, s.ja), D.u.ld_(s.ia + 1, s.ja), D.u.ld_(s.ia, s.ja + 1), D.u.ld_(s.ia + 1, s.ja + 1));
    if (columns & CSI_DRIFTER_COL_V)
        val[3] = bilinear(s.ry, s.rx, D.v.ld_(s.ib, s.jb), D.v.ld_(s.ib, s.jb + 1), D.v.ld_(s.ib + 1, s.jb), D.v.ld_(s.ib + 1, s.jb + 1));
    if (columns & CSI_DRIFTER_COL_H) val[4] = D.h.ld_(s.ic, s.jc);
    if (columns & CSI_DRIFTER_COL_A) val[5] = D.a.ld_(s.ic, s.jc);
    if (columns & CSI_DRIFTER_COL_HS) val[6] = D.hs.ld_(s.ic, s.jc);
    long k = 0;
#pragma unroll
    for (int c = 0; c < 7; ++c)
        if (columns & (1 << c)) {
            out[k * ld + q] = active ? val[c] : NAN;
            ++k;
        }
}

template <int MK>
static void launch_mk(const DriftersDev& D, double tau, int m, unsigned blocks, hipStream_t s) {
    if (D.g.has_mask) hipLaunchKernelGGL((k_drifters_advance<MK, true>), dim3(blocks), dim3(256), 0, s, D, tau, m);
    else hipLaunchKernelGGL((k_drifters_advance<MK, false>), dim3(blocks), dim3(256), 0, s, D, tau, m);
}

}  // namespace drift

void launch_drifters_advance(const DriftersDev& D, double tau, int m, hipStream_t s) {
    const unsigned blocks = (unsigned)((D.n + 255) / 256);
    if (D.g.metric_kind == 0) drift::launch_mk<0>(D, tau, m, blocks, s);
    else if (D.g.metric_kind == 1) drift::launch_mk<1>(D, tau, m, blocks, s);
    else drift::launch_mk<2>(D, tau, m, blocks, s);
}

void launch_drifters_sample(const DriftersDev& D, int columns, double* out, long ld, hipStream_t s) {
    hipLaunchKernelGGL(drift::k_drifters_sample, dim3((unsigned)((D.n + 255) / 256)), dim3(256), 0, s, D, columns, out, ld);
}

}  // namespace csi
