// derived.hip -- derived (Center, Center) fields of the bound state in one launch (include/csi.h: csi_derived_compute).
//
//   k_derived<MK, STRESS>   one thread per cell i = 1 .. Nx, j = 1 .. Ny; blocks of 64 x 4 threads, consecutive lanes on consecutive
//                           columns.  MK: metric kind (uniform / per row / per point), STRESS: the stress group is requested as well.
// A stencil kernel on the cache: a cell reads u at (i .. i + 1, j - 1 .. j + 1), v at (i - 1 .. i + 1, j .. j + 1), with STRESS sigma12 at
// its four corners and sigma11, sigma22, P at the centre; the neighbours' elements are the same lines the neighbouring lanes and rows
// load, so from HBM every array is read once (12 + 12 metric planes aside): compulsory traffic 16 B per cell in, 8 B per requested
// field out, + 48 B in with STRESS.  No LDS: the stencil's reuse is one element left and right (the same wave's line) and one row up
// and down (the block's own rows, L1 / L2), and a tile staged in LDS would need a barrier between its halo loads and the first use.
// Every load of a cell precedes its first store (the stores are the last statements; the outputs are other arrays than the inputs),
// so the compiler issues the loads together.  No atomics, no flags.  Compiled without contraction: STRICT and FAST run this code.
// Threads beyond the grid leave at once; nothing outside the elements named in include/csi.h is addressed.
#include "csi_kernels.h"
#include "derived_dev.h"
#include <math.h>

namespace csi {
namespace dv {

template <int MK, bool STRESS>
__global__ void __launch_bounds__(256) k_derived(DerivedDev D) {
    const GridDev& g = D.g;
    const int i = 1 + (int)(blockIdx.x * 64 + threadIdx.x), j = 1 + (int)(blockIdx.y * 4 + threadIdx.y);
    if (i > g.Nx || j > g.Ny) return;
    const FRef &u = D.u, &v = D.v;
    const double e11 = e_xx<MK>(g, u, v, i, j), e22 = e_yy<MK>(g, u, v, i, j);
    const double x00 = e_xy<MK>(g, u, v, i, j), x10 = e_xy<MK>(g, u, v, i + 1, j);
    const double x01 = e_xy<MK>(g, u, v, i, j + 1), x11 = e_xy<MK>(g, u, v, i + 1, j + 1);
    const double e12c = avg4(x00, x10, x01, x11);
    const double uc = (u.ld_(i, j) + u.ld_(i + 1, j)) / 2, vc = (v.ld_(i, j) + v.ld_(i, j + 1)) / 2;
    const double div = e11 + e22;
    const double shear = sqrt((e11 - e22) * (e11 - e22) + 4 * (e12c * e12c));
    const double deform = sqrt(div * div + shear * shear);
    const double speed = sqrt(uc * uc + vc * vc);
    double sI = 0.0, sII = 0.0, power = 0.0;
    if (STRESS) {
        const double s11 = D.s11.ld_(i, j), s22 = D.s22.ld_(i, j), P = D.P.ld_(i, j);
        const double t00 = D.s12.ld_(i, j), t10 = D.s12.ld_(i + 1, j), t01 = D.s12.ld_(i, j + 1), t11 = D.s12.ld_(i + 1, j + 1);
        const double s12c = avg4(t00, t10, t01, t11);
        const double half = (s11 - s22) / 2;
        const double qI = ((s11 + s22) / 2) / P;
        const double qII = sqrt(half * half + s12c * s12c) / P;
        sI = (P == 0) ? 0.0 : qI;
        sII = (P == 0) ? 0.0 : qII;
        power = (s11 * e11 + s22 * e22) + 2 * avg4(t00 * x00, t10 * x10, t01 * x01, t11 * x11);
    }
    const bool land = g.has_mask && g.mask[i + (long)j * g.mask_ld] == 0;
    const double val[DV_COUNT] = {div, shear, deform, speed, sI, sII, power};
#pragma unroll
    for (int k = 0; k < (STRESS ? DV_COUNT : DV_SIGMA_I); ++k)
        if (D.out[k].p) D.out[k](i, j) = land ? 0.0 : val[k];
}

template <int MK>
static void launch_mk(const DerivedDev& D, bool stress, dim3 grid, dim3 block, hipStream_t s) {
    if (stress) hipLaunchKernelGGL((k_derived<MK, true>), grid, block, 0, s, D);
    else hipLaunchKernelGGL((k_derived<MK, false>), grid, block, 0, s, D);
}

}  // namespace dv

void launch_derived(const DerivedDev& D, bool stress, hipStream_t s) {
    const dim3 b(64, 4), g((unsigned)((D.g.Nx + 63) / 64), (unsigned)((D.g.Ny + 3) / 4), 1);
    if (D.g.metric_kind == 0) dv::launch_mk<0>(D, stress, g, b, s);
    else if (D.g.metric_kind == 1) dv::launch_mk<1>(D, stress, g, b, s);
    else dv::launch_mk<2>(D, stress, g, b, s);
}

}  // namespace csi
