// tracers.hip -- advected ice tracers (include/csi.h, "advected ice tracers and ice age": that comment is the definition).
//
//   k_tracer_tendencies   the FIRST HALF of a stage for every tracer in ONE launch: G = -horizontal_div_Uc(c) (or of q = aice c, the
//                         product formed on load), with the reconstructions, the order reduction and the closed-face rule of
//                         advect_dev.h -- the functions k_tendencies calls for h, aice and the snow thickness, so a PLAIN tracer gets
//                         the operations hs gets --, then c* = c^- + dtau G (or the concentration-weighted quotient) into the dense c*.
//   k_tracer_star_noadv   the first half with scheme == 0 (G = 0): point-wise.
//   k_tracer_finish       the SECOND HALF for every tracer in one point-wise launch: clip, zero rule, source, halo images.
//
// Compiled with -ffp-contract=off like advect.hip.  Layout of k_tracer_tendencies: one thread per cell of a (TX + 1) x (TY + 1) flux
// tile owns the west and south face of its cell for NTR tracers; tracer groups on blockIdx.z.  The face velocity, its sign, the
// order-reduction decision, the closed-face test, the face area, the address arithmetic and -- for weighted tracers -- the aice line
// are formed once per face and shared by the thread's NTR tracers (round 5 measured that these were half of a thread's instructions
// in k_tendencies); fluxes are exchanged through LDS as there.  A tracer's own operations do not depend on NTR or on its place in the
// group: results are the same bits in every layout.
#include "csi_dev.h"
#include "csi_kernels.h"
#include "evp_fast_math.h"
#include "advect_dev.h"

namespace csi {
namespace trc {

// 64 x 8 threads = 8 full waves: the 63 x 7 shape of k_tendencies' two-tracer layout (advect.hip)
constexpr int TTX = 63, TTY = 7;

// the values of the thread's NTR tracers on a line of W cells around the upwind cell `up`, element stride s, handed to f; the aice
// line is loaded once where any tracer of the group is weighted, and q = aice * c is ONE rounded product per stencil point
template <int W, int NTR, class F>
__device__ __forceinline__ void line_values(const TracersDev& T, int t0, long up, long s, bool anyw, F f, double (&out)[NTR]) {
    double aw[W];
#pragma unroll
    for (int k = 0; k < W; ++k) aw[k] = anyw ? T.a.p[up + (k - W / 2) * s] : 0.0;
#pragma unroll
    for (int t = 0; t < NTR; ++t) {
        out[t] = 0.0;
        if (t0 + t < T.n) {
            const double* cp = T.cin[t0 + t];
            const bool wt = T.weighting[t0 + t] != 0;
            double p[W];
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const double v = cp[up + (k - W / 2) * s];
                p[k] = wt ? aw[k] * v : v;
            }
            out[t] = f(p);
        }
    }
}

// adv::reconstruct for NTR tracers at once: the same choice of function per buffer B, the same window per function
template <int SCHEME, bool FAST, bool W32, int NTR>
__device__ __forceinline__ void face_values(const TracersDev& T, int t0, long off, long st, bool left, int B, bool anyw, double (&out)[NTR]) {
    const long up = left ? off - st : off;
    const long s = left ? st : -st;
    constexpr bool WENO = SCHEME > 0;
    if (SCHEME == 1 || B == 1) {
        line_values<1, NTR>(T, t0, up, s, anyw, [](const double* p) { return p[0]; }, out);
        return;
    }
    if (B == 2) {
        line_values<3, NTR>(T, t0, up, s, anyw, [](const double* p) {
            return WENO ? (W32 ? adv::weno3_w32<FAST>(p) : (FAST ? adv::weno3_fast(p) : adv::weno3(p))) : (FAST ? adv::upwind3_fast(p) : adv::upwind3(p));
        }, out);
        return;
    }
    if (B == 3 || SCHEME != 7) {
        line_values<5, NTR>(T, t0, up, s, anyw, [](const double* p) {
            return WENO ? (W32 ? adv::weno5_w32<FAST>(p) : (FAST ? adv::weno5_fast(p) : adv::weno5(p))) : (FAST ? adv::upwind5_fast(p) : adv::upwind5(p));
        }, out);
        return;
    }
    line_values<7, NTR>(T, t0, up, s, anyw, [](const double* p) {
        return W32 ? adv::weno7_w32<FAST>(p) : (FAST ? adv::weno7_fast(p) : adv::weno7(p));
    }, out);
}

// c* of tracer k at cell (i, j)
__device__ __forceinline__ double* star_at(const TracersDev& T, int k, int i, int j) {
    return T.star + (long)k * T.star_plane + (i - 1) + (long)(j - 1) * T.star_ld;
}
// the first half's update at one cell, G given: PLAIN c^- + dtau G; BY_CONCENTRATION ((aice^- c^-) + dtau G) / aice* where aice* > 0
__device__ __forceinline__ double star_value(bool wt, double cb, double ab, double as, double dt, double G) {
    return wt ? (as > 0 ? ((ab * cb) + dt * G) / as : 0.0) : cb + dt * G;
}

template <int SCHEME, bool FAST, bool W32, int NTR>
__global__ void __launch_bounds__((TTX + 1) * (TTY + 1)) k_tracer_tendencies(TracersDev T) {
    __shared__ double sFx[NTR][TTY + 1][TTX + 2], sFy[NTR][TTY + 1][TTX + 2];
    const GridDev& g = T.g;
    const int tx = threadIdx.x, ty = threadIdx.y, t0 = blockIdx.z * NTR;          // tx in [0, TTX], ty in [0, TTY]
    const int i = 1 + blockIdx.x * TTX + tx, j = 1 + blockIdx.y * TTY + ty;
    const long off = i + (long)j * T.ld;
    bool anyw = false;
#pragma unroll
    for (int t = 0; t < NTR; ++t) anyw |= (t0 + t < T.n) && T.weighting[t0 + t] != 0;
    if (i <= g.Nx + 1 && j <= g.Ny + 1) {
        if (ty < TTY && j <= g.Ny) {
            const double uu = T.u(i, j);
            const bool left = uu > 0;
            const int B = adv::buffer_at<SCHEME>(g, i, j, false, left);
            const bool closed = g.has_mask && peripheral_u(g, i, j);          // conditional_flux_fcc
            const double ax = dym(g, LOC_F, LOC_C, i, j);                    // Ax^{fcc} = dy^{fcc} * dz
            double cc[NTR];
            face_values<SCHEME, FAST, W32, NTR>(T, t0, off, 1, left, B, anyw, cc);
#pragma unroll
            for (int t = 0; t < NTR; ++t) sFx[t][ty][tx] = closed ? 0.0 : ax * uu * cc[t];
        }
        if (tx < TTX && i <= g.Nx) {
            const double vv = T.v(i, j);
            const bool left = vv > 0;
            const int B = adv::buffer_at<SCHEME>(g, i, j, true, left);
            const double dxf = dxm(g, LOC_C, LOC_F, i, j);                   // Ay^{cfc} = dx^{cfc} * dz
            const bool closed = g.has_mask && peripheral_v(g, i, j);          // conditional_flux_cfc
            double cc[NTR];
            face_values<SCHEME, FAST, W32, NTR>(T, t0, off, T.ld, left, B, anyw, cc);
#pragma unroll
            for (int t = 0; t < NTR; ++t) sFy[t][ty][tx] = closed ? 0.0 : dxf * vv * cc[t];
        }
    }
    __syncthreads();
    if (tx < TTX && ty < TTY && i <= g.Nx && j <= g.Ny) {
        const double V = azm(g, LOC_C, LOC_C, i, j);
        const double rV = FAST ? fm::rcp(V) : 1 / V;
        double ab = 0.0, as = 0.0;
        if (anyw) {
            ab = T.ab(i, j);
            as = ab + T.dt * T.Ga(i, j);
        }
#pragma unroll
        for (int t = 0; t < NTR; ++t) {
            const int k = t0 + t;
            if (k < T.n) {
                const double cb = T.cb[k][off];
                const double fx = sFx[t][ty][tx + 1] - sFx[t][ty][tx], fy = sFy[t][ty + 1][tx] - sFy[t][ty][tx];
                const double Gv = -(rV * (fx + fy));
                if (T.G[k]) T.G[k][off] = Gv;
                *star_at(T, k, i, j) = star_value(T.weighting[k] != 0, cb, ab, as, T.dt, Gv);
            }
        }
    }
}

// scheme == 0: G = 0 (horizontal_div_Uc(..., ::Nothing, ...) = zero(grid)), the same update expression; tracer on blockIdx.z
__global__ void __launch_bounds__(256) k_tracer_star_noadv(TracersDev T) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y, k = blockIdx.z;
    if (i > T.g.Nx || j > T.g.Ny) return;
    const long off = i + (long)j * T.ld;
    const bool wt = T.weighting[k] != 0;
    const double cb = T.cb[k][off];
    const double ab = wt ? T.ab(i, j) : 0.0, ga = wt ? T.Ga(i, j) : 0.0;
    if (T.G[k]) T.G[k][off] = 0.0;
    *star_at(T, k, i, j) = star_value(wt, cb, ab, ab + T.dt * ga, T.dt, 0.0);
}

// the second half at one cell: the clipped value where the cell keeps ice (else 0), without the source (free) and with it (c)
__device__ __forceinline__ void finish_values(bool nonneg, double star, double a, bool active, double add, double& c, double& free) {
    const double x = nonneg ? jmax(0.0, star) : star;
    const bool ice = a > 0 && active;
    free = ice ? x : 0.0;
    c = ice ? x + add : 0.0;
}
// One thread: two neighbouring cells (i, i + 1) of row j of tracer blockIdx.z.  c* is dense with an even row stride: its pair is one
// 16-byte load; the pairs of aice and c are 16-byte accesses where their rows start so (decided per thread from the address).  Every
// load is issued before the first value is used.
__global__ void __launch_bounds__(256) k_tracer_finish(TracersDev T) {
    const GridDev& g = T.g;
    const int i = 1 + 2 * (int)(blockIdx.x * blockDim.x + threadIdx.x), j = 1 + blockIdx.y * blockDim.y + threadIdx.y, k = blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
    const bool two = i + 1 <= g.Nx;
    const double* sp = star_at(T, k, i, j);
    const double* ap = &T.a(i, j);
    double* cp = T.c[k] + i + (long)j * T.ld;
    double s0, s1 = 0.0, a0, a1 = 0.0;
    if (two) { const double2 s = *reinterpret_cast<const double2*>(sp); s0 = s.x; s1 = s.y; } else s0 = sp[0];
    if (two && ((uintptr_t)ap & 15) == 0) { const double2 a = *reinterpret_cast<const double2*>(ap); a0 = a.x; a1 = a.y; }
    else { a0 = ap[0]; if (two) a1 = ap[1]; }
    bool act0 = true, act1 = true;
    if (g.has_mask) {
        const uint8_t* mp = g.mask + i + (long)j * g.mask_ld;
        const uint8_t m0 = mp[0], m1 = two ? mp[1] : (uint8_t)0;
        act0 = m0 != 0; act1 = m1 != 0;
    }
    const bool nonneg = T.nonnegative[k] != 0;
    const double add = T.dt * T.source[k];
    double c0, c1, f0, f1;
    finish_values(nonneg, s0, a0, act0, add, c0, f0);
    finish_values(nonneg, s1, a1, act1, add, c1, f1);
    double* fp = T.cfree[k] ? T.cfree[k] + i + (long)j * T.ld : nullptr;      // (the source-free copy: the next RK stage's stencil input)
    if (two && (((uintptr_t)cp | (uintptr_t)fp) & 15) == 0 && !has_halo_images(g, T.im, i, j) && !has_halo_images(g, T.im, i + 1, j)) {
        *reinterpret_cast<double2*>(cp) = make_double2(c0, c1);
        if (fp) *reinterpret_cast<double2*>(fp) = make_double2(f0, f1);
        return;
    }
    const FRef f{T.c[k], (int)T.ld};
    store_with_images(f, g, T.im, i, j, c0);
    if (two) store_with_images(f, g, T.im, i + 1, j, c1);
    if (fp) {
        const FRef ff{T.cfree[k], (int)T.ld};
        store_with_images(ff, g, T.im, i, j, f0);
        if (two) store_with_images(ff, g, T.im, i + 1, j, f1);
    }
}

}  // namespace trc

// NTR, tracers per thread: the rule, and the measurement behind it, are stated in profiles/r30_tracers.md.  force: 1 / 2 / 4 (tuning aid
// / tests: CSI_TRACERS_NTR, read when the context is created), 0: by the rule -- the smallest of 1, 2, 4 that holds all n tracers in one
// group, 4 beyond
static int tracers_per_thread(int n, int force) {
    if (force == 1 || force == 2 || force == 4) return force;
    return n >= 3 ? 4 : n;
}
template <bool FAST, int NTR>
static void launch_tendencies_ntr(const TracersDev& T, dim3 gr, dim3 b, hipStream_t s) {
    const bool w = T.w32 != 0;
#define CSI_TRC_LAUNCH(S, W) hipLaunchKernelGGL((trc::k_tracer_tendencies<S, FAST, W, NTR>), gr, b, 0, s, T)
    switch (T.scheme) {
        case 1: CSI_TRC_LAUNCH(1, false); break;
        case 3: if (w) CSI_TRC_LAUNCH(3, true); else CSI_TRC_LAUNCH(3, false); break;
        case -3: CSI_TRC_LAUNCH(-3, false); break;
        case 5: if (w) CSI_TRC_LAUNCH(5, true); else CSI_TRC_LAUNCH(5, false); break;
        case -5: CSI_TRC_LAUNCH(-5, false); break;
        default: if (w) CSI_TRC_LAUNCH(7, true); else CSI_TRC_LAUNCH(7, false); break;
    }
#undef CSI_TRC_LAUNCH
}
TracerLayout launch_tracers_tendencies(const TracersDev& T, int mode, int force_ntr, hipStream_t s) {
    const int ntr = tracers_per_thread(T.n, force_ntr), groups = (T.n + ntr - 1) / ntr;
    dim3 b(trc::TTX + 1, trc::TTY + 1, 1);
    dim3 gr((unsigned)((T.g.Nx + trc::TTX - 1) / trc::TTX), (unsigned)((T.g.Ny + trc::TTY - 1) / trc::TTY), (unsigned)groups);
    const bool fast = mode == 1;
    if (ntr == 1) { if (fast) launch_tendencies_ntr<true, 1>(T, gr, b, s); else launch_tendencies_ntr<false, 1>(T, gr, b, s); }
    else if (ntr == 2) { if (fast) launch_tendencies_ntr<true, 2>(T, gr, b, s); else launch_tendencies_ntr<false, 2>(T, gr, b, s); }
    else { if (fast) launch_tendencies_ntr<true, 4>(T, gr, b, s); else launch_tendencies_ntr<false, 4>(T, gr, b, s); }
    return TracerLayout{ntr, trc::TTX, trc::TTY, groups};
}
void launch_tracers_star_noadv(const TracersDev& T, hipStream_t s) {
    dim3 b(64, 4);
    hipLaunchKernelGGL(trc::k_tracer_star_noadv, dim3((unsigned)((T.g.Nx + 63) / 64), (unsigned)((T.g.Ny + 3) / 4), (unsigned)T.n), b, 0, s, T);
}
void launch_tracers_finish(const TracersDev& T, hipStream_t s) {
    dim3 b(64, 4);
    hipLaunchKernelGGL(trc::k_tracer_finish, dim3((unsigned)((T.g.Nx + 127) / 128), (unsigned)((T.g.Ny + 3) / 4), (unsigned)T.n), b, 0, s, T);
}

}  // namespace csi
