// advect.hip -- h / aice advection tendencies and the tracer update.
//
//   k_tendencies  _compute_dynamic_tracer_tendencies!  tracer_tendency_kernel_functions.jl:27-45
//                 = - horizontal_div_Uc (sea_ice_advection.jl:51-54) with the upstream
//                 Oceananigans upwind-biased reconstructions (WENO(order = 5 | 7) in the WENO-Z
//                 form, UpwindBiased(order = 5), first-order upwind), their
//                 order reduction next to walls and immersed cells, zero flux through immersed faces.
//   k_tracer_step _dynamic_step_tracers!               sea_ice_fe_step.jl:56-82
//                 (RK3: h^n, aice^n = Psi^-, sea_ice_rk_substep.jl:140-149)
//
// This translation unit is compiled with -ffp-contract=off.  STRICT mode keeps the oracle's expression order and IEEE
// divisions: bit-identical tracer tendencies.  FAST mode (round 3) evaluates the SAME reconstructions -- same stencils,
// same smoothness indicators, same WENO-Z weights per tracer, same order reduction -- with the divisions by constants as
// multiplications, the four or five true divisions of a reconstruction as hardware reciprocal + one Newton step (fm::rcp,
// relative error <= 130 u, u = 2^-53, under the seed cap tests/test_gpu_fast_math.py holds: RCP_U of
// tests/fast_math_ref.py, the figure the per-face bounds of tests/advect_ref.py count a reciprocal with) and fused
// multiply-adds: a WENO7 reconstruction is ~150 instead of ~450 instructions (nine IEEE divisions of ~35 instructions
// each were two thirds of it).  Stated tolerance: |dG| <= 1e-12 max|G| on the tendencies (round 5: contracted smoothness
// indicators, below; 1e-13 before), 1e-13 relative on h, aice after a step (measured ~1e-16); masks, zero sets and the
// order-reduction decisions are the same code.  Each thread owns one
// face pair (west, south) of its cell: fluxes are computed once, shared with the east / north
// neighbours through LDS, so every face flux is evaluated exactly once per tile interior.
#include <cstdlib>

#include "csi_dev.h"
#include "csi_kernels.h"
#include "evp_fast_math.h"
#include "advect_dev.h"

namespace csi {
namespace adv {

// measured (scripts/r03_adv_shapes.sh, us per RK3 step at 512^2 / 1024^2 / 2048^2): 64 x 4 cells per block 55 / 185 / 762, 64 x 6: 52 / 171 / 704,
// 32 x 12: 51 / 176 / 693, 40 x 10: 54 / 171 / 709, 64 x 2: 64 / 208 / 849 (the extra face row / column of a tile is redundant work)
#ifndef CSI_ADV_TY
#define CSI_ADV_TY 6
#endif
#ifndef CSI_ADV_TX
#define CSI_ADV_TX 64
#endif
constexpr int TX = CSI_ADV_TX, TY2 = CSI_ADV_TY, TY3 = 4;      // rows of a flux tile with two tracers / with three (snow): (TX + 1)(TY + 1) tracers <= 1024 threads

// One thread per cell AND TRACER of a (TX+1) x (TY+1) flux tile (threadIdx.z: h, aice [, snow thickness]): the extra column /
// row holds the east / north faces of the tile.  Fx[i] = Ax u c~ at the west face of cell i, Fy[j] at the south face.  (Round 3:
// the tracers used to share a thread -- four WENO7 reconstructions behind 28 dependent loads; at 512^2 the launch lasts as long
// as one block, so halving the chain per thread is what shortens it.)
// store_with_images for a tracer on a grid with N >= 2 H and no fold: a cell is within H of at most one side per direction, so it
// has at most one x image, one y image and their corner -- scalars instead of store_with_images' four slots (a specialisation
// under that precondition, kept because it sits in the advection hot loop)
__device__ __forceinline__ void store_tracer_images(const FRef& f, const GridDev& g, const ImageSpec& im, int i, int j, double val) {
    f(i, j) = val;
    int ix = 0, jy = 0;
    bool hx = false, hy = false;
    if (i <= g.Hx) {
        if (im.xhi == IMG_WRAP) { ix = i + g.Nx; hx = true; }
        if (im.xlo == IMG_MIRROR) { ix = 1 - i; hx = true; }
    } else if (i > g.Nx - g.Hx) {
        if (im.xlo == IMG_WRAP) { ix = i - g.Nx; hx = true; }
        if (im.xhi == IMG_MIRROR) { ix = 2 * g.Nx + 1 - i; hx = true; }
    }
    if (j <= g.Hy) {
        if (im.yhi == IMG_WRAP) { jy = j + g.Ny; hy = true; }
        if (im.ylo == IMG_MIRROR) { jy = 1 - j; hy = true; }
    } else if (j > g.Ny - g.Hy) {
        if (im.ylo == IMG_WRAP) { jy = j - g.Ny; hy = true; }
        if (im.yhi == IMG_MIRROR) { jy = 2 * g.Ny + 1 - j; hy = true; }
    }
    if (hx) f(ix, j) = val;
    if (hy) f(i, jy) = val;
    if (hx & hy) f(ix, jy) = val;
}

// STEP (launch_advect_stage): the launch is a whole RK stage of an advection-only model -- the h thread of a cell also does
// _dynamic_step_tracers! (k_tracer_step's arithmetic, statement for statement) with the two tendencies of its cell, into the
// stage's OUTPUT arrays.
// NT (round 5): tracers per thread.  1: one thread per cell AND tracer (threadIdx.z), the latency-optimal layout of small grids
// (round 3: at 512^2 a launch lasts as long as one block).  2: one thread per cell does h AND aice -- the face velocity and its
// sign, the order-reduction decision, the closed-face test, the face area and the stencil's address arithmetic are the same for
// both tracers and were half of a thread's instructions (ISA: ~300 of ~590 per cell and tracer were not the reconstruction's
// arithmetic); large grids, which are throughput-bound (VALU busy 0.68 at 2048^2), take this one.  Same operations per value:
// bit-identical to NT = 1.
template <int SCHEME, bool FAST, bool STEP = false, int TY = TY2, bool W32 = false, int NT = 1, int TXP = TX>
__global__ void __launch_bounds__(NT == 2 ? (TXP + 1) * (TY + 1) : 1024) k_tendencies(AdvDev A) {
    __shared__ double sFx[NT == 2 ? 2 : 3][TY + 1][TXP + 2], sFy[NT == 2 ? 2 : 3][TY + 1][TXP + 2];
    __shared__ double sG[(STEP && NT == 1) ? 2 : 1][(STEP && NT == 1) ? TY : 1][(STEP && NT == 1) ? TXP : 1];
    const GridDev& g = A.g;
    const int tx = threadIdx.x, ty = threadIdx.y, tz = NT == 2 ? 0 : threadIdx.z;          // tx in [0, TX], ty in [0, TY], tz: tracer
    const int i = 1 + blockIdx.x * TXP + tx, j = 1 + blockIdx.y * TY + ty;
    const bool in_x = i <= g.Nx + 1, in_y = j <= g.Ny + 1;
    const FRef& c = tz == 0 ? A.h : (tz == 1 ? A.a : A.hs);
    // STEP: the update's base values are independent of the fluxes: loaded (and, first stage, cached as Psi^-) up front, so that
    // behind the fluxes only a few flops and one store remain; the h thread stores h, the aice thread aice
    const bool owns = tx < TXP && ty < TY && i <= g.Nx && j <= g.Ny;
    double hn = 0.0, an = 0.0;
    if (STEP && owns) {
        hn = A.hb(i, j); an = A.ab(i, j);
        if (A.write_cache) {              // Psi^- = the state this step starts from (its halos: images, like the state's)
            if (NT == 2 || tz == 0) store_tracer_images(A.hm, A.g, A.im, i, j, hn);
            if (NT == 2 || tz != 0) store_tracer_images(A.am, A.g, A.im, i, j, an);
        }
    }
    if (in_x && in_y) {
        // x-face flux (needed for ty < TY rows), y-face flux (needed for tx < TX columns)
        if (ty < TY && j <= g.Ny) {
            const double uu = A.u(i, j);
            const bool left = uu > 0;
            const int B = buffer_at<SCHEME>(g, i, j, false, left);
            const bool closed = g.has_mask && peripheral_u(g, i, j);          // conditional_flux_fcc
            const double ax = dym(g, LOC_F, LOC_C, i, j);                    // Ax^{fcc} = dy^{fcc} * dz
            const double cc = reconstruct<SCHEME, FAST, W32>(&c(i, j), 1, left, B);
            sFx[tz][ty][tx] = closed ? 0.0 : ax * uu * cc;
            if (NT == 2) {
                const double c2 = reconstruct<SCHEME, FAST, W32>(&A.a(i, j), 1, left, B);
                sFx[1][ty][tx] = closed ? 0.0 : ax * uu * c2;
            }
        }
        if (tx < TXP && i <= g.Nx) {
            const double vv = A.v(i, j);
            const bool left = vv > 0;
            const int B = buffer_at<SCHEME>(g, i, j, true, left);
            const double dxf = dxm(g, LOC_C, LOC_F, i, j);                   // Ay^{cfc} = dx^{cfc} * dz
            const bool closed = g.has_mask && peripheral_v(g, i, j);          // conditional_flux_cfc
            const double cc = reconstruct<SCHEME, FAST, W32>(&c(i, j), c.ld, left, B);
            sFy[tz][ty][tx] = closed ? 0.0 : dxf * vv * cc;
            if (NT == 2) {
                const double c2 = reconstruct<SCHEME, FAST, W32>(&A.a(i, j), A.a.ld, left, B);
                sFy[1][ty][tx] = closed ? 0.0 : dxf * vv * c2;
            }
        }
    }
    __syncthreads();
    double G0 = 0.0, G1 = 0.0;
    if (tx < TXP && ty < TY && i <= g.Nx && j <= g.Ny) {
        const double V = azm(g, LOC_C, LOC_C, i, j);
        const double rV = FAST ? fm::rcp(V) : 1 / V;
        const double fx = sFx[tz][ty][tx + 1] - sFx[tz][ty][tx], fy = sFy[tz][ty + 1][tx] - sFy[tz][ty][tx];
        const FRef& G = tz == 0 ? A.Gh : (tz == 1 ? A.Ga : A.Ghs);         // (snow: compute_snow_advection_tendency!, tracer_tendency_kernel_functions.jl:49-52)
        const double Gv = -(rV * (fx + fy));
        G(i, j) = Gv;
        G0 = Gv;
        if (NT == 2) {
            const double fx2 = sFx[1][ty][tx + 1] - sFx[1][ty][tx], fy2 = sFy[1][ty + 1][tx] - sFy[1][ty][tx];
            G1 = -(rV * (fx2 + fy2));
            A.Ga(i, j) = G1;
        } else if (STEP) sG[tz][ty][tx] = Gv;
    }
    if (STEP) {
        if (NT == 1) __syncthreads();
        if (owns) {
            double hp = hn + A.dt * (NT == 2 ? G0 : sG[0][ty][tx]);
            double ap = an + A.dt * (NT == 2 ? G1 : sG[1][ty][tx]);
            ap = jmax(0.0, ap);
            hp = jmax(0.0, hp);
            ap = (hp == 0) ? 0.0 : ap;
            hp = (ap == 0) ? 0.0 : hp;
            const double Vp = hp * ap;
            const double a1 = (ap > 1) ? 1.0 : ap, h1 = (ap > 1) ? Vp : hp;
            if (NT == 2 || tz == 0) store_tracer_images(A.ho, A.g, A.im, i, j, h1);
            if (NT == 2 || tz != 0) store_tracer_images(A.ao, A.g, A.im, i, j, a1);
        }
    }
}

__global__ void __launch_bounds__(256) k_tracer_step(AdvDev A) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > A.g.Nx || j > A.g.Ny) return;
    const double hn = A.from_cache ? A.hm(i, j) : A.h(i, j);
    const double an = A.from_cache ? A.am(i, j) : A.a(i, j);
    double hp = hn + A.dt * A.Gh(i, j);
    double ap = an + A.dt * A.Ga(i, j);
    ap = jmax(0.0, ap);
    hp = jmax(0.0, hp);
    ap = (hp == 0) ? 0.0 : ap;
    hp = (ap == 0) ? 0.0 : hp;
    const double Vp = hp * ap;
    const double a1 = (ap > 1) ? 1.0 : ap, h1 = (ap > 1) ? Vp : hp;
    if (A.fill_images) {             // update_state!'s halo fill of h, aice fused into the stores (csi_abi.hip)
        store_with_images(A.a, A.g, A.im, i, j, a1);
        store_with_images(A.h, A.g, A.im, i, j, h1);
    } else {
        A.a(i, j) = a1;
        A.h(i, j) = h1;
    }
    if (A.has_snow) {                // dynamic_step_snow!, sea_ice_fe_step.jl:86-94
        const double sn = A.from_cache ? A.hsm(i, j) : A.hs(i, j);
        double sp = sn + A.dt * A.Ghs(i, j);
        sp = jmax(0.0, sp);
        const double s1 = (a1 <= 0) ? 0.0 : sp;
        if (A.fill_images) store_with_images(A.hs, A.g, A.im, i, j, s1); else A.hs(i, j) = s1;
    }
}

}  // namespace adv

// W32: the WENO weights in single precision (AdvDev::w32; only the WENO schemes have weights)
// NT: tracers per thread (k_tendencies): 2 from CSI_ADV_NT2_CELLS cells on.  Measured round 5 (scripts/adv_bench.py, one box, WENO7, us per
// advection-only RK3 step / per tendency launch, NT = 1 -> 2): 256^2 25.7 -> 25.8 / 7.0 -> 7.4; 512^2 53.5 -> 48.5 / 14.2 -> 13.0;
// 1024^2 171 -> 142 / 47 -> 38; 2048^2 728 -> 621 / 173 -> 139 (profiles/r05_advection.md)
#ifndef CSI_ADV_NT2_CELLS
#define CSI_ADV_NT2_CELLS 200000L
#endif
static bool adv_two_tracers(const AdvDev& A) {
    if (A.has_snow) return false;
    if (A.nt > 0) return A.nt == 2;              // tuning aid / tests (CSI_ADV_NT, read when the context is created)
    return (long)A.g.Nx * (long)A.g.Ny >= CSI_ADV_NT2_CELLS;
}
// Block shapes of the two-tracers-per-thread layout by grid size (round 5, one box, us per advection-only RK3 step at 512^2 / 1024^2 /
// 2048^2; profiles/r05_advection_shapes.txt): 64 x 6 cells 48.5 / 142 / 621; 64 x 8: 46 / 161 / 678; 63 x 7 (64 x 8 threads = 8 full
// waves): 49.5 / 132 / 591; 63 x 11: 49 / 138 / 577; 63 x 5: 53.5 / 150 / 646; 63 x 9: 60 / 154 / 650; 64 x 12: 63 / 175 / 715 -- not
// monotonic in anything simple (wave quantisation of the block, blocks per CU, redundant face rows), so: the best measured shape per size
enum { SHAPE_64x8 = 0, SHAPE_63x7 = 1, SHAPE_63x11 = 2 };
static int adv_shape(const AdvDev& A) {
    if (A.shape > 0) return A.shape - 1;         // tuning aid / tests (CSI_ADV_SHAPE, read when the context is created)
    const long cells = (long)A.g.Nx * (long)A.g.Ny;
    return cells < 600000L ? SHAPE_64x8 : (cells < 2500000L ? SHAPE_63x7 : SHAPE_63x11);
}
template <bool FAST, bool W32>
static AdvLayout launch_tendencies_mode(const AdvDev& A, hipStream_t s) {
    const bool two = adv_two_tracers(A);
    const int shape = adv_shape(A);
    const int tx = two ? (shape == SHAPE_64x8 ? 64 : 63) : adv::TX;
    const int ty = A.has_snow ? adv::TY3 : (two ? (shape == SHAPE_64x8 ? 8 : (shape == SHAPE_63x7 ? 7 : 11)) : adv::TY2);
    dim3 b(tx + 1, ty + 1, A.has_snow ? 3 : (two ? 1 : 2));
    dim3 gr((unsigned)((A.g.Nx + tx - 1) / tx), (unsigned)((A.g.Ny + ty - 1) / ty));
#define CSI_ADV_LAUNCH(S, W) do { if (A.has_snow) hipLaunchKernelGGL((adv::k_tendencies<S, FAST, false, adv::TY3, W>), gr, b, 0, s, A); \
                                  else if (two && shape == SHAPE_64x8) hipLaunchKernelGGL((adv::k_tendencies<S, FAST, false, 8, W, 2, 64>), gr, b, 0, s, A); \
                                  else if (two && shape == SHAPE_63x7) hipLaunchKernelGGL((adv::k_tendencies<S, FAST, false, 7, W, 2, 63>), gr, b, 0, s, A); \
                                  else if (two) hipLaunchKernelGGL((adv::k_tendencies<S, FAST, false, 11, W, 2, 63>), gr, b, 0, s, A); \
                                  else hipLaunchKernelGGL((adv::k_tendencies<S, FAST, false, adv::TY2, W>), gr, b, 0, s, A); } while (0)
    switch (A.scheme) {
        case 1: CSI_ADV_LAUNCH(1, false); break;
        case 3: CSI_ADV_LAUNCH(3, W32); break;
        case -3: CSI_ADV_LAUNCH(-3, false); break;
        case 5: CSI_ADV_LAUNCH(5, W32); break;
        case -5: CSI_ADV_LAUNCH(-5, false); break;
        default: CSI_ADV_LAUNCH(7, W32); break;
    }
#undef CSI_ADV_LAUNCH
    return AdvLayout{two ? 2 : 1, tx, ty};
}
// mode: CSI_MODE_STRICT (0) the oracle's arithmetic, bit for bit; CSI_MODE_FAST (1) reciprocals and contraction (header)
AdvLayout launch_tracer_tendencies(const AdvDev& A, int mode, hipStream_t s) {
    if (A.w32) return mode == 1 ? launch_tendencies_mode<true, true>(A, s) : launch_tendencies_mode<false, true>(A, s);
    return mode == 1 ? launch_tendencies_mode<true, false>(A, s) : launch_tendencies_mode<false, false>(A, s);
}
template <bool FAST, bool W32>
static AdvLayout launch_stage_mode(const AdvDev& A, hipStream_t s) {
    const bool two = adv_two_tracers(A);
    const int shape = adv_shape(A);
    const int tx = two ? (shape == SHAPE_64x8 ? 64 : 63) : adv::TX;
    const int ty = two ? (shape == SHAPE_64x8 ? 8 : (shape == SHAPE_63x7 ? 7 : 11)) : adv::TY2;
    dim3 b(tx + 1, ty + 1, two ? 1 : 2);
    dim3 gr((unsigned)((A.g.Nx + tx - 1) / tx), (unsigned)((A.g.Ny + ty - 1) / ty));
#define CSI_ADV_STAGE(S, W) do { if (two && shape == SHAPE_64x8) hipLaunchKernelGGL((adv::k_tendencies<S, FAST, true, 8, W, 2, 64>), gr, b, 0, s, A); \
                                 else if (two && shape == SHAPE_63x7) hipLaunchKernelGGL((adv::k_tendencies<S, FAST, true, 7, W, 2, 63>), gr, b, 0, s, A); \
                                 else if (two) hipLaunchKernelGGL((adv::k_tendencies<S, FAST, true, 11, W, 2, 63>), gr, b, 0, s, A); \
                                 else hipLaunchKernelGGL((adv::k_tendencies<S, FAST, true, adv::TY2, W>), gr, b, 0, s, A); } while (0)
    switch (A.scheme) {
        case 1: CSI_ADV_STAGE(1, false); break;
        case 3: CSI_ADV_STAGE(3, W32); break;
        case -3: CSI_ADV_STAGE(-3, false); break;
        case 5: CSI_ADV_STAGE(5, W32); break;
        case -5: CSI_ADV_STAGE(-5, false); break;
        default: CSI_ADV_STAGE(7, W32); break;
    }
#undef CSI_ADV_STAGE
    return AdvLayout{two ? 2 : 1, tx, ty};
}
// one RK stage of an advection-only model without snow: tendencies of (A.h, A.a), update A.hb + dt G -> A.ho (A.ab, A.ao)
AdvLayout launch_advect_stage(const AdvDev& A, int mode, hipStream_t s) {
    if (A.w32) return mode == 1 ? launch_stage_mode<true, true>(A, s) : launch_stage_mode<false, true>(A, s);
    return mode == 1 ? launch_stage_mode<true, false>(A, s) : launch_stage_mode<false, false>(A, s);
}
void launch_tracer_step(const AdvDev& A, hipStream_t s) {
    dim3 b(64, 4);
    hipLaunchKernelGGL(adv::k_tracer_step, dim3((unsigned)((A.g.Nx + 63) / 64), (unsigned)((A.g.Ny + 3) / 4)), b, 0, s, A);
}

}  // namespace csi
