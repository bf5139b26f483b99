// thermo_flux.hip -- the slab and layered thermodynamic steps with per-cell heat fluxes, RadiativeEmission, the LINEAR top term, the
// SHORTWAVE top term with its stepped albedo (csi_shortwave_set), the
// surface-temperature solve, a per-cell bottom salinity and the used-flux outputs (include/csi.h, csi_heat_fluxes_set).  The numeric
// configuration keeps k_slab / k_layered (thermo.hip); these kernels run once a side has flux terms, the prescribed temperature, the
// snowfall or the bottom salinity is an array, or a used-flux output is bound.
//
//   getflux of a Number / array / Tuple / RadiativeEmission   HeatBoundaryConditions/boundary_fluxes.jl:8-22, 98-127
//   thermodynamic_tendency with the surface solve            slab_thermodynamics_tendencies.jl:74-135
//   top_surface_temperature (secant)                          HeatBoundaryConditions/top_heat_boundary_conditions.jl:82-100
//   _layered_thermodynamic_time_step!                         thermodynamic_time_step.jl:131-298
// Per-cell, no stencil.  Compiled with -ffp-contract=off, the reference's expression order (STRICT and FAST alike).
// Every load of a cell is issued before the first use; the template flags select which loads exist, so
// a configuration pays only for the arrays it reads.
#include <utility>

#include "csi_dev.h"
#include "csi_kernels.h"
#include "thermo_dev.h"

namespace csi {

// (T + T_r)^4 as (x * x) * (x * x): Julia's Float64 ^ 4 is a compensated power (include/csi.h)
__device__ __forceinline__ double pow4(double x) {
    const double x2 = x * x;
    return x2 * x2;
}

// what the LINEAR term reads of a cell: K and Ta (LIN_ARRAYS; the term's numbers otherwise), the concentration the step starts from
// and the weighting
struct LinCell {
    double K, Ta, a;
    int w;
};

// what the SHORTWAVE term reads of a cell: F (SW_CELL; the setting's number otherwise), the albedo triple that holds in the cell (the
// snow triple where the layered step starts with hs > 0), the concentration the step starts from and the weighting
struct SwCell {
    double F, cold, warm, thr, a;
    int w;
};
__device__ __forceinline__ double albedo(const SwCell& sc, double T) { return (T < sc.thr) ? sc.cold : sc.warm; }

// getflux of one term at surface temperature T; q: the cell's value of the side's ARRAY term.  EMIT / LIN / SW: the side has a term that
// depends on T -- RadiativeEmission / the LINEAR term (K * (T - Ta)) * w / the SHORTWAVE term (F * (1 - alpha(T))) * w, in this order
template <bool EMIT, int LIN, int SW>
__device__ __forceinline__ double flux_term(const FluxTermsDev& t, int k, double q, double T, const LinCell& lc, const SwCell& sc) {
    if (EMIT && t.kind[k] == FLUX_EMISSION) return t.eps[k] * t.sigma[k] * pow4(T + t.Tr[k]);
    if (SW != SW_NONE && t.kind[k] == FLUX_SHORTWAVE) {
        const double v = sc.F * (1 - albedo(sc, T));
        if (sc.w == WEIGHT_CONCENTRATION) return v * sc.a;
        if (sc.w == WEIGHT_ICE_PRESENT) return (sc.a == 0) ? 0.0 : v;
        return v;
    }
    if (LIN != LIN_NONE && t.kind[k] == FLUX_LINEAR) {
        const double K = (LIN == LIN_ARRAYS) ? lc.K : t.value[k], Ta = (LIN == LIN_ARRAYS) ? lc.Ta : t.Tr[k];
        const double v = K * (T - Ta);
        if (lc.w == WEIGHT_CONCENTRATION) return v * lc.a;
        if (lc.w == WEIGHT_ICE_PRESENT) return (lc.a == 0) ? 0.0 : v;
        return v;
    }
    return t.kind[k] == FLUX_ARRAY ? q : t.value[k];
}

// getflux of the side's Tuple: t0 + (t1 + (... + t_{n-1})), right-nested (boundary_fluxes.jl:15-22); n >= 1.  Unrolled over the
// fixed capacity so that every term index is a constant (no dynamically indexed kernel argument).
template <bool EMIT, int LIN, int SW>
__device__ __forceinline__ double flux_sum(const FluxTermsDev& t, double q, double T, const LinCell& lc, const SwCell& sc) {
    double acc = 0.0;
#pragma unroll
    for (int k = kMaxFluxTerms - 1; k >= 0; --k) {
        if (k < t.n) {
            const double v = flux_term<EMIT, LIN, SW>(t, k, q, T, lc, sc);
            acc = (k == t.n - 1) ? v : v + acc;
        }
    }
    return acc;
}

// The SHORTWAVE instantiations keep the top's terms in vector registers.  A side's FluxTermsDev is 68 scalar registers of kernel
// argument, and all of it is live across the secant loop: with the shortwave setting on top that no longer fits the 102 scalar registers
// a wave has.  So before the loop each term is reduced to the two numbers its value needs -- A, B: CONSTANT / ARRAY the value, -;
// EMISSION eps * sigma (the product the term forms first anyway), T_r; LINEAR K, Ta -- and an empty asm with a "v" constraint keeps
// them (and the cell's shortwave numbers) in vector registers, of which these kernels have plenty.  Only kind[] and n stay scalar.
__device__ __forceinline__ double in_vgpr(double x) {
    asm("" : "+v"(x));
    return x;
}
// ... and what the step needs only after the loop -- the bottom's external flux, which does not depend on the surface temperature, and
// the latent heat's numbers -- is formed BEFORE it (a volatile asm is not moved across the loop), so that the scalar registers those
// kernel arguments arrive in are free while the loop runs.  The values and the order of their arithmetic are flux_sum's and latent_heat's.
__device__ __forceinline__ double before_loop(double x) {
    asm volatile("" : "+v"(x));
    return x;
}
struct LatentRegs {
    double L0, c, T0, rho;
};
__device__ __forceinline__ LatentRegs load_latent(const SlabDev& s) {
    return LatentRegs{before_loop(s.L0), before_loop(s.rho_l * s.c_l / s.rho_pure - s.c_i), before_loop(s.T0), before_loop(s.rho_bulk)};
}
__device__ __forceinline__ double latent_heat(const LatentRegs& l, double T) { return l.L0 + l.c * (T - l.T0); }
struct TermRegs {
    double A[kMaxFluxTerms], B[kMaxFluxTerms];
};
template <bool EMIT, int LIN>
__device__ __forceinline__ void load_terms(TermRegs& r, const FluxTermsDev& t, double q, const LinCell& lc) {
#pragma unroll
    for (int k = 0; k < kMaxFluxTerms; ++k) {
        double A = t.value[k], B = t.Tr[k];
        if (EMIT && t.kind[k] == FLUX_EMISSION) A = t.eps[k] * t.sigma[k];
        if (t.kind[k] == FLUX_ARRAY) A = q;
        if (LIN == LIN_ARRAYS && t.kind[k] == FLUX_LINEAR) { A = lc.K; B = lc.Ta; }
        r.A[k] = in_vgpr(A);
        r.B[k] = in_vgpr(B);
    }
}
// flux_term / flux_sum on those registers: the same values in the same order
template <bool EMIT, int LIN, int SW>
__device__ __forceinline__ double flux_sum_regs(const FluxTermsDev& t, const TermRegs& r, double T, const LinCell& lc, const SwCell& sc) {
    double acc = 0.0;
#pragma unroll
    for (int k = kMaxFluxTerms - 1; k >= 0; --k) {
        if (k < t.n) {
            double v = r.A[k];
            if (EMIT && t.kind[k] == FLUX_EMISSION) {
                v = r.A[k] * pow4(T + r.B[k]);
            } else if (SW != SW_NONE && t.kind[k] == FLUX_SHORTWAVE) {
                v = sc.F * (1 - albedo(sc, T));
                if (sc.w == WEIGHT_CONCENTRATION) v = v * sc.a;
                if (sc.w == WEIGHT_ICE_PRESENT) v = (sc.a == 0) ? 0.0 : v;
            } else if (LIN != LIN_NONE && t.kind[k] == FLUX_LINEAR) {
                v = r.A[k] * (T - r.B[k]);
                if (lc.w == WEIGHT_CONCENTRATION) v = v * lc.a;
                if (lc.w == WEIGHT_ICE_PRESENT) v = (lc.a == 0) ? 0.0 : v;
            }
            acc = (k == t.n - 1) ? v : v + acc;
        }
    }
    return acc;
}

// find_zero(f, SecantMethod(Tu- + 1, Tu-), CompactSolution()) as recalled in include/csi.h: at most maxiters updates, the last
// iterate is the root whether or not it converged.  Lanes leave the loop at different iterations; nothing is stored inside it.
template <class Fn>
__device__ __forceinline__ double secant_root(const Fn& f, double Tu_prev, double tol, int maxiters) {
    double x0 = Tu_prev + 1, x1 = Tu_prev;
    double y0 = f(x0), y1 = f(x1);
    for (int it = 0; it < maxiters; ++it) {
        const double dx = x1 - x0, dy = y1 - y0;
        x0 = x1;
        y0 = y1;
        x1 = x1 - y1 * dx / dy;
        y1 = f(x1);
        if (fabs(x1 - x0) < tol) break;
    }
    return x1;
}

// QT / QB: the top / bottom side has an ARRAY term; EMIT: the top has a RadiativeEmission term; LTU: the cell's surface temperature
// is read (Tu- of the secant, or the prescribed per-cell value); LIN: the top's LINEAR term (LIN_NONE / LIN_NUMBERS / LIN_ARRAYS);
// SB: the bottom salinity is read per cell; SW: the top's SHORTWAVE term (SW_NONE / SW_NUMBER / SW_CELL), whose setting is the last
// argument -- a parameter pack that is empty for SW_NONE and one ShortwaveDev otherwise, so that the SW_NONE instantiations have the
// argument list, and with it the code, of before.  The last three flags default to "off".
__device__ __forceinline__ ShortwaveDev shortwave_arg() { return ShortwaveDev{}; }
__device__ __forceinline__ const ShortwaveDev& shortwave_arg(const ShortwaveDev& sw) { return sw; }

template <bool QT, bool QB, bool EMIT, bool LTU, int LIN = LIN_NONE, bool SB = false, int SW = SW_NONE, class... SwArg>
__global__ void __launch_bounds__(256) k_slab_flux(SlabDev s, HeatFluxDev F, FluxFields ff, GridDev g, FRef h, FRef a, FRef mf, int has_mf,
                                                   double dt, SwArg... sw_arg) {
    static_assert(sizeof...(SwArg) == (SW == SW_NONE ? 0 : 1), "the shortwave setting travels exactly when there is a term");
    const ShortwaveDev& sw = shortwave_arg(sw_arg...);
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const double hn = h(i, j), an = a(i, j);
    const double tum = LTU ? ff.tu(i, j) : 0.0;
    const double qt = QT ? ff.qtop(i, j) : 0.0;
    const double qb = QB ? ff.qbot(i, j) : 0.0;
    const LinCell lc{LIN == LIN_ARRAYS ? ff.lin_k(i, j) : 0.0, LIN == LIN_ARRAYS ? ff.lin_ta(i, j) : 0.0, an, F.lin_weight};
    const double Sb = SB ? ff.sbot(i, j) : s.S;
    const double fsw = SW == SW_CELL ? sw.f(i, j) : (SW == SW_NUMBER ? sw.F : 0.0);
    const SwCell sc = SW == SW_NONE ? SwCell{} : SwCell{in_vgpr(fsw), in_vgpr(sw.cold), in_vgpr(sw.warm), in_vgpr(sw.thr), an, sw.weight};
    const double hc = (SW != SW_NONE) ? in_vgpr(s.hc) : s.hc;
    const bool consolidated = hn >= hc;
    const double Tb = s.liq_T0 - s.liq_slope * Sb;
    auto Qb_ext = [&](double T) {
        return (s.bot_flux_kind == 1) ? (-(1 - an)) * s.Qb : (F.bot.n ? flux_sum<false, LIN_NONE, SW_NONE>(F.bot, qb, T, lc, sc) : s.Qb);
    };
    TermRegs tr;
    LatentRegs lr;
    double Qb_pre = 0.0;
    if constexpr (SW != SW_NONE) {
        load_terms<EMIT, LIN>(tr, F.top, qt, lc);
        lr = load_latent(s);
        Qb_pre = before_loop(Qb_ext(0.0));
    }
    auto Qx = [&](double T) {
        if constexpr (SW != SW_NONE) return flux_sum_regs<EMIT, LIN, SW>(F.top, tr, T, lc, sc);      // (the term is in the tuple: n >= 1)
        else return F.top.n ? flux_sum<EMIT, LIN, SW>(F.top, qt, T, lc, sc) : s.Qu;
    };
    double Tu = s.Tu;
    if (s.top_bc_kind == 1) {      // MeltingConstrainedFluxBalance: root of Qx - Qi(T), capped at Tm(S_ice); thin slab: Tb
        const double Tm = s.liq_T0 - s.liq_slope * s.ice_salinity;
        double root = Tb;
        if (consolidated) {
            if ((EMIT || LIN != LIN_NONE || SW != SW_NONE) && LTU) {      // (the host sets LTU whenever the flux balance has a term that depends on T)
                auto f = [&](double T) { return Qx(T) - ((hn <= 0) ? 0.0 : -s.k * (T - Tb) / hn); };
                root = secant_root(f, tum, (SW != SW_NONE) ? in_vgpr(F.tol) : F.tol, F.maxiters);
            } else {
                root = Tb - Qx(0.0) * hn / s.k;      // Qx does not depend on T: the closed form of the numeric path
            }
        }
        Tu = consolidated ? jmin(root, Tm) : Tb;
    } else if (LTU) {              // PrescribedTemperature per cell
        Tu = tum;
    }
    // (what follows the loop reads the copies made before it in the SHORTWAVE instantiations, the arguments themselves otherwise)
    auto E = [&](double T) {
        if constexpr (SW != SW_NONE) return lr.rho * latent_heat(lr, T);
        else return s.rho_bulk * latent_heat(s, T);
    };
    auto Qb = [&](double T) {
        if constexpr (SW != SW_NONE) return Qb_pre;
        else return Qb_ext(T);
    };
    const UsedFluxes used = slab_from_surface(s, i, j, h, a, mf, has_mf, hn, an, hc, dt, Tb, Tu, E, Qx, Qb);
    if (s.top_bc_kind == 1 && ff.tu.p) ff.tu(i, j) = Tu;
    if (ff.qtop_used.p) ff.qtop_used(i, j) = used.top;
    if (ff.qbot_used.p) ff.qbot_used(i, j) = used.bottom;
    if (SW != SW_NONE && sw.albedo_used.p) sw.albedo_used(i, j) = albedo(sc, Tu);
}

// PS: per-cell snowfall
template <bool QT, bool QB, bool EMIT, bool LTU, bool PS, int LIN = LIN_NONE, bool SB = false, int SW = SW_NONE, class... SwArg>
__global__ void __launch_bounds__(256) k_layered_flux(SlabDev s, SnowDev w, HeatFluxDev F, FluxFields ff, GridDev g, FRef h, FRef a, FRef hs,
                                                      LayeredOut o, double dt, SwArg... sw_arg) {
    static_assert(sizeof...(SwArg) == (SW == SW_NONE ? 0 : 1), "the shortwave setting travels exactly when there is a term");
    const ShortwaveDev& sw = shortwave_arg(sw_arg...);
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const double hin = h(i, j), an = a(i, j);
    double hsn = hs(i, j);
    const double tum = LTU ? ff.tu(i, j) : 0.0;
    const double qt = QT ? ff.qtop(i, j) : 0.0;
    const double qb = QB ? ff.qbot(i, j) : 0.0;
    const double Ps = PS ? ff.snowfall(i, j) : w.snowfall;
    const LinCell lc{LIN == LIN_ARRAYS ? ff.lin_k(i, j) : 0.0, LIN == LIN_ARRAYS ? ff.lin_ta(i, j) : 0.0, an, F.lin_weight};
    const double Sb = SB ? ff.sbot(i, j) : s.S;
    const double fsw = SW == SW_CELL ? sw.f(i, j) : (SW == SW_NUMBER ? sw.F : 0.0);
    const bool snowy = SW != SW_NONE && sw.snow_pair && hsn > 0;      // (the condition under which Tm = 0 below)
    const SwCell sc = SW == SW_NONE ? SwCell{}
                                    : SwCell{in_vgpr(fsw), snowy ? sw.snow_cold : sw.cold, snowy ? sw.snow_warm : sw.warm,
                                             snowy ? sw.snow_thr : sw.thr, an, sw.weight};
    const double hc = (SW != SW_NONE) ? in_vgpr(s.hc) : s.hc;
    const bool consolidated = hin >= hc;
    const double Tb = s.liq_T0 - s.liq_slope * Sb;
    double Tm = s.liq_T0 - s.liq_slope * s.ice_salinity;
    const double ks = w.k, ki = s.k;
    auto Qb_ext = [&](double T) {
        return (s.bot_flux_kind == 1) ? (-(1 - an)) * s.Qb : (F.bot.n ? flux_sum<false, LIN_NONE, SW_NONE>(F.bot, qb, T, lc, sc) : s.Qb);
    };
    // what the step reads from the surface temperature on: the arguments themselves, or in the SHORTWAVE instantiations copies made
    // before the loop
    TermRegs tr;
    LatentRegs lr;
    double Qb_pre = 0.0;
    LayeredNums n{w.rho, s.rho_l, ki, dt, Ps, s.rho_bulk, s.L0, hc};
    if constexpr (SW != SW_NONE) {
        load_terms<EMIT, LIN>(tr, F.top, qt, lc);
        lr = load_latent(s);
        Qb_pre = before_loop(Qb_ext(0.0));
        n = LayeredNums{before_loop(w.rho), before_loop(s.rho_l), before_loop(ki), before_loop(dt), before_loop(Ps), lr.rho, lr.L0, hc};
    }
    auto Qx = [&](double T) {
        if constexpr (SW != SW_NONE) return flux_sum_regs<EMIT, LIN, SW>(F.top, tr, T, lc, sc);      // (the term is in the tuple: n >= 1)
        else return F.top.n ? flux_sum<EMIT, LIN, SW>(F.top, qt, T, lc, sc) : s.Qu;
    };
    Tm = (hsn > 0) ? 0.0 : Tm;
    const double Ri = hin / ki, Rs = hsn / ks, R = Rs + Ri;
    double Tus = w.Tu;
    if (w.top_bc_kind == 1) {
        double root = Tb;
        if (consolidated) {
            if ((EMIT || LIN != LIN_NONE || SW != SW_NONE) && LTU) {      // (the host sets LTU whenever the flux balance has a term that depends on T)
                auto f = [&](double T) { return Qx(T) - ((R <= 0) ? 0.0 : (Tb - T) / R); };
                root = secant_root(f, tum, (SW != SW_NONE) ? in_vgpr(F.tol) : F.tol, F.maxiters);
            } else {
                root = Tb - Qx(0.0) * R;
            }
        }
        Tus = consolidated ? jmin(root, Tm) : Tb;
    } else if (LTU) {
        Tus = tum;
    }
    auto latent = [&](double T) {
        if constexpr (SW != SW_NONE) return latent_heat(lr, T);
        else return latent_heat(s, T);
    };
    auto Qb = [&](double T) {
        if constexpr (SW != SW_NONE) return Qb_pre;
        else return Qb_ext(T);
    };
    const UsedFluxes used = layered_from_surface(n, i, j, h, a, hs, o, hin, an, hsn, Tb, Tus, Ri, R, latent, Qx, Qb);
    if (ff.qtop_used.p) ff.qtop_used(i, j) = used.top;
    if (ff.qbot_used.p) ff.qbot_used(i, j) = used.bottom;
    if (SW != SW_NONE && sw.albedo_used.p) sw.albedo_used(i, j) = albedo(sc, Tus);
}

// This source makes three objects (Makefile): CSI_FLUX_SW = 0 (thermo_flux.o: the kernels of before, the host's selection and the launch
// functions), 1 and 2 (thermo_flux_sw1.o / _sw2.o: the SW_NUMBER / SW_CELL instantiations), so that the three compile side by side.
#ifndef CSI_FLUX_SW
#define CSI_FLUX_SW 0
#endif

using SlabFn = void (*)(const SlabDev&, const HeatFluxDev&, const FluxFields&, const ShortwaveDev&, const GridDev&, const FRef&, const FRef&,
                        const FRef&, int, double, hipStream_t);
using LayeredFn = void (*)(const SlabDev&, const SnowDev&, const HeatFluxDev&, const FluxFields&, const ShortwaveDev&, const GridDev&,
                           const FRef&, const FRef&, const FRef&, const LayeredOut&, double, hipStream_t);
// the launcher of one instantiation: b = flux_bits + 16 (32 layered) * (LIN + 3 * SB); one specialisation per object
template <int SW> SlabFn slab_flux_entry(int b);
template <int SW> LayeredFn layered_flux_entry(int b);

namespace {
template <int B>
void slab_inst(const SlabDev& S, const HeatFluxDev& F, const FluxFields& ff, const ShortwaveDev& sw, const GridDev& g, const FRef& h,
               const FRef& a, const FRef& mf, int has_mf, double dt, hipStream_t st) {
#if CSI_FLUX_SW == 0
    hipLaunchKernelGGL((k_slab_flux<(B & 1) != 0, (B & 2) != 0, (B & 4) != 0, (B & 8) != 0, (B / 16) % 3, (B / 48) != 0>), thermo_grid(g),
                       thermo_block(), 0, st, S, F, ff, g, h, a, mf, has_mf, dt);
#else
    hipLaunchKernelGGL((k_slab_flux<(B & 1) != 0, (B & 2) != 0, (B & 4) != 0, (B & 8) != 0, (B / 16) % 3, (B / 48) != 0, CSI_FLUX_SW, ShortwaveDev>),
                       thermo_grid(g), thermo_block(), 0, st, S, F, ff, g, h, a, mf, has_mf, dt, sw);
#endif
}
template <int... B>
constexpr SlabFn slab_table_entry(int b, std::integer_sequence<int, B...>) {
    constexpr SlabFn t[] = {&slab_inst<B>...};
    return t[b];
}

template <int B>
void layered_inst(const SlabDev& S, const SnowDev& W, const HeatFluxDev& F, const FluxFields& ff, const ShortwaveDev& sw, const GridDev& g,
                  const FRef& h, const FRef& a, const FRef& hs, const LayeredOut& o, double dt, hipStream_t st) {
#if CSI_FLUX_SW == 0
    hipLaunchKernelGGL((k_layered_flux<(B & 1) != 0, (B & 2) != 0, (B & 4) != 0, (B & 8) != 0, (B & 16) != 0, (B / 32) % 3, (B / 96) != 0>),
                       thermo_grid(g), thermo_block(), 0, st, S, W, F, ff, g, h, a, hs, o, dt);
#else
    hipLaunchKernelGGL((k_layered_flux<(B & 1) != 0, (B & 2) != 0, (B & 4) != 0, (B & 8) != 0, (B & 16) != 0, (B / 32) % 3, (B / 96) != 0,
                                       CSI_FLUX_SW, ShortwaveDev>),
                       thermo_grid(g), thermo_block(), 0, st, S, W, F, ff, g, h, a, hs, o, dt, sw);
#endif
}
template <int... B>
constexpr LayeredFn layered_table_entry(int b, std::integer_sequence<int, B...>) {
    constexpr LayeredFn t[] = {&layered_inst<B>...};
    return t[b];
}
}  // namespace

template <> SlabFn slab_flux_entry<CSI_FLUX_SW>(int b) { return slab_table_entry(b, std::make_integer_sequence<int, 16 * 6>{}); }
template <> LayeredFn layered_flux_entry<CSI_FLUX_SW>(int b) { return layered_table_entry(b, std::make_integer_sequence<int, 32 * 6>{}); }

#if CSI_FLUX_SW == 0
template <> SlabFn slab_flux_entry<SW_NUMBER>(int b);
template <> SlabFn slab_flux_entry<SW_CELL>(int b);
template <> LayeredFn layered_flux_entry<SW_NUMBER>(int b);
template <> LayeredFn layered_flux_entry<SW_CELL>(int b);

bool flux_has_emission(const FluxTermsDev& t) {
    for (int k = 0; k < t.n; ++k)
        if (t.kind[k] == FLUX_EMISSION) return true;
    return false;
}

bool flux_reads_surface_temperature(const HeatFluxDev& F, int sw_mode, int top_bc_kind) {
    // PrescribedTemperature per cell, or Tu- of the secant: the flux balance has a term that depends on T
    return (top_bc_kind == 0 && F.prescribed_array) ||
           (top_bc_kind == 1 && (flux_has_emission(F.top) || F.lin != LIN_NONE || sw_mode != SW_NONE));
}

namespace {
// template bits shared by both steps: which per-cell arrays a configuration reads
int flux_bits(const HeatFluxDev& F, const FluxFields& ff, const ShortwaveDev& sw, int top_bc_kind) {
    return (ff.qtop.p ? 1 : 0) | (ff.qbot.p ? 2 : 0) | (flux_has_emission(F.top) ? 4 : 0) |
           (flux_reads_surface_temperature(F, sw.mode, top_bc_kind) ? 8 : 0);
}
// the variants beyond them: the LINEAR term's three states, times the per-cell bottom salinity (6 per combination of bits), in each
// of the SHORTWAVE term's three states.  Every one can be selected: with a SHORTWAVE term the flux balance always has LTU, and a
// PrescribedTemperature top has it exactly when the temperature is per cell.  tests/test_thermo_flux_matrix_table.py proves it --
// tests/thermo_flux_matrix.py restates this rule and builds a configuration for each of the 864 --, and tests/test_gpu_thermo_flux_matrix.py
// runs every one with the launch reported by csi_last_thermo.
int flux_variant(const HeatFluxDev& F) { return F.lin + 3 * (F.bottom_salinity_array ? 1 : 0); }
}  // namespace

ThermoLaunch launch_slab_flux_step(const SlabDev& S, const HeatFluxDev& F, const FluxFields& ff, const ShortwaveDev& sw, const GridDev& g,
                                   const FRef& h, const FRef& a, const FRef& mf, int has_mf, double dt, hipStream_t s) {
    const int b = flux_bits(F, ff, sw, S.top_bc_kind) + 16 * flux_variant(F);
    const int table = sw.mode == SW_CELL ? SW_CELL : (sw.mode == SW_NUMBER ? SW_NUMBER : SW_NONE);
    const SlabFn fn = table == SW_CELL ? slab_flux_entry<SW_CELL>(b) : (table == SW_NUMBER ? slab_flux_entry<SW_NUMBER>(b) : slab_flux_entry<SW_NONE>(b));
    fn(S, F, ff, sw, g, h, a, mf, has_mf, dt, s);
    return ThermoLaunch{3, table, b};
}

ThermoLaunch launch_layered_flux_step(const SlabDev& S, const SnowDev& W, const HeatFluxDev& F, const FluxFields& ff, const ShortwaveDev& sw,
                                      const GridDev& g, const FRef& h, const FRef& a, const FRef& hs, const LayeredOut& o, double dt,
                                      hipStream_t s) {
    const int b = (flux_bits(F, ff, sw, W.top_bc_kind) | (F.snowfall_array ? 16 : 0)) + 32 * flux_variant(F);
    const int table = sw.mode == SW_CELL ? SW_CELL : (sw.mode == SW_NUMBER ? SW_NUMBER : SW_NONE);
    const LayeredFn fn = table == SW_CELL ? layered_flux_entry<SW_CELL>(b)
                                          : (table == SW_NUMBER ? layered_flux_entry<SW_NUMBER>(b) : layered_flux_entry<SW_NONE>(b));
    fn(S, W, F, ff, sw, g, h, a, hs, o, dt, s);
    return ThermoLaunch{4, table, b};
}
#endif

}  // namespace csi
