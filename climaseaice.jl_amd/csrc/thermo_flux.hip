// thermo_flux.hip -- the slab and layered thermodynamic steps with per-cell heat fluxes, RadiativeEmission, the LINEAR top term, the
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

// getflux of one term at surface temperature T; q: the cell's value of the side's ARRAY term.  EMIT / LIN: the side has a term that
// depends on T -- RadiativeEmission / the LINEAR term (K * (T - Ta)) * w, in this order
template <bool EMIT, int LIN>
__device__ __forceinline__ double flux_term(const FluxTermsDev& t, int k, double q, double T, const LinCell& lc) {
    if (EMIT && t.kind[k] == FLUX_EMISSION) return t.eps[k] * t.sigma[k] * pow4(T + t.Tr[k]);
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
template <bool EMIT, int LIN>
__device__ __forceinline__ double flux_sum(const FluxTermsDev& t, double q, double T, const LinCell& lc) {
    double acc = 0.0;
#pragma unroll
    for (int k = kMaxFluxTerms - 1; k >= 0; --k) {
        if (k < t.n) {
            const double v = flux_term<EMIT, LIN>(t, k, q, T, lc);
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
// SB: the bottom salinity is read per cell.  The last two default to "off": those instantiations are the kernels of before.
template <bool QT, bool QB, bool EMIT, bool LTU, int LIN = LIN_NONE, bool SB = false>
__global__ void __launch_bounds__(256) k_slab_flux(SlabDev s, HeatFluxDev F, FluxFields ff, GridDev g, FRef h, FRef a, FRef mf, int has_mf,
                                                   double dt) {
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const double hn = h(i, j), an = a(i, j);
    const double tum = LTU ? ff.tu(i, j) : 0.0;
    const double qt = QT ? ff.qtop(i, j) : 0.0;
    const double qb = QB ? ff.qbot(i, j) : 0.0;
    const LinCell lc{LIN == LIN_ARRAYS ? ff.lin_k(i, j) : 0.0, LIN == LIN_ARRAYS ? ff.lin_ta(i, j) : 0.0, an, F.lin_weight};
    const double Sb = SB ? ff.sbot(i, j) : s.S;
    const double hc = s.hc;
    const bool consolidated = hn >= hc;
    const double Tb = s.liq_T0 - s.liq_slope * Sb;
    auto Qx = [&](double T) { return F.top.n ? flux_sum<EMIT, LIN>(F.top, qt, T, lc) : s.Qu; };
    double Tu = s.Tu;
    if (s.top_bc_kind == 1) {      // MeltingConstrainedFluxBalance: root of Qx - Qi(T), capped at Tm(S_ice); thin slab: Tb
        const double Tm = s.liq_T0 - s.liq_slope * s.ice_salinity;
        double root = Tb;
        if (consolidated) {
            if ((EMIT || LIN != LIN_NONE) && LTU) {      // (the host sets LTU whenever the flux balance has a term that depends on T)
                auto f = [&](double T) { return Qx(T) - ((hn <= 0) ? 0.0 : -s.k * (T - Tb) / hn); };
                root = secant_root(f, tum, F.tol, F.maxiters);
            } else {
                root = Tb - Qx(0.0) * hn / s.k;      // Qx does not depend on T: the closed form of the numeric path
            }
        }
        Tu = consolidated ? jmin(root, Tm) : Tb;
    } else if (LTU) {              // PrescribedTemperature per cell
        Tu = tum;
    }
    const double Eb = s.rho_bulk * latent_heat(s, Tb);
    const double Eu = s.rho_bulk * latent_heat(s, Tu);
    const double Qi_fun = (hn <= 0) ? 0.0 : -s.k * (Tu - Tb) / hn;
    const double Qu = (s.top_flux_kind == 1) ? Qi_fun : Qx(Tu);
    const double Qb = (s.bot_flux_kind == 1) ? (-(1 - an)) * s.Qb : (F.bot.n ? flux_sum<false, LIN_NONE>(F.bot, qb, Tu, lc) : s.Qb);
    const double Qi = consolidated ? Qi_fun : 0.0;
    const double wu = (Qu - Qi) / Eu;
    const double wb = (Qi - Qb) / Eb;
    double h1, a1;
    ice_volume_update(wu + wb, hn, an, hc, dt, h1, a1);
    a(i, j) = a1;
    h(i, j) = h1;
    if (has_mf) mf(i, j) = s.rho_bulk * (h1 * a1 - hn * an) / dt;
    if (s.top_bc_kind == 1 && ff.tu.p) ff.tu(i, j) = Tu;
    if (ff.qtop_used.p) ff.qtop_used(i, j) = Qu;
    if (ff.qbot_used.p) ff.qbot_used(i, j) = Qb;
}

// PS: per-cell snowfall
template <bool QT, bool QB, bool EMIT, bool LTU, bool PS, int LIN = LIN_NONE, bool SB = false>
__global__ void __launch_bounds__(256) k_layered_flux(SlabDev s, SnowDev w, HeatFluxDev F, FluxFields ff, GridDev g, FRef h, FRef a, FRef hs,
                                                      LayeredOut o, double dt) {
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
    const double hc = s.hc;
    const double Vin = hin * an, Vsn = hsn * an;
    const bool consolidated = hin >= hc;
    const double Tb = s.liq_T0 - s.liq_slope * Sb;
    double Tm = s.liq_T0 - s.liq_slope * s.ice_salinity;
    const double ks = w.k, ki = s.k;
    auto Qx = [&](double T) { return F.top.n ? flux_sum<EMIT, LIN>(F.top, qt, T, lc) : s.Qu; };
    Tm = (hsn > 0) ? 0.0 : Tm;
    const double R = hsn / ks + hin / ki;
    double Tus = w.Tu;
    if (w.top_bc_kind == 1) {
        double root = Tb;
        if (consolidated) {
            if ((EMIT || LIN != LIN_NONE) && LTU) {      // (the host sets LTU whenever the flux balance has a term that depends on T)
                auto f = [&](double T) { return Qx(T) - ((R <= 0) ? 0.0 : (Tb - T) / R); };
                root = secant_root(f, tum, F.tol, F.maxiters);
            } else {
                root = Tb - Qx(0.0) * R;
            }
        }
        Tus = consolidated ? jmin(root, Tm) : Tb;
    } else if (LTU) {
        Tus = tum;
    }
    const double Ri = hin / ki, Rs = hsn / ks, Rt = Rs + Ri;
    const double Tsi = (Rt <= 0) ? Tb : Tb + (Tus - Tb) * Ri / Rt;
    const double Qic = (R <= 0) ? 0.0 : (Tb - Tus) / R;
    const double Qis = consolidated ? Qic : 0.0;
    const double Qui = Qx(Tus);
    const double Qui_per_ice = (an > 0) ? Qui / an : 0.0;
    const double dQ = Qui_per_ice - Qis;
    const double melt_energy = jmax(0.0, -dQ);
    const double rs = w.rho, Ls = s.L0;
    const double cap = rs * Ls * hsn / dt;
    const double Qs = jmin(melt_energy, cap);
    const double Gsm = Qs / (rs * Ls);
    const double ri = s.rho_bulk, riL = ri * Ls;
    const double Qbi = (s.bot_flux_kind == 1) ? (-(1 - an)) * s.Qb : (F.bot.n ? flux_sum<false, LIN_NONE>(F.bot, qb, Tus, lc) : s.Qb);
    const double alpha = (Qui - Qbi) / riL, beta = Qs / riL;
    const double Cm = (hin > 0) ? an / (2 * hin) : 0.0;
    const double Cf = (hc > 0) ? (1 - an) / hc : 0.0;
    const double Km = dt * Cm, Kf = dt * Cf;
    const double eps = 2.220446049250313e-16;
    const double Dm = 1 - Km * beta, Df = 1 - Kf * beta;
    const double am = (fabs(Dm) > eps) ? (an + Km * alpha) / Dm : an + Km * alpha;
    const double af = (fabs(Df) > eps) ? (an + Kf * alpha) / Df : an + Kf * alpha;
    const double dtVm = alpha + beta * am;
    const bool melting = dtVm < 0;
    const double atmp = melting ? am : af;
    const double Qeff = Qui + Qs * atmp;
    const double Eb = ri * latent_heat(s, Tb), Eu = ri * latent_heat(s, Tsi);
    const double Qii_fun = (hin <= 0) ? 0.0 : -ki * (Tsi - Tb) / hin;
    const double Qii = consolidated ? Qii_fun : 0.0;
    const double wu = (Qeff - Qii) / Eu, wb = (Qii - Qbi) / Eb;
    double hi1, a1;
    ice_volume_update(wu + wb, hin, an, hc, dt, hi1, a1);
    hsn = (a1 > 0) ? hsn * an / a1 : 0.0;
    const double Gsp = (a1 > 0) ? Ps / rs : 0.0;
    double hs1 = hsn + dt * (Gsp - Gsm);
    hs1 = jmax(0.0, hs1);
    {
        const double rw = s.rho_l;
        const double hf = hi1 * (1 - ri / rw) - hs1 * rs / rw;
        double dhs = (hf < 0) ? -hf * ri / rs : 0.0;
        const double hsp = jmax(0.0, hs1 - dhs);
        dhs = hs1 - hsp;
        hi1 = hi1 + dhs * rs / ri;
        hs1 = hsp;
    }
    hs1 = (a1 <= 0) ? 0.0 : hs1;
    a(i, j) = a1; h(i, j) = hi1; hs(i, j) = hs1;
    const double Pabs = rs * Gsp * a1;
    if (o.mf_ice.p) o.mf_ice(i, j) = ri * (hi1 * a1 - Vin) / dt;
    if (o.mf_snow.p) o.mf_snow(i, j) = rs * (hs1 * a1 - Vsn) / dt - Pabs;
    if (o.mf_int.p) o.mf_int(i, j) = Pabs;
    if (o.tu_ice.p) o.tu_ice(i, j) = Tsi;
    if (o.tu_snow.p) o.tu_snow(i, j) = Tus;
    if (ff.qtop_used.p) ff.qtop_used(i, j) = Qui;
    if (ff.qbot_used.p) ff.qbot_used(i, j) = Qbi;
}

bool flux_has_emission(const FluxTermsDev& t) {
    for (int k = 0; k < t.n; ++k)
        if (t.kind[k] == FLUX_EMISSION) return true;
    return false;
}

namespace {
constexpr int kBlockX = 64, kBlockY = 4;
dim3 cells(const GridDev& g) { return dim3((unsigned)((g.Nx + kBlockX - 1) / kBlockX), (unsigned)((g.Ny + kBlockY - 1) / kBlockY)); }

using SlabFn = void (*)(const SlabDev&, const HeatFluxDev&, const FluxFields&, const GridDev&, const FRef&, const FRef&, const FRef&, int,
                        double, hipStream_t);
template <int B>
void slab_inst(const SlabDev& S, const HeatFluxDev& F, const FluxFields& ff, const GridDev& g, const FRef& h, const FRef& a, const FRef& mf,
               int has_mf, double dt, hipStream_t st) {
    hipLaunchKernelGGL((k_slab_flux<(B & 1) != 0, (B & 2) != 0, (B & 4) != 0, (B & 8) != 0, (B / 16) % 3, (B / 48) != 0>), cells(g),
                       dim3(kBlockX, kBlockY), 0, st, S, F, ff, g, h, a, mf, has_mf, dt);
}
template <int... B>
constexpr SlabFn slab_table_entry(int b, std::integer_sequence<int, B...>) {
    constexpr SlabFn t[] = {&slab_inst<B>...};
    return t[b];
}

using LayeredFn = void (*)(const SlabDev&, const SnowDev&, const HeatFluxDev&, const FluxFields&, const GridDev&, const FRef&, const FRef&,
                           const FRef&, const LayeredOut&, double, hipStream_t);
template <int B>
void layered_inst(const SlabDev& S, const SnowDev& W, const HeatFluxDev& F, const FluxFields& ff, const GridDev& g, const FRef& h,
                  const FRef& a, const FRef& hs, const LayeredOut& o, double dt, hipStream_t st) {
    hipLaunchKernelGGL((k_layered_flux<(B & 1) != 0, (B & 2) != 0, (B & 4) != 0, (B & 8) != 0, (B & 16) != 0, (B / 32) % 3, (B / 96) != 0>),
                       cells(g), dim3(kBlockX, kBlockY), 0, st, S, W, F, ff, g, h, a, hs, o, dt);
}
template <int... B>
constexpr LayeredFn layered_table_entry(int b, std::integer_sequence<int, B...>) {
    constexpr LayeredFn t[] = {&layered_inst<B>...};
    return t[b];
}

// template bits shared by both steps: which per-cell arrays a configuration reads
int flux_bits(const HeatFluxDev& F, const FluxFields& ff, int top_bc_kind) {
    const bool emit = flux_has_emission(F.top);
    const bool ltu = (top_bc_kind == 0 && F.prescribed_array) || (top_bc_kind == 1 && (emit || F.lin != LIN_NONE));
    return (ff.qtop.p ? 1 : 0) | (ff.qbot.p ? 2 : 0) | (emit ? 4 : 0) | (ltu ? 8 : 0);
}
// the variants beyond them: the LINEAR term's three states, times the per-cell bottom salinity (6 per combination of bits)
int flux_variant(const HeatFluxDev& F) { return F.lin + 3 * (F.bottom_salinity_array ? 1 : 0); }
}  // namespace

void launch_slab_flux_step(const SlabDev& S, const HeatFluxDev& F, const FluxFields& ff, const GridDev& g, const FRef& h, const FRef& a,
                           const FRef& mf, int has_mf, double dt, hipStream_t s) {
    const int b = flux_bits(F, ff, S.top_bc_kind) + 16 * flux_variant(F);
    slab_table_entry(b, std::make_integer_sequence<int, 16 * 6>{})(S, F, ff, g, h, a, mf, has_mf, dt, s);
}

void launch_layered_flux_step(const SlabDev& S, const SnowDev& W, const HeatFluxDev& F, const FluxFields& ff, const GridDev& g,
                              const FRef& h, const FRef& a, const FRef& hs, const LayeredOut& o, double dt, hipStream_t s) {
    const int b = (flux_bits(F, ff, W.top_bc_kind) | (F.snowfall_array ? 16 : 0)) + 32 * flux_variant(F);
    layered_table_entry(b, std::make_integer_sequence<int, 32 * 6>{})(S, W, F, ff, g, h, a, hs, o, dt, s);
}

}  // namespace csi
