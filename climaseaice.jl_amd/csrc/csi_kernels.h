// csi_kernels.h -- host-side launchers of the HIP kernels (one translation unit per kernel family).
#pragma once
#include "csi_dev.h"
#include "csi_fast_coef.h"

namespace csi {

// one thread per point of a Range in blocks of b: the thread's (i, j), and the grid that covers the range
#define CELL_OF_RANGE(r)                                                   \
    const int i = (r).i0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);   \
    const int j = (r).j0 + (int)(blockIdx.y * blockDim.y + threadIdx.y);   \
    if (i > (r).i1 || j > (r).j1) return;
static inline dim3 grid_for(const Range& r, dim3 b) {
    return dim3((unsigned)((r.i1 - r.i0 + 1 + b.x - 1) / b.x), (unsigned)((r.j1 - r.j0 + 1 + b.y - 1) / b.y), 1);
}

// STRICT mode: one kernel per reference @kernel (evp_strict.hip)
void launch_strict_init(const EvpDev& P, const Range& r, hipStream_t s);
void launch_strict_visc(const EvpDev& P, const Range& r, hipStream_t s);
void launch_strict_stress(const EvpDev& P, const Range& r, hipStream_t s);
void launch_strict_ustep(const EvpDev& P, const Range& r, const ImageSpec& im, hipStream_t s);
void launch_strict_vstep(const EvpDev& P, const Range& r, const ImageSpec& im, hipStream_t s);

// free-drift velocities of marginal ice (StressBalanceFreeDrift), once per sub-cycle, both modes (momentum_free_drift.hip)
void launch_free_drift(const EvpDev& P, const Range& r, hipStream_t s);
// StressBalanceFreeDrift as the model's dynamics (momentum_free_drift.hip): u and v over r, each with its halo images, in one launch
void launch_free_drift_step(const EvpDev& P, const Range& r, const ImageSpec& imu, const ImageSpec& imv, hipStream_t s);

// FAST mode (evp_fast.hip): fused viscosity + stress phase, u step, v step
void launch_fast_init(const EvpDev& P, const Range& r, hipStream_t s);
void launch_fast_stress(const EvpDev& P, const Range& r, const FastCoef& c, hipStream_t s);
void launch_fast_ustep(const EvpDev& P, const Range& r, const ImageSpec& im, const FastCoef& c, hipStream_t s);
void launch_fast_vstep(const EvpDev& P, const Range& r, const ImageSpec& im, const FastCoef& c, hipStream_t s);
// the fold band's launches (evp_fast.hip, k_band_stress / k_band_vel): inputs from P, outputs into other arrays.  stress: a, b, c take
// sigma11, sigma22, sigma12 and da, db, dc (may be null) rows >= j0 a second time; a velocity component: a (and da, rows >= j0).
struct BandOut { FRef a, b, c, da, db, dc; int j0; };
void launch_band_stress(const EvpDev& P, const Range& r, const FastCoef& c, const BandOut& o, hipStream_t s);
void launch_band_vel(const EvpDev& P, const Range& r, const ImageSpec& im, const FastCoef& c, bool u, const BandOut& o, hipStream_t s);
bool fast_supported(const EvpDev& P);

// fused sub-step (evp_fused.hip): stress + both velocities in one launch, double-buffered u, v, sigma.
// All uniform inputs live in a device table read through the constant address space.
// (order of use: adjacent entries are read by merged wide scalar loads)
enum : int { FK_EM2 = 0, FK_DMIN, FK_DMIN2, FK_AMIN2, FK_AMAX2, FK_HK1, FK_HKC, FK_HKF,      // stress phase
             FK_DT, FK_RDT, FK_MIN_MASS, FK_MIN_CONC, FK_RHO,                                     // velocity phases
             FK_DT2, FK_MIN_MASS2, FK_MIN_CONC2,      // 2 dt, 2 minimum_mass, 2 minimum_concentration (fm::vel_update_sum)
             FK_TOP_TAU_U, FK_TOP_TAU_V, FK_TOP_RHOCD, FK_TOP_UE, FK_TOP_VE,
             FK_BOT_TAU_U, FK_BOT_TAU_V, FK_BOT_RHOCD, FK_BOT_UE, FK_BOT_VE,
             FK_BCU, FK_BCV = FK_BCU + 2,      // ValueBoundaryCondition values: u at the y walls (low, high), v at the x walls
             FK_CA_DT = FK_BCV + 2, FK_RDMIN, FK_AMIN, FK_AMAX, FK_RAMIN, FK_RAMAX, FK_FCOR,
             FK_COEF0,
             FK_PCOEF0 = FK_COEF0 + FC_COUNT,      // the pair kernel's scaled copy of the uniform-grid coefficients (pair_coef_scale)
             FK_PK_EM2_8 = FK_PCOEF0 + FC_COUNT, FK_PK_DMIN2_16, FK_PK_HKF4, FK_PK_CA_DT4,      // e^-2 / 8, 16 Delta_min^2, 4 hkf, 4 x (c_alpha dt / 2): fm::stress_update_s
             FK_COUNT };
enum : int { FP_U_IN = 0, FP_V_IN, FP_S11_IN, FP_S22_IN, FP_S12_IN, FP_P, FP_H, FP_A, FP_UN, FP_VN,     // 10 inputs, contiguous
             FP_S11_OUT, FP_S22_OUT, FP_S12_OUT, FP_U_OUTP, FP_V_OUTP,                                // 5 outputs (parent addresses), contiguous
             FP_U_OUT, FP_V_OUT, FP_S11_OUT0, FP_S22_OUT0, FP_S12_OUT0,                               // (0,0)-offset addresses for stores with halo images
             FP_AL, FP_ZC, FP_ZF, FP_DL, FP_COEF_VEC, FP_PCOEF_VEC, FP_MASK,
             FP_FT_U, FP_FT_V, FP_FB_U, FP_FB_V, FP_FB_UBAR, FP_FB_VBAR, FP_FD_U, FP_FD_V,
             FP_FT_UBAR, FP_FT_VBAR,      // wind drag (a SemiImplicitStress on top with array-valued air velocities, in FP_FT_U / _V): their cross averages
             FP_FROW_U, FP_FROW_V,      // CSI_METRIC_FULL: per-row Coriolis parameter (device pointers, ptr[j] = row j)
             FP_F2U, FP_F2V,            // ... per-point Coriolis planes (parent addresses)
             FP_XC_U, FP_XC_V, FP_XD_U, FP_XD_V,   // EXTRA: model.forcing arrays; immersed-flux-BC stress divergence arrays (parent addresses)
             FP_C2_0,
             // halo images of the two-sub-steps kernel: for each of 9 arrays (sigma11, sigma22, sigma12, u, v, alpha, zeta_c, zeta_f, Delta)
             // and 8 directions (W E S N SW SE NW NE) the parent address of the array that receives the image -- the array itself
             // on untiled periodic sides and walls, the neighbouring tile's (mapped into this process) on peer-connected sides
             FP_IMG0 = FP_C2_0 + C2_COUNT,
             FP_SLOT_IN = FP_IMG0 + 72,     // peer flags: per direction, this rank's slots the neighbour there writes ...
             FP_SLOT_OUT = FP_SLOT_IN + 8,  // ... and that neighbour's slots this rank writes (device addresses)
             FP_PERR = FP_SLOT_OUT + 8,     // error word (a wait timed out)
             FP_ACT_LIVE,                   // tile activity (csi_activity.hip): device int array {live tiles, all tiles, list of the live tiles' numbers ...};
                                            // 0: every tile runs.  Read by launches whose write_diag has bit 2 set (run_fused: not the first two, not the last)
             FP_ACT_LIVE0,                  // ... the same for the FIRST TWO launches (write_diag bit 3): every tile but those that are quiescent from the
                                            // start -- u = v = +0.0 as well, no halo image to store --, 0: every tile runs
             FP_ROWPAD_ = FP_ACT_LIVE0 + (FP_C2_0 - FP_F2U),      // (room for FP_F2ROW_U / _V below FP_C2ROW_0)
             FP_C2ROW_0,                    // CSI_METRIC_FULL: the C2_COUNT planes as per-ROW vectors (ptr[parent row]), valid for the rows FP_RCSUM marks constant
             FP_F2ROW_U = FP_F2U + (FP_C2ROW_0 - FP_C2_0), FP_F2ROW_V,      // ... and the per-point Coriolis planes likewise (the SAME distance from FP_F2U / _V as the vectors from the planes: Stage::rcd_)
             FP_RCSUM = FP_C2ROW_0 + C2_COUNT,      // int prefix sums over parent rows: rcsum[t] = rows among parent rows [0, t) whose plane values are the same in every column (0: none marked)
             FP_COUNT };   // (FP_FT_* .. FP_FD_*: forcing arrays; FP_MASK: the uint8 mask; FP_C2_0 ..: the C2_COUNT per-point coefficient planes -- parent addresses)
enum : int { FI_NX = 0, FI_NY, FI_HX, FI_HY, FI_XLO, FI_XHI, FI_YLO, FI_YHI, FI_LD_C, FI_LD_F,
             FI_RS, FI_R1 = FI_RS + 4, FI_R1C = FI_R1 + 4, FI_R2 = FI_R1C + 4, FI_IMU = FI_R2 + 4, FI_IMV = FI_IMU + 4,
             FI_PRESSURE_KIND = FI_IMV + 4, FI_HAS_COR, FI_TOP_KIND, FI_BOT_KIND, FI_COEF_STRIDE, FI_COEF_JMIN, FI_COEF_JMAX,
             FI_DEC, FI_AJ0 = FI_DEC + 4, FI_AJ1, FI_IMS11, FI_IMS22 = FI_IMS11 + 4, FI_IMS12 = FI_IMS22 + 4, FI_MASK_LD = FI_IMS12 + 4, FI_BOT_UEK, FI_BOT_VEK, FI_FREE_DRIFT, FI_TOP_UEK, FI_TOP_VEK,
             FI_C2_LD, FI_FKIND,        // CSI_METRIC_FULL: leading dimension of the coefficient / Coriolis planes; f kind 0 number, 1 rows, 2 points
             FI_EXTRA,                  // EXTRA instantiations: bit 0 model.forcing arrays, bit 1 immersed flux boundary conditions
             FI_PEER,                   // 1: peer-connected sides (flags instead of a halo exchange, evp_fused2.hip)
             FI_PSET, FI_PMASK = FI_PSET + 4,   // tile sets next to the W / E / S / N side: strips, strips, chunks, chunks; directions with a neighbour
             FI_PWAIT,                  // slots to wait for per direction (= the size of the neighbour's opposite set)
             FI_PDLD = FI_PWAIT + 8,    // per direction x {Center in x, Face in x}: the neighbour's row stride minus this tile's, in bytes
             FI_PHASDLD = FI_PDLD + 16, // any of them non-zero (a Bounded x direction partitioned in x: the easternmost tile's Face fields are one column wider)
             FI_NYLO,                   // PEER: Ny of the neighbour beyond the LOW y side (rows of the image shift of this tile's low rows; a fold tile's own Ny is cut)
             FI_ELO, FI_EHI,            // rows of the first chunk / rows kept for the last chunk (0: `rows` / what is left): shorter tiles next to peer-connected y sides
             FI_WT,                     // 1: the pair kernel stores its results write-through (small grids: the launch does not end on a write-back of its dirty lines)
             FI_PTIER,                  // peer protocol tier (csi_set_peer_tier): 0 write-through images + drained stores + flags; 1: + a system-scope acquire
                                        // fence once the flags have been seen; 2: + a system-scope release fence before the flags are published
             FI_COUNT };
// peer flag arrays: slots per direction block; the LAST slot of a block is the abort word (a neighbour whose wait has given up sets
// it: this rank's waits stop at once)
constexpr int kPeerSlots = 1024;
struct FusedTable {
    double K[FK_COUNT];
    unsigned long P[FP_COUNT];
    int I[FI_COUNT + (FI_COUNT & 1)];
};
bool fused_supported(const EvpDev& P);
bool fused_supported_forcing(const EvpDev& P);   // everything but the mask restriction
void fused_fill_table(const EvpDev& P, const FastCoef& c, const FRef* in, const FRef* out,
                      const Range& rs, const Range& r1, const Range& r1c, const Range& r2,
                      const ImageSpec& imu, const ImageSpec& imv, FusedTable* host_table);
void launch_fused_substep(const FusedTable* dev_table, bool uniform, bool ufirst, int nstrips, int nchunks, int rows,
                          int write_diag, hipStream_t s);
// two sub-steps per launch (evp_fused2.hip); metric: 0 uniform coefficients, 1 per-row table, 2 per-point planes (CSI_METRIC_FULL).
// The table is one filled by fused_fill_table for the SECOND
// sub-step's store ranges (rs, r1, r2; r1c unused) plus: dec = the second sub-step's compute (stress) range that
// the wave tiles decompose, a_j0 / a_j1 = the first sub-step's stress rows, sigma image specs.
void fused_fill_pair_extra(const Range& dec, int a_j0, int a_j1, const ImageSpec& ims11, const ImageSpec& ims22,
                           const ImageSpec& ims12, FusedTable* host_table, int elo = 0, int ehi = 0, int write_through = 0);
// seq: launch number of the peer-flag protocol (0 on grids without peer-connected sides)
// extra: model.forcing arrays / immersed flux boundary conditions (the EXTRA instantiations; implies force)
// Tile activity (csi_activity.hip).  A tile of the two-sub-steps launch is QUIESCENT when the ice mass h rho aice is exactly zero in every cell
// of its owned box and one cell around it and no owned stress holds a negative zero: there sigma += (m > 0 ? ... : 0) and the velocity
// select's zero branch (elasto_visco_plastic_rheology.jl:343-347, split_explicit_momentum_equations.jl:217-228) make both sub-steps
// an exact fixed point of u, v, sigma -- every later launch would store what the launch two before it stored.  `act` receives
// {number of live tiles, number of tiles, the live tiles' numbers in ascending order}.
struct ActivityArgs {
    FRef h, a, s11, s22, s12, u, v;    // (0,0)-offset references; sigma, u, v: the CURRENT state
    double rho;
    Range dec;                         // the range the launch's tiles decompose (FI_DEC)
    int nstrips, nchunks, rows, elo, ehi;
    Range pc, pf;                      // index bounds of the Center-Center / Face-Face parents
    Range pu, pv;                      // ... of the u / v parents
    int Nx, Ny, Hx, Hy;                // the launch's grid: tiles within H of a side store halo images (never quiescent from the start)
    int pset[4], pmask;                // peer-connected launches (FI_PSET, FI_PMASK): the tiles of the direction sets wait for / publish flags
                                       // and store halo images into the neighbours' arrays -- always live
};
constexpr int kMaxActTiles = 16384;
// flags: 0 quiescent from the start (the first two launches may leave it out as well), 1 quiescent after two launches, 2 live.
// act / act0: {count, tiles, numbers ...} of the tiles with flag 2 / with flag >= 1.
// sample: device-visible pinned host words {seqlock, live, tiles, sample_id} the compaction writes for the host to read without an API call
void launch_tile_activity(const ActivityArgs& A, int* flags, int* act, int* act0, int* sample, int sample_id, hipStream_t s);
void launch_fused_pair(const FusedTable* dev_table, int metric, bool a_ufirst, bool walls, bool mask, bool force, bool free_drift, int extra,
                       int common_forcing, int nstrips, int nchunks, int rows, int write_diag, unsigned long long seq, hipStream_t s);
// stress divergence of the immersed FluxBoundaryConditions at every u / v point whose stencil stays inside the parents (evp_fast.hip)
void launch_immersed_div(const EvpDev& P, const FRef& xd_u, const FRef& xd_v, hipStream_t s);
// array-valued forcing the pair kernel takes: 0 none needed, 1 supported (FORCE variant), -1 not supported;
// free drift (P.free_drift non-zero -- StressBalanceFreeDrift or prescribed fields: the arrays P.ufd / P.vfd) also selects the FORCE variant
int pair_forcing_kind(const EvpDev& P);
bool evp_array_forcing(const EvpDev& P);
bool evp_ring_forcing(const EvpDev& P);
// bottom SemiImplicitStress with array-valued ocean velocities: the cross component averaged to the u / v points
// (ubar at v points from fu, vbar at u points from fv), once per sub-cycle (evp_fast.hip)
void launch_forcing_bars(const EvpDev& P, const FRef& ubar_v, const FRef& vbar_u, hipStream_t s, bool top = false);
void fused_fill_forcing_top(const EvpDev& P, const FRef& ubar_v, const FRef& vbar_u, FusedTable* t);
void fused_fill_forcing(const EvpDev& P, const FRef& ubar_v, const FRef& vbar_u, FusedTable* host_table);
void fused_fill_extra(const EvpDev& P, const FRef& xd_u, const FRef& xd_v, FusedTable* host_table);

// halo / masks / copies (halo.hip)
void launch_fill_halo(const FRef& f, const GridDev& g, const ImageSpec& im, hipStream_t s);
void launch_mask_center(const FRef& f, const GridDev& g, hipStream_t s);
void launch_mask_u(const FRef& f, const GridDev& g, hipStream_t s);
struct HaloBatch { FRef f[6]; ImageSpec im[6]; int n; };
void launch_fill_halo_batch(const HaloBatch& B, const GridDev& g, hipStream_t s);
void launch_fill_halo_xcolumns(const HaloBatch& B, const GridDev& g, hipStream_t s);
void launch_mask_v(const FRef& f, const GridDev& g, hipStream_t s);
struct CopyBatch { const double* src[6]; double* dst[6]; long n[6]; int count; int aligned16; };
void launch_copy_batch(const CopyBatch& B, hipStream_t s, int block = 256);      // block 64: beside a pair launch (one-wave workgroups find a slot)

// advection + tracer update (advect.hip)
struct AdvDev {
    GridDev g;
    FRef u, v, h, a, Gh, Ga, hm, am;
    FRef hs, Ghs, hsm;      // snow thickness as a third tracer (has_snow)
    int has_snow;
    int fill_images;        // tracer update: also store the local halo images (im) of h, aice [, hs]
    ImageSpec im;
    int scheme;
    double dt;
    int from_cache;
    // one RK stage in ONE launch (launch_advect_stage): tendencies of (h, a) -- the stage's input --, then the tracer update
    // base + dt G written to OTHER arrays (ho, ao; with their halo images), so that no block reads what another has updated
    FRef hb, ab, ho, ao;    // the update's base (Psi^-) and output
    int write_cache;        // first stage: also store the base values into hm, am (cache_current_fields!, with halo images)
    int nt;                 // tracers per thread of the tendency kernel: 0 by grid size, 1 / 2 forced (CSI_ADV_NT)
    int w32;                // WENO schemes: smoothness indicators / weights in single precision (csi_set_weno_weight_dtype; advect.hip)
    int shape;              // block shape of the two-tracers-per-thread layout: 0 by grid size, 1 / 2 / 3 forced to 64 x 8 / 63 x 7 / 63 x 11 (CSI_ADV_SHAPE)
};
// what a tendency / stage launch used: tracers per thread and the cells of a flux tile (csi_last_advection)
struct AdvLayout { int nt, tx, ty; };
AdvLayout launch_tracer_tendencies(const AdvDev& A, int mode, hipStream_t s);
void launch_tracer_step(const AdvDev& A, hipStream_t s);
AdvLayout launch_advect_stage(const AdvDev& A, int mode, hipStream_t s);

// slab thermodynamics (thermo.hip)
struct SlabDev {
    double k, rho_bulk, rho_pure, rho_l, c_l, c_i, L0, T0, liq_slope, liq_T0, S, hc, Tu, Qu, Qb;
    int top_flux_kind, bot_flux_kind;
    int top_bc_kind;         // 0 PrescribedTemperature, 1 MeltingConstrainedFluxBalance (numeric flux, closed form)
    double ice_salinity;
};
struct SnowDev {
    double k, rho, snowfall, Tu;
    int top_bc_kind;
};
struct LayeredOut { FRef mf_ice, mf_snow, mf_int, tu_ice, tu_snow; };   // optional outputs (p == nullptr: absent)
// what a thermodynamic launch used (csi_last_thermo): step 1 k_slab, 2 k_layered, 3 k_slab_flux, 4 k_layered_flux (0: none yet); the
// table of the flux kernels it took the launcher from (SW_NONE / SW_NUMBER / SW_CELL); the index into that table (-1: the numeric kernels)
struct ThermoLaunch { int step, sw, index; };
ThermoLaunch launch_layered_step(const SlabDev& S, const SnowDev& W, const GridDev& g, const FRef& h, const FRef& a, const FRef& hs,
                                 const LayeredOut& o, double dt, hipStream_t s);
ThermoLaunch launch_slab_step(const SlabDev& S, const GridDev& g, const FRef& h, const FRef& a, const FRef& mf, int has_mf,
                              double dt, hipStream_t s);

// per-cell heat fluxes, RadiativeEmission, the surface-temperature solve (thermo_flux.hip; include/csi.h csi_heat_fluxes_set)
constexpr int kMaxFluxTerms = 8;
enum : int { FLUX_CONST = 0, FLUX_ARRAY = 1, FLUX_EMISSION = 2, FLUX_LINEAR = 3, FLUX_SHORTWAVE = 4 };
enum : int { LIN_NONE = 0, LIN_NUMBERS = 1, LIN_ARRAYS = 2 };                 // the top's LINEAR term: absent, K and Ta numbers, both per cell
enum : int { WEIGHT_NONE = 0, WEIGHT_CONCENTRATION = 1, WEIGHT_ICE_PRESENT = 2 };
enum : int { SW_NONE = 0, SW_NUMBER = 1, SW_CELL = 2 };                       // the top's SHORTWAVE term: absent, F a number, F per cell
struct FluxTermsDev {
    int n;                     // 0: the side takes SlabDev's number (Qu / Qb with top_flux_kind / bot_flux_kind)
    int kind[kMaxFluxTerms];
    double value[kMaxFluxTerms], eps[kMaxFluxTerms], sigma[kMaxFluxTerms], Tr[kMaxFluxTerms];   // (LINEAR: value = K, Tr = Ta)
};
struct HeatFluxDev {
    FluxTermsDev top, bot;
    double tol = 1e-3;
    int maxiters = 1000;
    int prescribed_array = 0;  // PrescribedTemperature read per cell from the surface's temperature field
    int snowfall_array = 0;
    int lin = LIN_NONE;        // the top's LINEAR term (at most one)
    int lin_weight = WEIGHT_NONE;
    int bottom_salinity_array = 0;      // Tb per cell from FluxFields.sbot
};
// qtop / qbot: the ARRAY terms' fields; snowfall: per-cell snowfall; tu: the solved surface's temperature field (CSI_F_TU for the
// bare-ice step, CSI_F_TUS for the layered one) -- Tu- of the secant, the prescribed per-cell value, and the output; lin_k / lin_ta:
// the LINEAR term's per-cell K and Ta; sbot: the per-cell bottom salinity; qtop_used / qbot_used: optional outputs (p == nullptr: absent)
struct FluxFields { FRef qtop, qbot, snowfall, tu, lin_k, lin_ta, sbot, qtop_used, qbot_used; };
// The SHORTWAVE term (include/csi.h csi_shortwave_set): alpha = (T < thr) ? cold : warm, Q = (F * (1 - alpha)) * w.  It is the LAST
// argument of the SW_NUMBER / SW_CELL instantiations of both kernels and no argument of the SW_NONE ones, so HeatFluxDev, FluxFields and
// every argument offset of the kernels of before keep their layout.  f: F per cell (SW_CELL); albedo_used: optional output (p == nullptr: absent); snow_pair: the
// layered step takes the snow triple where hs > 0.
struct ShortwaveDev {
    int mode = SW_NONE, weight = WEIGHT_NONE, snow_pair = 0, pad_ = 0;
    double F = 0, cold = 0, warm = 0, thr = 0, snow_cold = 0, snow_warm = 0, snow_thr = 0;
    FRef f{}, albedo_used{};
};
bool flux_has_emission(const FluxTermsDev& t);
// the kernels read the cell's surface temperature (their LTU flag): the field -- CSI_F_TU / CSI_F_TUS -- must be bound exactly then
bool flux_reads_surface_temperature(const HeatFluxDev& F, int sw_mode, int top_bc_kind);
// (both return the table and the index b they launched from)
ThermoLaunch launch_slab_flux_step(const SlabDev& S, const HeatFluxDev& F, const FluxFields& ff, const ShortwaveDev& sw, const GridDev& g,
                                   const FRef& h, const FRef& a, const FRef& mf, int has_mf, double dt, hipStream_t s);
ThermoLaunch launch_layered_flux_step(const SlabDev& S, const SnowDev& W, const HeatFluxDev& F, const FluxFields& ff, const ShortwaveDev& sw,
                                      const GridDev& g, const FRef& h, const FRef& a, const FRef& hs, const LayeredOut& o, double dt,
                                      hipStream_t s);

// the slab-ocean mixed layer (mixed_layer.hip; include/csi.h csi_mixed_layer_set).  rc = rho * c, C = rc * depth, grc = gamma * rc,
// formed on the host in this order; Fo, K, Ta, Qd, S: the numbers a configuration without the array reads; nx, ny: the interior.
struct MixedLayerDev {
    double rc, C, grc, Fo, K, Ta, Qd, liq_T0, liq_slope, S, dt;
    int has_surface, has_bulk;       // which terms of Qs exist (an array implies its term)
    int nx, ny;
};
// to_in: To or its Psi^- copy; to_out: To; a: the concentration; qb: the bottom heat-flux array (output); fo, k, ta, qd, sb: the arrays
// a configuration has (p == nullptr: the number); qow: optional output (p == nullptr: absent)
struct MixedLayerFields { FRef to_in, to_out, a, qb, fo, k, ta, qd, sb, qow; };
void launch_mixed_layer(const MixedLayerDev& M, const MixedLayerFields& F, hipStream_t s);

// forcing time series interpolated at the model clock (time_series.hip; include/csi.h csi_time_series_update): every series-driven
// slot in ONE launch.  A descriptor: the two slices around the clock (a: psi_1, b: psi_2; b == a where n1 == n2), the interior of the
// bound array, row strides in doubles, the interior extents and the weights w2 = n~, w1 = 1 - n~ (formed on the host, in double).
constexpr int kMaxSeries = 19;      // (fourteen, the mixed layer's four inputs and the shortwave flux)
struct SeriesDesc {
    const double *a, *b;
    double* dst;
    long lda, ldb, ldd;
    int nx, ny;
    double w1, w2;
    int same;                  // n1 == n2: dst = psi_1, bit for bit
    int pad_;
};
struct SeriesTable { int n; int pad_; SeriesDesc d[kMaxSeries]; };
void launch_time_series(const SeriesTable& T, hipStream_t s);

// ... given on a source grid of their own (time_series_regrid.hip; include/csi.h csi_time_series_set_regridded): every regridded slot
// in ONE launch.  A descriptor: per source series (part 0: the scalar or the east series, part 1: the north series of a pair) the two
// slices around the clock, their row stride and time weights as in SeriesDesc; the map's planes (entries of 8 bytes, `plane` entries
// apart, rows mld entries apart: IDX, WX, WY and, with rotation, COS, SIN; target point x of row j at entry j * mld + x + head(j),
// head(j) = 1 where the destination row's interior starts 8 bytes behind a 16-byte boundary -- the padding entries are zero); the
// interior of the bound array.
struct RegridDesc {
    const double *a[2], *b[2];
    double w1[2], w2[2];
    long lds[2];
    const unsigned long long* map;
    long mld, plane;
    double* dst;
    long ldd;
    int nx, ny;
    int same[2];
    int pair;                  // 0: scalar; 1: one component of a vector pair (the map has COS and SIN)
    int component;             // 0: x = E cos + N sin; 1: y = N cos - E sin
};
struct RegridTable { int n; int pad_; RegridDesc d[kMaxSeries]; };
static_assert(sizeof(RegridTable) <= 4096, "the table travels by value as the kernel argument");
void launch_time_series_regrid(const RegridTable& T, hipStream_t s);

// device diagnostics (diagnostics.hip; include/csi.h csi_diagnostics_compute).  One 8-byte slot per quantity, in this order, in every
// partial record and in the result; the counts are int64 bit patterns in their slots.  Slots below DQ_VOLUME: CSI_DIAG_VELOCITY,
// from DQ_VOLUME on: CSI_DIAG_TRACERS.
enum : int { DQ_INV_TIMESCALE = 0, DQ_MAX_ABS_U, DQ_MAX_ABS_V, DQ_NONFINITE_U, DQ_NONFINITE_V, DQ_NAN_U, DQ_NAN_V,
             DQ_VOLUME, DQ_AREA, DQ_EXTENT, DQ_SNOW_VOLUME, DQ_ACTIVE_AREA, DQ_MIN_H, DQ_MAX_H, DQ_MIN_AICE, DQ_MAX_AICE, DQ_MAX_HS,
             DQ_NONFINITE_H, DQ_NONFINITE_AICE, DQ_NONFINITE_HS, DQ_ACTIVE_CELLS, DQ_COUNT };
// what a slot holds (ordered_reduce.h combine / identity), and the diagnostics' map from slot to kind: the ONE statement, used by the
// kernels (diagnostics.hip) and by the host's combine over ranks (csi_diagnostics.hip)
enum : int { K_SUM = 0, K_MAX = 1, K_MIN = 2, K_CNT = 3 };
struct DiagKinds {
    __host__ __device__ static constexpr int kind(int q) {
        return (q == DQ_INV_TIMESCALE || q == DQ_MAX_ABS_U || q == DQ_MAX_ABS_V || q == DQ_MAX_H || q == DQ_MAX_AICE || q == DQ_MAX_HS) ? K_MAX
             : (q == DQ_MIN_H || q == DQ_MIN_AICE) ? K_MIN
             : (q >= DQ_VOLUME && q <= DQ_ACTIVE_AREA) ? K_SUM
             : K_CNT;
    }
};
struct DiagDev {
    GridDev g;
    FRef u, v, h, a, hs;       // (a group that is not requested: unused)
    int exu, eyv;              // 1: u has the faces i = Nx + 1 / v the faces j = Ny + 1 (Bounded direction; a tile: its east / north wall)
    int has_hs;
    int pad_;
    double threshold;          // ice_extent counts cells with aice >= threshold
    double* part;              // partial records (layout, block shape and order: ordered_reduce.h)
    long nrec;                 // records = blocks of the first launch (red::diag_geometry)
};
// the two launches: partial records into D.part, the folded result into out[DQ_COUNT] (device memory; only the requested groups' slots are written)
void launch_diagnostics(const DiagDev& D, bool vel, bool trc, double* out, hipStream_t s);

// derived fields (derived.hip; include/csi.h csi_derived_compute): every requested field in ONE launch.  out[k]: the array bound to slot
// CSI_F_D_DIVERGENCE + k as a (0, 0)-offset reference, p == nullptr where the field is not requested.
enum : int { DV_DIVERGENCE = 0, DV_SHEAR, DV_DEFORMATION, DV_SPEED, DV_SIGMA_I, DV_SIGMA_II, DV_STRESS_POWER, DV_COUNT };
struct DerivedDev {
    GridDev g;
    FRef u, v, s11, s22, s12, P;      // (the stress group's four: unused without it)
    FRef out[DV_COUNT];
};
void launch_derived(const DerivedDev& D, bool stress, hipStream_t s);

// energy budget integrals (budget.hip; include/csi.h csi_budget_compute): the ordered reduction of ordered_reduce.h with three sums.
// Slots below BQ_KINETIC: CSI_BUDGET_STRESS.
enum : int { BQ_WORK = 0, BQ_POWER, BQ_KINETIC, BQ_COUNT };
struct BudgetDev {
    GridDev g;
    FRef u, v, s11, s22, s12, h, a;
    double rho;
    double* part;
    long nrec;
};
void launch_budget(const BudgetDev& D, bool stress, bool kin, double* out, hipStream_t s);

// momentum balance terms and their power (momentum_terms.hip; include/csi.h csi_momentum_terms_compute / csi_momentum_budget_compute).
// out[2 * t] / out[2 * t + 1]: the arrays bound to the _X / _Y slot of term t as (0, 0)-offset references, p == nullptr where the slot is
// not requested.  The power sums: the ordered reduction of ordered_reduce.h, every slot a sum.
enum : int { MQ_CORIOLIS = 0, MQ_TOP, MQ_BOTTOM, MQ_INTERNAL, MQ_FORCING, MQ_COUNT };
struct MomTermsDev {
    EvpDev P;                  // grid, u, v, h, aice, sigma (unused by the viscous instantiation), stresses, Coriolis, forcing, rho
    double nu;                 // ViscousRheology(nu)
    FRef out[2 * MQ_COUNT];
    int exu, eyv;              // 1: u has the faces i = Nx + 1 / v the faces j = Ny + 1 (the high side is a wall)
    int no_internal;           // the internal term is +0.0: free-drift dynamics (no rheology), or the term is not requested
    int raw_stress;            // TOP / BOTTOM receive tau itself
    double* part;              // power: partial records
    long nrec;
};
// visc: sigma = nu * delta u inline and no load of the stored stresses (also chosen where the internal term is off)
void launch_momentum_terms(const MomTermsDev& T, bool visc, hipStream_t s);
void launch_momentum_power(const MomTermsDev& T, bool visc, double* out, hipStream_t s);

// device-side output (output.hip; include/csi.h csi_output_accumulate / csi_output_snapshot): every field of a set in ONE launch.  A
// descriptor: the first INTERIOR element of the bound array and its row stride in doubles, the dense (ny, nx) accumulator of an
// averaged field, the field's place in the staging slot, the interior extents.  accumulate: w = the weight, the table holds the
// averaged fields only; pack: w = W, the sum of the weights; mask = the byte of cell (1, 1) (null: no mask set), rows mask_ld apart.
constexpr int kMaxOutputFields = 16;
struct OutputDesc {
    const double* src;
    double* acc;
    void* dst;
    long lds;
    int nx, ny;
    int f32, averaged, masked;
    int pad_;
    double fill;
};
struct OutputTable { int n; int mask_ld; double w; const unsigned char* mask; OutputDesc d[kMaxOutputFields]; };
void launch_output_accumulate(const OutputTable& T, hipStream_t s);
void launch_output_pack(const OutputTable& T, hipStream_t s);

// Lagrangian ice drifters (drifters.hip; include/csi.h csi_drifters_advance / csi_drifters_sample): one thread per drifter.  xi, eta,
// status: the caller's arrays of n entries.  advance: m sub-steps of tau in ONE launch; sample: the columns of `columns` at
// out[k * ld + q]; hs.p == nullptr where the HS column is not requested (h, a likewise).
struct DriftersDev {
    GridDev g;
    FRef u, v, h, a, hs;
    double* xi;
    double* eta;
    int32_t* status;
    long n;
};
void launch_drifters_advance(const DriftersDev& D, double tau, int m, hipStream_t s);
void launch_drifters_sample(const DriftersDev& D, int columns, double* out, long ld, hipStream_t s);

// per-region ice integrals and extrema (regions.hip; include/csi.h csi_regions_compute): the diagnostics' tracer group restricted to the
// cells of each region of the caller's id map.  One 8-byte slot per quantity, in this order, in every record; RQ_CELLS is an int64 bit
// pattern.  Records: slot q of region r of block b at part[((long)r * RQ_COUNT + q) * nrec + b] -- contiguous per region and slot, so
// red::finish_records' block r reads region r as the diagnostics' single block reads its own.  Region index n_regions is the record of
// the cells that belong to NO region: identities, and their number in RQ_CELLS.
enum : int { RQ_VOLUME = 0, RQ_AREA, RQ_EXTENT, RQ_SNOW_VOLUME, RQ_REGION_AREA, RQ_MIN_H, RQ_MAX_H, RQ_MIN_AICE, RQ_MAX_AICE, RQ_MAX_HS,
             RQ_CELLS, RQ_COUNT };
constexpr int kRegionsMax = 64;
struct RegionKinds {
    __host__ __device__ static constexpr int kind(int q) {
        return (q == RQ_MAX_H || q == RQ_MAX_AICE || q == RQ_MAX_HS) ? K_MAX : (q == RQ_MIN_H || q == RQ_MIN_AICE) ? K_MIN : q == RQ_CELLS ? K_CNT : K_SUM;
    }
};
struct RegionsDev {
    GridDev g;
    FRef h, a, hs;
    const int32_t* ids;        // element (0, 0)-offset like the mask: the id of cell (i, j) at ids[i + j * ids_ld]
    long ids_ld;
    int n_regions;             // 1 .. kRegionsMax
    int has_hs;
    double threshold;
    double* part;
    long nrec;
};
// the two launches: records into D.part, the (n_regions + 1) x RQ_COUNT folded slots into out (device memory)
void launch_regions(const RegionsDev& D, double* out, hipStream_t s);

// advected ice tracers (tracers.hip; include/csi.h csi_tracers_tendencies / csi_tracers_update).  Every tracer array has the row stride
// ld of the array bound to CSI_F_H: c, cb (the base c^-: the tracer itself under FE, the library's Psi^- copy under RK3) and G are
// (0, 0)-offset addresses, G[k] == nullptr where the tendency is not stored.  cin: what the stencil reads -- the tracer itself, or under RK3
// from the second stage on, for a tracer with a source, the library's source-free copy of the stage before; cfree: where the second half
// stores that copy (nullptr: not stored).  star: the dense c* of the stage -- tracer k, cell (i, j)
// at star[k * star_plane + (i - 1) + (j - 1) * star_ld], star_ld and star_plane even, so that a pair of cells (odd i, i + 1) is 16-byte aligned.
constexpr int kTracersMax = 8;
struct TracersDev {
    GridDev g;
    FRef u, v;
    FRef a;                    // the concentration of the stage's input (the weight of the stencil values) / of its end (second half)
    FRef ab, Ga;               // the base aice^- and the tendency just written (BY_CONCENTRATION)
    ImageSpec im;
    int n, scheme, w32, pad_;
    double dt;
    long ld;
    double* c[kTracersMax];
    double* cin[kTracersMax];
    double* cfree[kTracersMax];
    double* cb[kTracersMax];
    double* G[kTracersMax];
    double* star;
    long star_ld, star_plane;
    int weighting[kTracersMax], nonnegative[kTracersMax];
    double source[kTracersMax];
};
static_assert(sizeof(TracersDev) <= 4096, "the description travels by value as the kernel argument");
// what a stencil launch used (csi_tracers_last): tracers per thread, the cells of a flux tile, tracer groups on blockIdx.z
struct TracerLayout { int ntr, tx, ty, groups; };
TracerLayout launch_tracers_tendencies(const TracersDev& T, int mode, int force_ntr, hipStream_t s);
void launch_tracers_star_noadv(const TracersDev& T, hipStream_t s);
void launch_tracers_finish(const TracersDev& T, hipStream_t s);

}  // namespace csi
