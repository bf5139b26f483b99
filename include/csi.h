/*
 * csi.h -- C ABI of the MI355X-native sea-ice hot path (libcsi_hip.so).
 *
 * Drop-in boundary for CliMA/ClimaSeaIce.jl's split-explicit EVP momentum sub-cycle,
 * the h / aice advection and their launch loop.  The reference has no FFI of its own:
 * its "operator API" is Julia multiple dispatch, so every entry point below names the
 * Julia method it replaces (paths relative to /root/reference/src); INTEGRATION.md shows
 * the `ccall` methods a maintainer adds on the Julia side.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, fp64 only, no C++ / torch types.
 *  - Every function returns int32_t: CSI_OK (0) or a negative csi_status; the text of the
 *    last failure is available from csi_last_error().  No exception crosses the boundary.
 *  - Ownership: the caller (Julia / AMDGPU.jl ROCArray parents; torch tensors in this repo's
 *    harness) owns all field memory; the library never frees or reallocates it.  Scratch
 *    lives in the context.
 *  - Field layout = Oceananigans parent array: column-major, i fastest, element (i, j)
 *    (1-based) at ptr[(i + Hx - 1) + (j + Hy - 1) * ld], ld = Nx + 2Hx (+1 when the field
 *    is Face-located in a Bounded x direction).
 *  - One context per GPU; calls on one context are serialised by the caller.  All work is
 *    ordered on the context's HIP stream (an external hipStream_t may be supplied); the only
 *    host synchronisation is csi_sync().
 *  - There is NO CPU fallback: every compute entry point needs a HIP device.
 */
#ifndef CSI_H
#define CSI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSI_VERSION 100 /* 0.1.0 */

typedef enum {
    CSI_OK = 0,
    CSI_ERR_INVALID_ARGUMENT = -1,
    CSI_ERR_NOT_BOUND = -2,     /* a field / grid / parameter needed by the call was never set */
    CSI_ERR_HIP = -3,           /* a HIP runtime call failed; see csi_last_error */
    CSI_ERR_UNSUPPORTED = -4,   /* valid in the reference, not (yet) in this library */
    CSI_ERR_NO_DEVICE = -5,
    CSI_ERR_COMM = -6           /* RCCL failure */
} csi_status;

/* Topology of one horizontal direction (Oceananigans.Grids topologies).  The *_CONNECTED
 * values mark tile edges whose halos are filled by csi_halo_exchange (multi-GPU) rather than
 * by a local boundary condition (split_explicit_momentum_equations.jl:13-16). */
typedef enum {
    CSI_PERIODIC = 0,
    CSI_BOUNDED = 1,
    CSI_FULLY_CONNECTED = 2,
    CSI_LEFT_CONNECTED = 3,   /* low side exchanged, high side Bounded */
    CSI_RIGHT_CONNECTED = 4,  /* low side Bounded, high side exchanged */
    /* y direction of a TripolarGrid: low side Bounded (the southernmost latitude), high side the north FOLD filled by the
     * Zipper boundary condition.  Sign: fields at the velocity points -- (Face, Center) and (Center, Face): u, v, the stress /
     * ocean-velocity / forcing arrays there, u^n, v^n -- change sign across the fold (sea_ice_model.jl:57-64 for u, v;
     * test/distributed_tests_utils.jl:196-197 builds the others with the same conditions), every (Center, Center) and
     * (Face, Face) field does not.  Pivot: the ONE variant implemented has the fold running through the cell CENTRES of row
     * Ny (Oceananigans' RightCenterFolded / LeftConnectedRightCenterFolded, the names the reference imports at
     * split_explicit_momentum_equations.jl:7-16): c[i, Ny + j] = s c[i', Ny - j] for Center-in-y fields (row Ny is stored
     * twice and its two copies are NOT symmetrised: they evolve independently, as in a fill that only writes halos),
     * s c[i', Ny - j + 1] for Face-in-y fields, i' = Nx - i + 1 (Center in x) / Nx - i + 2 (Face in x; column 1 maps onto itself
     * without the sign change).  The F-point pivot (RightFaceFolded) is not implemented.  STATUS: these fill semantics are
     * RECALLED from the un-vendored Oceananigans, restated three times here (oracle/csi_oracle.c fold_north,
     * grids.fold_north, the HIP store images) and checked against each other only -- no reference-run fixture exists; run
     * bench/reference_driver.jl on a tripolar case before relying on them.  x must be Periodic (or, on
     * tiles, unpartitioned: the reference's own distributed tripolar test partitions y only,
     * test/distributed_tests_utils.jl:239).  Fusion level 2 on an untiled RIGHT_FOLDED grid: rows 1 .. Ny - Hy - 4 run
     * through the two-sub-steps kernel, the rows next to the fold through the three kernels on their own stream (they read and
     * store fold images like the reference's kernels; csi_abi.hip FoldBand) -- bit-identical to the three-kernel run of the whole
     * grid; the fold tile of a y partition (LEFT_CONNECTED_RIGHT_FOLDED) does the same when the exchange interval is even.  Fusion
     * level 1 stays on the three kernels. */
    CSI_RIGHT_FOLDED = 5,
    CSI_LEFT_CONNECTED_RIGHT_FOLDED = 6   /* the northernmost tile of a y partition of such a grid */
} csi_topology;

typedef enum {
    CSI_METRIC_UNIFORM = 0,   /* RectilinearGrid, regular spacing */
    CSI_METRIC_PER_J = 1,     /* LatitudeLongitudeGrid, regular: metrics vary with j only */
    CSI_METRIC_FULL = 2       /* orthogonal curvilinear grid (OrthogonalSphericalShellGrid, TripolarGrid and the like): 2-D metric
                               * arrays.  Every operator takes them (same calls as the reference's Oceananigans.Operators).  FAST
                               * mode folds them into twelve per-POINT coefficient planes; the two-sub-steps kernel has
                               * instantiations for them (fusion level 2), level 1 runs the three kernels.  Rows whose planes hold
                               * one value per row are read from per-row vectors (csi_set_row_constant). */
} csi_metric_kind;

/* Host-side description of the grid metrics (copied by csi_grid_set).  PER_J vectors have
 * length Ny + 2Hy + 1; the entry for row j (1-based) sits at [j + Hy - 1]:
 *   dxc = dx at Center rows (dx^cc = dx^fc)   dxf = dx at Face rows (dx^cf = dx^ff)
 *   azc = Az at Center rows (Az^cc = Az^fc)   azf = Az at Face rows (Az^cf = Az^ff)
 * dy is constant for these two kinds. */
typedef struct {
    double dx, dy;
    const double *dxc, *dxf, *azc, *azf;
    /* CSI_METRIC_FULL: the twelve HOST arrays dx, dy, Az at (c,c), (f,c), (c,f), (f,f) -- index 4 * {dx 0, dy 1, Az 2}
     * + (x at Face) + 2 * (y at Face), i.e. dx^ccc, dx^fcc, dx^cfc, dx^ffc, dy^ccc, ... -- each with Ny + 2Hy + 1 rows
     * of leading dimension full_ld >= Nx + 2Hx + 1; element (i, j) at [(i + Hx - 1) + (j + Hy - 1) * full_ld]. */
    const double* full[12];
    int64_t full_ld;
} csi_metrics;

/* Field slots (csi_field_bind).  Locations: (x, y) with c = Center, f = Face. */
typedef enum {
    CSI_F_U = 0,      /* (f,c) model.velocities.u */
    CSI_F_V,          /* (c,f) model.velocities.v */
    CSI_F_H,          /* (c,c) model.ice_thickness */
    CSI_F_A,          /* (c,c) model.ice_concentration */
    CSI_F_S11,        /* (c,c) auxiliaries.fields.sigma11  (elasto_visco_plastic_rheology.jl:147) */
    CSI_F_S22,        /* (c,c) :148 */
    CSI_F_S12,        /* (f,f) :149 */
    CSI_F_UN,         /* (f,c) :150 */
    CSI_F_VN,         /* (c,f) :151 */
    CSI_F_P,          /* (c,c) :152 */
    CSI_F_ALPHA,      /* (c,c) :153 */
    CSI_F_DELTA,      /* (c,c) :154 */
    CSI_F_ZETA_F,     /* (f,f) :157 */
    CSI_F_ZETA_C,     /* (c,c) :158 */
    CSI_F_GH,         /* (c,c) timestepper.G^n.h */
    CSI_F_GA,         /* (c,c) timestepper.G^n.aice */
    CSI_F_HM,         /* (c,c) timestepper.Psi^-.h   (sea_ice_rk_substep.jl:29-42) */
    CSI_F_AM,         /* (c,c) timestepper.Psi^-.aice */
    CSI_F_UM,         /* (f,c) timestepper.Psi^-.u */
    CSI_F_VM,         /* (c,f) timestepper.Psi^-.v */
    CSI_F_TOP_U,      /* (f,c) top stress array or top external velocity u_e */
    CSI_F_TOP_V,      /* (c,f) */
    CSI_F_BOT_U,      /* (f,c) bottom stress array or bottom external velocity u_e */
    CSI_F_BOT_V,      /* (c,f) */
    CSI_F_MASS_FLUX,  /* (c,c) mass_fluxes.thermodynamics.ice */
    CSI_F_HS,         /* (c,c) model.snow_thickness (snow layer; optional) */
    CSI_F_GHS,        /* (c,c) timestepper.G^n.hs */
    CSI_F_HSM,        /* (c,c) timestepper.Psi^-.hs */
    CSI_F_MASS_FLUX_SNOW,   /* (c,c) mass_fluxes.thermodynamics.snow (optional) */
    CSI_F_SNOWFALL_INTERCEPTED, /* (c,c) mass_fluxes.intercepted_snowfall (optional) */
    CSI_F_TU,         /* (c,c) ice_thermodynamics.top_surface_temperature (optional output; read-write state under
                       * csi_heat_fluxes_set / csi_surface_solve_set, see there) */
    CSI_F_TUS,        /* (c,c) snow_thermodynamics.top_surface_temperature (likewise) */
    CSI_F_FORCING_U,  /* (f,c) model.forcing.u given as an array: the `user_forcing` of sum_of_forcing_u
                       * (elasto_visco_plastic_rheology.jl:391-395), an acceleration in m s^-2; optional, both or neither */
    CSI_F_FORCING_V,  /* (c,f) model.forcing.v (:397-401) */
    CSI_F_GU,         /* (f,c) timestepper.G^n.u: the ExplicitSolver's velocity tendency (explicit_momentum_equations.jl:103-104) */
    CSI_F_GV,         /* (c,f) timestepper.G^n.v */
    CSI_F_COUNT
} csi_field_id;
/* Further (c,c) slots of csi_field_bind: the thermodynamics' per-cell inputs (csi_heat_fluxes_set, csi_surface_solve_set).  They are
 * numbered from CSI_F_COUNT on, so that csi_field_id and CSI_F_COUNT keep their values. */
typedef enum {
    CSI_F_TOP_HEAT_FLUX = CSI_F_COUNT,   /* the ARRAY term of the top heat flux, W m^-2 */
    CSI_F_BOTTOM_HEAT_FLUX,              /* the ARRAY term of the bottom heat flux */
    CSI_F_SNOWFALL,                      /* per-cell snowfall, kg m^-2 s^-1 (csi_surface_solve.snowfall_array) */
    CSI_F_COUNT_ALL
} csi_thermo_field_id;
/* Further slots of csi_field_bind: the prescribed free-drift velocity fields of csi_free_drift_set(ctx, 2).  Numbered from
 * CSI_F_COUNT_ALL on, so that csi_field_id, csi_thermo_field_id, CSI_F_COUNT and CSI_F_COUNT_ALL keep their values. */
typedef enum {
    CSI_F_FREE_DRIFT_U = CSI_F_COUNT_ALL,   /* (f,c) free_drift.u of `free_drift = (u = ..., v = ...)` (stress_balance_free_drift.jl:123-125) */
    CSI_F_FREE_DRIFT_V,                     /* (c,f) free_drift.v */
    CSI_F_COUNT_TOTAL                       /* every slot csi_field_bind takes */
} csi_free_drift_field_id;

typedef enum { CSI_PRESSURE_REPLACEMENT = 0, CSI_PRESSURE_ICE_STRENGTH = 1 } csi_pressure_kind;

/* ElastoViscoPlasticRheology (elasto_visco_plastic_rheology.jl:14-25, defaults :119-127) +
 * SeaIceMomentumEquation scalars (sea_ice_momentum_equations.jl:67-94) + FPlane coriolis +
 * sea_ice_density (sea_ice_model.jl:142-145). */
typedef struct {
    double ice_compressive_strength;   /* P*      27500 */
    double ice_compaction_hardening;   /* C       20 */
    double yield_curve_eccentricity;   /* e       2 */
    double minimum_plastic_stress;     /* Dmin    2e-9 */
    double min_relaxation_parameter;   /* alpha-  50 */
    double max_relaxation_parameter;   /* alpha+  300 */
    double relaxation_strength;        /* c_alpha pi^2 */
    int32_t pressure_formulation;      /* csi_pressure_kind */
    int32_t has_coriolis;              /* 0: coriolis = nothing, 1: FPlane(f) */
    double coriolis_f;
    double minimum_concentration;      /* 1e-3 */
    double minimum_mass;               /* 1.0 */
    double sea_ice_density;            /* 900 */
} csi_evp_params;

typedef enum {
    CSI_STRESS_NONE = 0,           /* nothing */
    CSI_STRESS_CONST = 1,          /* Number / NamedTuple of Numbers (sea_ice_external_stress.jl:16-17,29-37) */
    CSI_STRESS_FIELD = 2,          /* arrays bound to CSI_F_{TOP,BOT}_{U,V} (:19-20) */
    CSI_STRESS_SEMI_IMPLICIT = 3   /* SemiImplicitStress (:84-130,176-202) */
} csi_stress_kind;
typedef enum { CSI_VEL_ZERO = 0, CSI_VEL_CONST = 1, CSI_VEL_FIELD = 2 } csi_velocity_kind;
typedef enum { CSI_STRESS_TOP = 0, CSI_STRESS_BOTTOM = 1 } csi_stress_side;

typedef struct {
    int32_t kind;                  /* csi_stress_kind */
    int32_t ue_kind, ve_kind;      /* csi_velocity_kind: ZeroField / ConstantField / Field (bound slots) */
    int32_t reserved;
    double tau_u, tau_v;           /* CONST */
    double ue, ve;                 /* SEMI_IMPLICIT with ConstantField external velocity */
    double rho_e, Cd;              /* SEMI_IMPLICIT: 1026, 5.5e-3 */
} csi_stress;

/* Arithmetic mode of the kernels.
 * STRICT: the reference's operation order, no FMA contraction, IEEE division -- bit-for-bit
 *         equal to the CPU oracle (used to anchor parity).
 * FAST:   hoisted reciprocals / FMA contraction, shared strain rates; differs from STRICT
 *         by rounding only (tolerance stated in DESIGN.md and enforced in tests/).  Requires
 *         minimum_mass > 0 (the reference's default is 1 kg m^-2): the mi <= 0 guards of the velocity
 *         tendencies are then implied by the active / marginal ice selection and are not evaluated
 *         (CSI_ERR_UNSUPPORTED otherwise).  Requires minimum_plastic_stress > 0 as well (the reference's default
 *         is 2e-9 s^-1): 1 / Delta is formed from max(Delta^2, Delta_min^2) without a guard, and with Delta_min = 0
 *         an ice-free cell at rest would turn its stresses into NaN where the reference leaves them alone
 *         (CSI_ERR_UNSUPPORTED otherwise).  Advection, the tracer update and the thermodynamic steps are
 *         computed in the reference's order in both modes. */
typedef enum { CSI_MODE_STRICT = 0, CSI_MODE_FAST = 1 } csi_mode;

typedef enum { CSI_ADVECT_NONE = 0, CSI_ADVECT_UPWIND1 = 1, CSI_ADVECT_WENO3 = 3, CSI_ADVECT_WENO5 = 5, CSI_ADVECT_WENO7 = 7,
               CSI_ADVECT_UPWIND3 = -3, CSI_ADVECT_UPWIND5 = -5 } csi_advection_scheme;

typedef struct csi_context csi_context;

/* ---- lifecycle ------------------------------------------------------------------------- */
int32_t csi_version(void);
/* stream: a hipStream_t owned by the caller, or NULL for a library-owned stream. */
int32_t csi_context_create(int32_t device_id, void* hip_stream, csi_context** out);
int32_t csi_context_destroy(csi_context* ctx);
/* Text of the most recent failure on ctx (or of context creation when ctx == NULL). */
const char* csi_last_error(const csi_context* ctx);
int32_t csi_sync(csi_context* ctx);
/* csi_sync + the halo transport's status reduced over ALL ranks of the context's communicator (collective: every rank calls it
 * between the same two steps; one rank: the same as csi_sync).  A peer-transport wait that gave up reaches only the direct
 * neighbours' abort words; this is the call that lets every rank see it and take the same decision -- what the Julia side calls
 * before output writers / checkpointers read a Distributed model's fields (julia/ClimaSeaIceHIP.jl validate_state!; the
 * reference's own check of a distributed run is done after the fact, test/distributed_tests_utils.jl:40-88). */
int32_t csi_validate_all(csi_context* ctx);
/* Testing aid: leaves the host side in the state a timed-out wait of the peer transport's flag protocol leaves it in (the sticky
 * CSI_ERR_COMM above), without the wait.  Not for production use. */
int32_t csi_debug_peer_abort(csi_context* ctx);
int32_t csi_set_mode(csi_context* ctx, int32_t mode);

/* ---- problem description ----------------------------------------------------------------- */
/* Replaces the grid argument every reference kernel receives (Nx, Ny, halo, topology, metrics). */
int32_t csi_grid_set(csi_context* ctx, int32_t Nx, int32_t Ny, int32_t Hx, int32_t Hy,
                     int32_t topo_x, int32_t topo_y, int32_t metric_kind, const csi_metrics* metrics);
/* Cell-centred activity mask of an ImmersedBoundaryGrid (1 = active), device pointer laid out
 * like a (c,c) parent with leading dimension ld; NULL removes it.
 * (peripheral_node, split_explicit_momentum_equations.jl:226,261; conditional_flux_*,
 * ice_stress_divergence.jl:21-24; mask_immersed_field_xy!, sea_ice_model.jl:381-389) */
int32_t csi_mask_set(csi_context* ctx, const uint8_t* dev_mask, int64_t ld);
/* Bind the parent array of one field: device pointer, leading dimension and parent extents
 * (validated against the grid: ni = Nx + 2Hx [+1], nj = Ny + 2Hy [+1]).  * On a tiled model with the peer halo transport the neighbouring ranks map u, v, sigma11, sigma22, sigma12, alpha, zeta_c, zeta_f and
 * Delta: binding another array to one of these slots makes the next sub-cycle set the transport up again, COLLECTIVELY -- every
 * rank of the decomposition has to re-bind between the same two steps (like any collective). */
int32_t csi_field_bind(csi_context* ctx, int32_t field_id, void* dev_ptr, int64_t ld, int32_t ni, int32_t nj);
int32_t csi_evp_params_set(csi_context* ctx, const csi_evp_params* p);
int32_t csi_stress_set(csi_context* ctx, int32_t side, const csi_stress* s);
/* Boundary condition of the TANGENTIAL velocity at a wall: field_id CSI_F_U with side 0 (south) / 1 (north), CSI_F_V with
 * side 0 (west) / 1 (east).  kind 0: the default no-flux condition (halo = mirror image, free slip); kind 1:
 * ValueBoundaryCondition(value) -- no-slip for value 0, as in examples/ice_advected_on_coastline.jl:96-99 -- whose
 * halo fill sets the first halo cell to 2 * value - c[first interior cell] (upstream fill_halo_regions!, SURVEY.md
 * App. B; a13 of the scope table).  Sides that are not walls ignore it.  Every path takes it (the fused kernels
 * reflect about 2 * value where they otherwise mirror). */
int32_t csi_velocity_bc_set(csi_context* ctx, int32_t field_id, int32_t side, int32_t kind, double value);
/* Immersed boundary conditions of u / v: ImmersedBoundaryCondition(west = FluxBoundaryCondition(number), ...) entering
 * immersed_dj_sigma_1j / immersed_dj_sigma_2j (ice_stress_divergence.jl:65-123; the stress is minus the flux on west / south
 * faces and plus the flux on east / north faces, :115-123).  field_id CSI_F_U or CSI_F_V; all zeros (the default) is the
 * reference's default `nothing`.  Non-zero values need a mask (csi_mask_set) to have any effect; the two-sub-steps kernel takes
 * them (their divergence is evaluated once per sub-cycle into two library arrays), the one-sub-step kernel does not (three kernels). */
int32_t csi_immersed_flux_bc_set(csi_context* ctx, int32_t field_id, double west, double east, double south, double north);
/* Row-dependent Coriolis parameter: BetaPlane, f = f0 + beta * ynode (upstream x_f_cross_U / y_f_cross_U called at
 * momentum_tendencies_kernel_functions.jl:31,64; in the reference's test matrix, test/test_time_stepping.jl:35).
 * f_u: f at the (Face, Center) nodes of each row (u points), f_v: at the (Center, Face) nodes (v points); HOST
 * arrays laid out like the PER_J metric vectors (value for row j at [j + Hy - 1], n = Ny + 2Hy + 1; halo rows hold the
 * value of the row they image: the neighbouring tile's row, the wrapped row of a Periodic direction -- the fused
 * kernels recompute ring rows there and must see their owner's f).  They replace csi_evp_params.coriolis_f while set (has_coriolis must be 1);
 * NULL, NULL returns to the FPlane value.  Call after csi_grid_set (a new grid drops them). */
int32_t csi_coriolis_rows_set(csi_context* ctx, const double* f_u, const double* f_v, int32_t n);
/* Point-dependent Coriolis parameter on CSI_METRIC_FULL grids (f = 2 Omega sin(latitude) of a curvilinear grid whose
 * latitude varies along both indices, e.g. a TripolarGrid): f at the (Face, Center) and (Center, Face) nodes, HOST arrays laid
 * out like the metric planes (Ny + 2Hy + 1 rows of leading dimension ld >= Nx + 2Hx + 1, element (i, j) at
 * [(i + Hx - 1) + (j + Hy - 1) * ld]; halo entries hold the value of the point they image).  Applied with the stencil the
 * reference's hot path exercises, -f * Ixy(v) / +f * Ixy(u) (FPlane / BetaPlane: test/test_time_stepping.jl:35,
 * examples and distributed tests); upstream's HydrostaticSphericalCoriolis enstrophy-conserving stencil appears nowhere in
 * the reference and is not implemented.  Replaces csi_evp_params.coriolis_f / the rows while set; NULL, NULL removes it. */
int32_t csi_coriolis_points_set(csi_context* ctx, const double* f_u, const double* f_v, int64_t ld);

/* ---- the reference's verbs ----------------------------------------------------------------- */
/* initialize_rheology!(model, ::ElastoViscoPlasticRheology), elasto_visco_plastic_rheology.jl:192-219 */
int32_t csi_evp_initialize(csi_context* ctx);
/* The sub-step loop of time_step_momentum!, split_explicit_momentum_equations.jl:170-189:
 * local halo fill of u, v, then `substeps` x [compute_stresses! ; alternating u/v steps with halo
 * fills].  dt is the stage step.  first_substep is the 1-based index of the first sub-step
 * (parity selects the u/v order, :178). */
int32_t csi_evp_subcycle(csi_context* ctx, double dt, int32_t substeps, int32_t first_substep);
/* finalize_rheology!, elasto_visco_plastic_rheology.jl:275-280 (local halo fill of sigma) */
int32_t csi_evp_finalize(csi_context* ctx);
/* time_step_momentum!(model, ::SplitExplicitMomentumEquation, dt), split_explicit_momentum_equations.jl:103-195.
 * rk_reset != 0: reset_velocities! from Psi^- (:89-93). */
int32_t csi_time_step_momentum(csi_context* ctx, double dt, int32_t substeps, int32_t rk_reset);
/* compute_tracer_tendencies!(model), tracer_tendency_kernel_functions.jl:9-45 */
int32_t csi_compute_tracer_tendencies(csi_context* ctx, int32_t scheme);
/* Precision of a WENO scheme's smoothness indicators and nonlinear weights inside csi_compute_tracer_tendencies / the time steppers.
 * CSI_WEIGHTS_F64 (default): everything in double.  CSI_WEIGHTS_F32: the indicators, tau, the ratios, the unnormalised weights and
 * their sum in float on float-converted stencil values; candidates and the final combination in double -- the library's reading
 * of the second float type parameter FT2 (= Float32 by default) that newer Oceananigans versions give WENO{N, FT, FT2, ...}, whose
 * instances the reference only calls (src/sea_ice_advection.jl:51-58).  RECALLED, not verified: the Julia side
 * selects the mode from typeof(model.advection) (julia/ClimaSeaIceHIP.jl weight_dtype), bench/reference_driver.jl dumps that type
 * with its fields so that a reference run shows which mode it was.  Both modes: STRICT equals the oracle bit for bit. */
enum { CSI_WEIGHTS_F64 = 0, CSI_WEIGHTS_F32 = 1 };
int32_t csi_set_weno_weight_dtype(csi_context* ctx, int32_t dtype);
int32_t csi_weno_weight_dtype(csi_context* ctx, int32_t* dtype);
/* dynamic_time_step!(model, dt): sea_ice_fe_step.jl:36-82 (from_cache = 0), sea_ice_rk_substep.jl:134-152 (1) */
int32_t csi_dynamic_step_tracers(csi_context* ctx, double dt, int32_t from_cache);
/* cache_current_fields!(model), sea_ice_rk_substep.jl:29-42 */
int32_t csi_cache_current_fields(csi_context* ctx);
/* update_state!(model), sea_ice_model.jl:379-394: immersed masking + local halo fill of h, aice, u, v.
 * CSI_ERR_UNSUPPORTED ("tile smaller than its halo") where one of these fields could not be filled (csi_fill_halo_local below):
 * refused as a whole, before the mask or any fill has written. */
int32_t csi_update_state(csi_context* ctx);
/* fill_halo_regions!(field; only_local_halos = true) for one bound field (a csi_field_id slot or CSI_F_FREE_DRIFT_U / _V; so
 * csi_halo_exchange).  A halo cell is written only as the image of a point (Periodic wrap, no-flux mirror, ValueBoundaryCondition
 * reflection, north fold; corners as the product of an x image and a y image): cells beyond a side without an image -- Face on a wall,
 * a connected side, the deeper cells of a ValueBoundaryCondition side, and the corner cells whose column lies beyond such an x side --
 * keep what they hold.  One image per side: in a direction where a side of this field wraps or mirrors the grid must be at least as wide
 * as its halo (N >= H; below a north fold Nx >= Hx and Ny >= Hy, Ny >= Hy + 1 for a Center-in-y field) -- CSI_ERR_UNSUPPORTED ("tile
 * smaller than its halo") otherwise, the parent untouched.  A direction whose sides have no image is legal at any N >= 1. */
int32_t csi_fill_halo_local(csi_context* ctx, int32_t field_id);
/* Whole model steps: FE (sea_ice_fe_step.jl:13-34) and the SplitRungeKutta3 stage loop around rk_substep!
 * (sea_ice_rk_substep.jl:81-94).  Without csi_evp_params_set and without csi_dynamics_set(ctx, CSI_DYNAMICS_FREE_DRIFT)
 * (dynamics = nothing) the velocities are prescribed and the momentum step is skipped: advection-only models.  Thermodynamics: csi_slab_params_set / csi_snow_params_set.
 * A grid on which h, aice (with dynamics: u, v) cannot be imaged (csi_fill_halo_local: "tile smaller than its halo") is refused with
 * CSI_ERR_UNSUPPORTED at the entry of the step, before anything is written. */
int32_t csi_time_step_fe(csi_context* ctx, double dt, int32_t substeps, int32_t scheme, int32_t first_iteration);
int32_t csi_time_step_rk3(csi_context* ctx, double dt, int32_t substeps, int32_t scheme);

/* Bare-ice slab thermodynamics with PrescribedTemperature top boundary condition
 * (thermodynamic_time_step.jl:75-118,304-370; slab_thermodynamics_tendencies.jl:28-135). */
typedef struct {
    double conductivity;             /* ConductiveFlux, 2 */
    double sea_ice_density;          /* bulk, 900 */
    double density;                  /* PhaseTransitions.density (pure ice), 917 */
    double liquid_density;           /* 999.8 */
    double liquid_heat_capacity;     /* 4186 */
    double heat_capacity;            /* 2000 */
    double reference_latent_heat;    /* 334e3 */
    double reference_temperature;    /* 0 */
    double liquidus_slope;           /* 0.054 */
    double freshwater_melting_temperature; /* 0 */
    double bottom_salinity;          /* IceWaterThermalEquilibrium salinity, 0 */
    double ice_consolidation_thickness;    /* 0.05 */
    double top_temperature;          /* PrescribedTemperature */
    int32_t top_flux_kind;           /* 0: constant Qu ; 1: internal-flux equilibrium (sea_ice_model.jl:248-256) */
    int32_t bottom_flux_kind;        /* 0: constant Qb ; 1: -(1 - aice) * Qb (examples/freezing_bucket.jl:79-81) */
    double top_heat_flux, bottom_heat_flux;
    /* top boundary condition (slab_thermodynamics_tendencies.jl:107-119).  0: PrescribedTemperature(top_temperature).
     * 1: MeltingConstrainedFluxBalance with a NUMERIC top_heat_flux: the reference's secant solve of
     * Qx - Qi(T) = 0 (top_heat_boundary_conditions.jl:80-97) has, for the linear conductive flux, the closed-form
     * root T = Tb - Qx R (R = h / k, with snow hs / ks + h / k), capped at the melting temperature. */
    int32_t top_bc_kind;
    int32_t pad_;
    double ice_salinity;             /* model.ice_salinity: Tm = melting_temperature(liquidus, S), 0 */
} csi_slab_params;
/* Snow layer on the slab: snow_slab_thermodynamics (slab_sea_ice_thermodynamics.jl:42-49) + snow_density / snowfall
 * of SeaIceModel.  The layered step is _layered_thermodynamic_time_step! (thermodynamic_time_step.jl:131-298); hs is
 * advected and updated like h (tracer_tendency_kernel_functions.jl:49-52, sea_ice_fe_step.jl:86-94) when
 * CSI_F_HS / CSI_F_GHS (/ CSI_F_HSM for RK3) are bound. */
typedef struct {
    double conductivity;             /* 0.31 */
    double snow_density;             /* 330 */
    double snowfall;                 /* kg m^-2 s^-1, constant */
    double top_temperature;          /* PrescribedTemperature of the snow surface (top_bc_kind 0) */
    int32_t top_bc_kind;             /* as csi_slab_params.top_bc_kind, for the snow surface */
    int32_t pad_;
} csi_snow_params;
/* thermodynamic_time_step!(model, ::SlabThermodynamics, ::SlabThermodynamics, dt): needs CSI_F_H, CSI_F_A, CSI_F_HS */
int32_t csi_layered_thermo_step(csi_context* ctx, const csi_slab_params* ice, const csi_snow_params* snow, double dt);
/* With slab parameters set: csi_time_step_fe / _rk3 run the layered step instead of the bare-ice one.  NULL removes it. */
int32_t csi_snow_params_set(csi_context* ctx, const csi_snow_params* p);
int32_t csi_slab_thermo_step(csi_context* ctx, const csi_slab_params* p, double dt);
/* Make csi_time_step_fe / csi_time_step_rk3 run the slab step where the reference does (after the tracer update of
 * every stage: sea_ice_fe_step.jl:28, sea_ice_rk_substep.jl:91).  NULL removes it. */
int32_t csi_slab_params_set(csi_context* ctx, const csi_slab_params* p);

/* ---- per-cell heat fluxes, RadiativeEmission and the surface-temperature solve ---------------------------------------------
 * External heat fluxes as the reference's getflux reads them (SeaIceThermodynamics/HeatBoundaryConditions/boundary_fluxes.jl):
 *   CONSTANT            a Number, `value` (:8)
 *   ARRAY               a 2-D array / Field read at [i, j] (:9-12): the (c,c) array bound to CSI_F_TOP_HEAT_FLUX / _BOTTOM_
 *   RADIATIVE_EMISSION  RadiativeEmission(emissivity, stefan_boltzmann_constant, reference_temperature) (:98-127):
 *                       (eps * sigma) * P at the surface temperature T, P = (T + T_r)^4 evaluated as (x * x) * (x * x) with
 *                       x = T + T_r, uncontracted.  DEPARTURE: Julia's Float64 ^ 4 is a compensated power, so the last bit of P
 *                       may differ from a Julia run.
 * n terms form a Tuple, summed RIGHT-nested as getflux(::Tuple) does (:15-22): t0 + (t1 + (t2 + ...)); n = 1 is the term alone.
 * Rules: at most one ARRAY term per side, RADIATIVE_EMISSION at the top only, n <= CSI_MAX_HEAT_FLUX_TERMS; a side with terms
 * excludes the numeric kinds of csi_slab_params on that side (top_flux_kind 1, the frazil bottom_flux_kind 1: CSI_ERR_UNSUPPORTED).
 * terms == NULL or n == 0 removes a side's terms: that side returns to csi_slab_params' numbers, and with no terms on either side,
 * no per-cell temperature and no snowfall array the thermodynamic steps run exactly the kernels they run without these calls.
 *
 * Where the fluxes enter (thermodynamic_tendency, slab_thermodynamics_tendencies.jl:74-135; _layered_thermodynamic_time_step!,
 * thermodynamic_time_step.jl:131-298): under MeltingConstrainedFluxBalance (top_bc_kind 1) a consolidated cell (h >= h_c) solves
 * Qx(T) - Qi(T) = 0 for the surface temperature, Qi the slab's conductive flux (with snow: resistors in series), caps the root
 * at Tm (the ice's melting temperature; 0 where there is snow) and WRITES it to CSI_F_TU (bare ice) / CSI_F_TUS (snow surface);
 * an unconsolidated cell writes Tb.  Both external fluxes are then evaluated once at that temperature.
 *   - Without an emission term Qx does not depend on T: the root is the closed form Tb - Qx R of the numeric path, Qx per cell.
 *   - With one the secant solve of top_heat_boundary_conditions.jl:82-100, find_zero(f, SecantMethod(Tu- + 1, Tu-)), runs per
 *     consolidated cell from Tu- = the value the bound CSI_F_TU / CSI_F_TUS holds.  RECALLED (RootSolvers is not vendored):
 *         x0 = Tu- + 1; x1 = Tu-; y0 = f(x0); y1 = f(x1)
 *         repeat maxiters times: dx = x1 - x0; dy = y1 - y0; x0 = x1; y0 = y1; x1 = x1 - y1 * dx / dy; y1 = f(x1);
 *                                stop if |x1 - x0| < tol
 *         root = x1 (also when not converged)
 *     tol and maxiters are csi_surface_solve's (defaults 1e-3 and 1000, the recalled SolutionTolerance and maxiters).
 * With a PrescribedTemperature top (top_bc_kind 0) and prescribed_array = 1 the surface temperature is read per cell from
 * CSI_F_TU (bare ice) / CSI_F_TUS (snow) instead of top_temperature.  The arithmetic follows the reference's order without
 * contraction in STRICT and FAST alike.
 *
 * LINEAR (top only, at most one per model): the bulk form the reference's users write into a FluxFunction closure
 * (examples/melting_in_spring.jl:64-73, test/test_energy_conservation.jl:8-13), as data:
 *     Q(T) = (K * (T - Ta)) * w      in exactly this order, uncontracted, STRICT and FAST alike
 *     CSI_WEIGHT_NONE           the product by w is not made
 *     CSI_WEIGHT_CONCENTRATION  w = aice[i, j], the concentration the step starts from
 *     CSI_WEIGHT_ICE_PRESENT    Q = (aice[i, j] == 0) ? 0 : K * (T - Ta)
 * The existing members carry it: `value` = K, `reference_temperature` = Ta, `reserved` = weighting (bits 0-1) |
 * CSI_LINEAR_COEFFICIENT_ARRAY | CSI_LINEAR_REFERENCE_ARRAY.  With the two array flags K and Ta are read per cell from the (c,c)
 * arrays bound to CSI_F_FLUX_COEFFICIENT and CSI_F_FLUX_REFERENCE_TEMPERATURE; both flags or neither (a front end broadcasts the
 * number into an array when only one of the two is per cell).  The term takes its place in the right-nested sum like any other.
 * It makes Qx depend on T: under MeltingConstrainedFluxBalance every consolidated cell runs the secant solve above, exactly as with
 * an emission term (same tol, same maxiters; no closed form is substituted, although f is linear: the solve then ends after at
 * most two updates).  Under PrescribedTemperature the term is evaluated at the prescribed temperature.
 *
 * PER-CELL BOTTOM SALINITY.  With csi_surface_solve.reserved = CSI_SOLVE_BOTTOM_SALINITY_ARRAY both steps form
 * Tb = liq_T0 - liq_slope * S[i, j] from the (c,c) array bound to CSI_F_BOTTOM_SALINITY (IceWaterThermalEquilibrium.salinity read per
 * cell, bottom_heat_boundary_conditions.jl:36-39) instead of csi_slab_params.bottom_salinity.  The ice salinity (Tm) stays a number.
 *
 * THE FLUXES A STEP USED.  Two optional OUTPUT slots, CSI_F_TOP_HEAT_FLUX_USED and CSI_F_BOTTOM_HEAT_FLUX_USED: when bound, the
 * thermodynamic step writes the values it used into their interior -- the bare-ice step its Qu (the internal flux under
 * top_flux_kind 1) and Qb, the layered step Qui (per cell, before the snow-melt partition) and Qbi.  Binding either one selects the
 * flux kernels also for a numeric configuration, which gives the number path's h, aice, hs bit for bit.  Read them after the step
 * (csi_sync, or work queued on the context's stream).  In an RK3 step they hold the last stage's values.
 *
 * The five slots are numbered from CSI_F_COUNT_BINDABLE on, so that every older id and count keeps its value. */
typedef enum { CSI_FLUX_CONSTANT = 0, CSI_FLUX_ARRAY = 1, CSI_FLUX_RADIATIVE_EMISSION = 2, CSI_FLUX_LINEAR = 3,
               CSI_FLUX_SHORTWAVE = 4 /* see csi_shortwave_set */ } csi_heat_flux_kind;
typedef enum { CSI_HEAT_TOP = 0, CSI_HEAT_BOTTOM = 1 } csi_heat_flux_side;
typedef enum { CSI_WEIGHT_NONE = 0, CSI_WEIGHT_CONCENTRATION = 1, CSI_WEIGHT_ICE_PRESENT = 2 } csi_flux_weighting;
#define CSI_LINEAR_WEIGHT_MASK 3
#define CSI_LINEAR_COEFFICIENT_ARRAY 4      /* csi_heat_flux_term.reserved of a LINEAR term: K per cell */
#define CSI_LINEAR_REFERENCE_ARRAY 8        /*                                               Ta per cell */
#define CSI_SOLVE_BOTTOM_SALINITY_ARRAY 1   /* csi_surface_solve.reserved: Tb per cell from CSI_F_BOTTOM_SALINITY */
#define CSI_MAX_HEAT_FLUX_TERMS 8
typedef struct {
    int32_t kind;                      /* csi_heat_flux_kind */
    int32_t reserved;                  /* LINEAR: weighting | array flags (above); 0 otherwise */
    double value;                      /* CONSTANT; LINEAR: K, W m^-2 K^-1 */
    double emissivity;                 /* RADIATIVE_EMISSION: 1 */
    double stefan_boltzmann_constant;  /*                     5.67e-8 */
    double reference_temperature;      /*                     273.15; LINEAR: Ta, in the unit of the surface temperature */
} csi_heat_flux_term;
int32_t csi_heat_fluxes_set(csi_context* ctx, int32_t side, const csi_heat_flux_term* terms, int32_t n);
typedef struct {
    double tol;                        /* the secant's |x1 - x0| tolerance, > 0 (1e-3) */
    int32_t maxiters;                  /* >= 1 (1000) */
    int32_t prescribed_array;          /* 1: PrescribedTemperature per cell, read from CSI_F_TU / CSI_F_TUS */
    int32_t snowfall_array;            /* 1: the layered step reads snowfall per cell from CSI_F_SNOWFALL */
    int32_t reserved;                  /* flags: CSI_SOLVE_BOTTOM_SALINITY_ARRAY; other bits 0 */
} csi_surface_solve;
/* NULL restores the defaults. */
int32_t csi_surface_solve_set(csi_context* ctx, const csi_surface_solve* p);

/* ---- multi-GPU tiles (one process per GPU; RCCL point-to-point over xGMI) ----------------- */
/* Position of this context's tile in an Rx x Ry decomposition of a global grid; the
 * *_CONNECTED topologies passed to csi_grid_set must agree with it. */
int32_t csi_tile_set(csi_context* ctx, int32_t rank_x, int32_t rank_y, int32_t Rx, int32_t Ry,
                     int32_t periodic_x, int32_t periodic_y);
/* 128-byte RCCL unique id produced on rank 0 (csi_comm_unique_id) and broadcast by the host. */
int32_t csi_comm_unique_id(uint8_t* id128);
int32_t csi_comm_init(csi_context* ctx, int32_t world_size, int32_t rank, const uint8_t* id128);
/* Ranks of the context's RCCL communicator as RCCL itself reports them (ncclCommCount; 0 before csi_comm_init): what
 * bench.py prints as `rccl_ranks`, so that a run that silently fell back to one rank cannot report n_gpus > 1. */
int32_t csi_comm_count(csi_context* ctx, int32_t* ranks);

/* In-process tile group: several contexts of ONE process -- one host thread each, normally all on one GPU -- exchange their halos
 * through device-to-device copies instead of RCCL (which refuses two ranks on one device), with RCCL's matching rule (messages
 * between a pair of ranks match in the order they were posted: the same send / receive plans run); the peer halo transport
 * addresses the neighbours' arrays directly.  Host-synchronous, built for correctness runs of real decompositions on a one-GPU
 * machine (tests/test_gpu_local_tiles.py: 2 x 2, 1 x 4 with the fold tile, a Bounded x partition) and for a single process that
 * drives several tiles.  Every context of a group calls the sub-cycle from its own thread; a rank that never arrives makes the
 * others fail with CSI_ERR_COMM after two minutes instead of hanging.  The group outlives its contexts' use of it (destroy it
 * after them).  csi_comm_init_local replaces csi_comm_init (csi_tile_set as usual); csi_comm_count reports the group size.
 * With the peer transport the tiles' kernels wait for each other's flags, so their streams must not share a hardware queue (two
 * streams on one queue run in submission order): set GPU_MAX_HW_QUEUES (default 4) to more than the number of tiles before the
 * HIP runtime initialises. */
typedef struct csi_local_group csi_local_group;
int32_t csi_local_group_create(int32_t world_size, csi_local_group** out);
void csi_local_group_destroy(csi_local_group* group);
int32_t csi_comm_init_local(csi_context* ctx, csi_local_group* group, int32_t rank);
/* Host-channel tile group: the ranks are PROCESSES (one context each, any devices -- in particular several on ONE GPU, where RCCL
 * refuses to form a communicator) that share the POSIX shared-memory segment `shm_name` (e.g. "/csi-<job>"; every rank passes
 * the same name; the name is unlinked once all have joined).  The halo exchanges and the two small collectives of the peer
 * set-up travel over the host and HIP IPC copies; the peer halo transport maps the neighbours' arrays and flag words with
 * hipIpcOpenMemHandle exactly as one process per GPU does under RCCL.  Host-synchronous: for correctness runs, not for speed.
 * Stands where the reference's distributed tests start `mpiexec -n 4` on whatever devices there are
 * (test/test_distributed_sea_ice.jl:41-54). */
int32_t csi_comm_init_host(csi_context* ctx, const char* shm_name, int32_t world_size, int32_t rank);
/* Exchange `width` halo layers of the fields in `field_ids` with the neighbouring tiles. */
int32_t csi_halo_exchange(csi_context* ctx, const int32_t* field_ids, int32_t nfields, int32_t width);

/* Velocity of marginal ice (0 < mass, concentration below minimum_mass / minimum_concentration;
 * split_explicit_momentum_equations.jl:219-228).
 * CSI_FREE_DRIFT_NONE (0, default): `free_drift = nothing`, zero (stress_balance_free_drift.jl:128-129).
 * CSI_FREE_DRIFT_STRESS_BALANCE (1): StressBalanceFreeDrift built on the model's own top / bottom stresses (:61-121,
 *   materialize_free_drift :44-46): exactly one of them must be a SemiImplicitStress, U = U_e - tau / sqrt(C |tau|).
 *   Evaluated once per sub-cycle (or explicit step) into library-owned arrays (it depends on the forcing only).
 * CSI_FREE_DRIFT_FIELDS (2): `free_drift = (u = ..., v = ...)`, the velocity of marginal ice read from two arrays (:123-125; e.g. the
 *   ocean surface velocity of a coupled model): the (f,c) array bound to CSI_F_FREE_DRIFT_U and the (c,f) array bound to
 *   CSI_F_FREE_DRIFT_V, which the kernels read in place (nothing is evaluated or copied per sub-cycle).  Both must be bound when a
 *   momentum step runs (CSI_ERR_NOT_BOUND, by name); no SemiImplicitStress is needed.  Their halos are the library's to fill, like
 *   those of the stress arrays at the same locations: csi_time_step_momentum fills them locally (periodic wrap, walls, the north
 *   fold with the sign change of a vector component) and exchanges them between tiles before the velocities are stepped
 *   (csi_evp_subcycle called on its own does not, as for the stress arrays: csi_fill_halo_local / csi_halo_exchange first).
 * Every momentum path reads the same two arrays: the EVP three-kernel paths, the fused kernels, the fold band, tiles on either
 * transport, the viscous sub-cycle and the ExplicitSolver. */
typedef enum { CSI_FREE_DRIFT_NONE = 0, CSI_FREE_DRIFT_STRESS_BALANCE = 1, CSI_FREE_DRIFT_FIELDS = 2 } csi_free_drift_kind;
int32_t csi_free_drift_set(csi_context* ctx, int32_t kind);

/* The model's dynamics.
 * CSI_DYNAMICS_MOMENTUM_EQUATION (0, default): a SeaIceMomentumEquation -- rheology, solver and free drift as set by the calls
 *   above and below; nothing changes.
 * CSI_DYNAMICS_FREE_DRIFT (1): `dynamics = StressBalanceFreeDrift(top_momentum_stress, bottom_momentum_stress)`, the free-drift
 *   velocity as the model's WHOLE dynamics (AbstractFreeDriftDynamics, stress_balance_free_drift.jl:131-151).  A momentum step is
 *   ONE launch over i = 1 .. Nx, j = 1 .. Ny that sets u[i, j] = free_drift_u, v[i, j] = free_drift_v (:61-109) at EVERY point:
 *   no mass or concentration select, no `* active` factor, no dependence on the current u, v, on dt, on substeps or on rk_reset;
 *   the stores also write the local halo images of u and v (periodic wrap, no-flux mirror, ValueBoundaryCondition, north fold), so
 *   no fill launch follows.  STRICT and FAST run the same arithmetic (the reference's operation order) and are bit-identical.
 *   Needs CSI_F_U, CSI_F_V, the grid (halo >= 1) and the two csi_stress_set stresses: exactly one of them a SemiImplicitStress
 *   (rho_e, C_D, u_e / v_e zero, numbers or the bound arrays), the other one nothing, a number pair or the two bound arrays;
 *   otherwise CSI_ERR_INVALID_ARGUMENT with the reference's wording (:24-32).  NOT read: the ten EVP slots, h, aice, CSI_F_GU /
 *   CSI_F_GV, csi_evp_params_set (not needed at all here: such a model has dynamics without it), csi_rheology_set,
 *   csi_momentum_solver_set, csi_free_drift_set, csi_set_fusion.  csi_time_step_momentum, csi_time_step_fe, csi_time_step_rk3,
 *   csi_update_state and csi_compute_momentum_tendencies (a no-op: SeaIceDynamics.jl:41) work; u and v are prognostic (Psi^- copies
 *   under RK3, masked and halo-filled by update_state! as for any dynamics).  Runs on tiles (the stress arrays' halos are exchanged
 *   first, the step itself needs no exchange: its four-point averages reach one cell; u, v beyond a connected side are
 *   update_state!'s to exchange, as in the reference, whose free-drift step fills no halos at all -- csi_time_step_fe / _rk3 do so at
 *   the end of every stage, after csi_time_step_momentum called on its own call csi_update_state) and on the north fold.
 *   Wall faces and immersed faces are written like any other point, as by the ExplicitSolver's velocity launches; the values the
 *   local fill and update_state! then leave there are recalled fill semantics, not pinned. */
typedef enum { CSI_DYNAMICS_MOMENTUM_EQUATION = 0, CSI_DYNAMICS_FREE_DRIFT = 1 } csi_dynamics_kind;
int32_t csi_dynamics_set(csi_context* ctx, int32_t kind);

/* ---- forcing time series interpolated at the model clock ---------------------------------------------------------------------------
 * The reference treats time-dependent forcing as part of the model: update_state! ends with update_model_field_time_series!(model,
 * clock) (sea_ice_model.jl:391-408) and its kernels read a FieldTimeSeries at Time(clock.time) (thermodynamic_time_step.jl:326-329).
 * Here a series drives one of ELEVEN slots of csi_field_bind: CSI_F_TOP_U / _V, CSI_F_BOT_U / _V (stress arrays or external
 * velocities), CSI_F_FORCING_U / _V, CSI_F_FREE_DRIFT_U / _V, CSI_F_TOP_HEAT_FLUX, CSI_F_BOTTOM_HEAT_FLUX, CSI_F_SNOWFALL.
 * Three thermodynamic inputs joined the eleven, fourteen in all: CSI_F_FLUX_COEFFICIENT, CSI_F_FLUX_REFERENCE_TEMPERATURE and
 * CSI_F_BOTTOM_SALINITY (csi_heat_fluxes_set); they ride in the same launch.  So do the mixed layer's four inputs (csi_mixed_layer_set:
 * CSI_F_ML_SURFACE_HEAT_FLUX, CSI_F_ML_COEFFICIENT, CSI_F_ML_REFERENCE_TEMPERATURE, CSI_F_ML_DEEP_HEAT_FLUX), eighteen in all, and the
 * SHORTWAVE term's flux (csi_shortwave_set: CSI_F_SHORTWAVE), nineteen.
 * csi_time_series_update(ctx, t) interpolates every series in ONE launch, in place, into the INTERIOR of the arrays bound to those
 * slots -- the arrays the momentum and thermodynamic kernels already read; no kernel of theirs changes.  The halos of the
 * velocity-point slots stay the library's to fill where it fills them for plain arrays (csi_time_step_momentum; csi_free_drift_set).
 *
 * Time indexing (csi_time_series_plan; pure host function, no context, no GPU).  times: strictly increasing, nt >= 2.  Output: 0-based
 * slice indices n1, n2 and the weight frac; the interpolated value is
 *     psi = (n1 == n2) ? psi_1 : psi_2 * frac + psi_1 * (1 - frac)          (two products, one sum, uncontracted; STRICT and FAST alike)
 *   CSI_TIME_CLAMP:    t <= times[0] / t >= times[nt-1]: the end slice (n1 == n2, frac 0).  Inside: n1 the last node at or below t,
 *                      n2 = n1 + 1, frac = (t - times[n1]) / (times[n2] - times[n1]); at a node n1 == n2, frac 0.
 *   CSI_TIME_LINEAR:   as CLAMP inside and at the two end nodes; beyond them it extrapolates from the first (0, 1) / last (nt-2, nt-1)
 *                      two slices with the same formula, so frac < 0 / frac > 1.
 *   CSI_TIME_CYCLICAL: period <= 0 means "infer": times[nt-1] - times[0] + (times[nt-1] - times[nt-2]); a given period must exceed
 *                      times[nt-1] - times[0].  t' = times[0] + r, r = fmod(t - times[0], period), plus period if r < 0.  t' inside
 *                      the nodes: as CLAMP.  In the gap behind the last node: n1 = nt-1, n2 = 0,
 *                      frac = (t' - times[nt-1]) / (period - (times[nt-1] - times[0])).
 * Invalid input (nt < 2, times not strictly increasing, an unknown kind, a period that is too short, a time that is not finite):
 * CSI_ERR_INVALID_ARGUMENT.  STATUS: Oceananigans is not vendored; these rules (its Clamp / Cyclical / Linear time indexing), the
 * inferred period and the interpolation formula are RECALLED, like the fold and the secant solve above.  This statement is the
 * definition; tests/time_series_ref.py restates it and tests/test_time_series_plan.py pins the library to it bit for bit. */
typedef enum { CSI_TIME_CLAMP = 0, CSI_TIME_CYCLICAL = 1, CSI_TIME_LINEAR = 2 } csi_time_indexing;
int32_t csi_time_series_plan(const double* times, int32_t nt, int32_t indexing, double period, double t,
                             int32_t* n1, int32_t* n2, double* frac);
/* CSI_SERIES_DEVICE: `data` is a DEVICE pointer to all nt slices; the caller keeps it alive; nothing is copied.
 * CSI_SERIES_HOST:   `data` is a HOST pointer to all nt slices (pageable or page-locked), which the caller keeps alive.  The library
 *   keeps `window` slices (>= 2; 0 selects the default, 3) in a device ring of its own and uploads slices on a copy stream of its own:
 *   the two an update needs if they are not resident, and the slice that time moving forward needs next.  That look-ahead is issued
 *   at the END of the next entry point that advances the model (csi_time_step_momentum, csi_time_step_fe / _rk3, csi_update_state),
 *   once its launches are queued -- by the next csi_time_series_update or _status at the latest --, so that the host's staging copy
 *   and the transfer both run under that step.  Residency is a table (ring slot -> slice); a slot is evicted only if
 *   neither current index uses it.  Any time is legal: jumps forward or backward (a restored checkpoint), a first call in the middle.
 *   No call waits for the device; the host copies a PAGEABLE slice into page-locked staging memory first (one staging slice per ring
 *   slot, rewritten only after the copy that last read it has completed).
 * Slices have the shape of the slot's field's INTERIOR: parent extents minus halos (so a Face field on a Bounded side is one wider);
 * rows are `ld` doubles apart, slices `slice_stride` doubles apart.  `times` is copied. */
typedef enum { CSI_SERIES_DEVICE = 0, CSI_SERIES_HOST = 1 } csi_series_backend;
typedef struct {
    int32_t nt;              /* slices, >= 2 */
    int32_t indexing;        /* csi_time_indexing */
    int32_t backend;         /* csi_series_backend */
    int32_t window;          /* HOST: slices of the device ring */
    double period;           /* CYCLICAL: <= 0 infers it */
    const double* times;     /* host, nt values */
    const void* data;        /* nt slices: device (DEVICE) or host (HOST) memory */
    int64_t ld;              /* doubles between rows */
    int64_t slice_stride;    /* doubles between slices */
} csi_time_series;
/* Set (or, ts == NULL, remove) the series of one slot.  Any slot but these nineteen: CSI_ERR_INVALID_ARGUMENT.  The slot's field must be
 * bound (CSI_ERR_NOT_BOUND): the series writes into that array.  Setting a slot again replaces its series (empty window, zero uploads). */
int32_t csi_time_series_set(csi_context* ctx, int32_t field_id, const csi_time_series* ts);
/* Interpolate every series at `time` into its bound array, one launch on the context's stream (no series: nothing is launched, CSI_OK).
 * The Python / Julia front ends call it with the model clock at the start of time_step!, time_step_momentum!,
 * compute_momentum_tendencies! and update_state!: all stages of a step read the forcing at the time the step starts from, as in the
 * reference, whose tick! follows the stages. */
int32_t csi_time_series_update(csi_context* ctx, double time);
/* For tests and profiles: resident[k] = the slice ring slot k holds (-1: none), k < window (HOST; DEVICE: nothing is written), and the
 * slice uploads since csi_time_series_set.  Either pointer may be NULL. */
int32_t csi_time_series_status(csi_context* ctx, int32_t field_id, int32_t* resident, int64_t* uploads);

/* ---- forcing time series on a source grid of their own: regridded on the device -------------------------------------------------
 * A series may be given on a RECTILINEAR source grid -- 1-D x nodes and 1-D y nodes in the coordinates of the model grid's nodes
 * (degrees of longitude / latitude on a latitude-longitude or tripolar grid); x may be periodic -- instead of on the model grid.  At
 * every csi_time_series_update ONE further launch (k_time_series_regrid, time_series_regrid.hip) serves all such slots: per target
 * point it interpolates in time at the four surrounding source points, then bilinearly in space, rotates one component of a vector
 * pair into the grid's local axes and writes the interior of the bound array.  Series on the model grid keep k_time_series.
 *
 * Per-axis rule (csi_regrid_plan_axis; pure host function, no context, no GPU): csi_time_series_plan (above) applied to space, and
 * implemented by calling it.  nodes: n >= 2 values, strictly increasing and finite; x finite; otherwise CSI_ERR_INVALID_ARGUMENT.
 *   periodic == 0: the CSI_TIME_CLAMP paragraph with times := nodes, t := x -- the end node outside the nodes, i0 == i1 and w = 0 at
 *                  a node and beyond the ends (`period` is ignored);
 *   periodic != 0: the CSI_TIME_CYCLICAL paragraph -- period <= 0 is inferred, a given one must exceed nodes[n-1] - nodes[0]; x is
 *                  wrapped with fmod from nodes[0]; in the gap behind the last node i0 = n-1, i1 = 0,
 *                  w = (x' - nodes[n-1]) / (period - (nodes[n-1] - nodes[0])).
 * Output: 0-based i0, i1 and the weight w of node i1, 0 <= w < 1.
 *
 * Value per target point.  a_k, b_k: the source values of the two slices around the clock at corner k; w1, w2, same_t: the weights of
 * k_time_series (w2 = frac, w1 = 1 - frac, formed on the host; same_t: n1 == n2).  Every line is two products and one sum,
 * uncontracted, in this order; STRICT and FAST are the same code:
 *     c_k  = same_t ? a_k : b_k * w2 + a_k * w1          k = 00, 10, 01, 11; c10 is the corner at (i1, j0)
 *     lo   = c10 * wx + c00 * (1 - wx)
 *     hi   = c11 * wx + c01 * (1 - wx)
 *     val  = hi  * wy + lo  * (1 - wy)
 * 1 - wx and 1 - wy are formed in the kernel.  Vector pair: a slot at (Face, Center) that is the x component of a pair forms val_E
 * and val_N from the pair's two source series (each with ITS time weights) at its own point and writes val_E * cos + val_N * sin; a
 * slot at (Center, Face) that is the y component writes val_N * cos - val_E * sin at its own point.  cos, sin: per-point arrays of the
 * map, the bearing of the grid's x direction against east.
 * Source values must be FINITE: a weight may be exactly 0, and 0 * Inf or 0 * NaN is NaN -- filling or masking the source
 * (land points of an ocean product) is the caller's responsibility.
 *
 * A map (csi_regrid_map_create) is made for ONE location of the context's grid or tile: its interior extents nx, ny (a Face field on a
 * Bounded side is one wider) and, per interior point, row-major and packed (point (i, j) at [j * nx + i]), the four 0-based source
 * indices, the two weights and optionally cos and sin (both or neither; a vector pair needs them).  The library validates the extents
 * against the grid, every index against the source extents and 0 <= w <= 1 (cos, sin: finite), and copies the map to the device; the
 * caller's arrays are not needed after the call.  DEVICE LAYOUT, stated because it sets the limits and the traffic: three planes of
 * 8-byte entries per point -- the four indices as uint16 {i0, i1, j0, j1}, wx, wy -- and two more (cos, sin) for a map with rotation:
 * 24 or 40 bytes per point, read with 16-byte loads (two points at a time), rows padded so that a pair of points that is 16-byte
 * aligned in the destination is 16-byte aligned in every plane.  Hence src_nx, src_ny <= 65536 (CSI_REGRID_MAX_SOURCE_EXTENT).
 * Compulsory memory traffic per update and point: the map plus the 8-byte store, 32 bytes (scalar) or 48 bytes (vector component);
 * the gathers (8 or 16 per point, 8 bytes each) go to a source slice that is small and shared by every workgroup.
 * At most CSI_REGRID_MAX_MAPS (16) maps per context live at a time; csi_context_destroy frees them.  csi_regrid_map_destroy refuses a
 * map that a slot still uses (CSI_ERR_INVALID_ARGUMENT).  csi_grid_set / csi_tile_set after a map was made leave it as it is: a slot
 * set on it later is refused if the extents no longer match.
 *
 * NOT BUILT: conservative or higher-order remapping; curvilinear source grids; extrapolation beyond the clamp (and the front end's
 * fill_missing); reading files; a per-slice source mask; rotation of pairs at (Center, Center). */
int32_t csi_regrid_plan_axis(const double* nodes, int32_t n, int32_t periodic, double period, double x,
                             int32_t* i0, int32_t* i1, double* w);
typedef enum { CSI_REGRID_FACE_CENTER = 0, CSI_REGRID_CENTER_FACE = 1, CSI_REGRID_CENTER_CENTER = 2 } csi_regrid_location;
enum { CSI_REGRID_MAX_MAPS = 16, CSI_REGRID_MAX_SOURCE_EXTENT = 65536 };
typedef struct {
    int32_t location;        /* csi_regrid_location of the target points */
    int32_t nx, ny;          /* target interior extents */
    int32_t src_nx, src_ny;  /* source extents, each 2 .. CSI_REGRID_MAX_SOURCE_EXTENT */
    int32_t reserved;        /* 0 */
    const int32_t* i0;       /* host arrays of ny * nx entries each */
    const int32_t* i1;
    const int32_t* j0;
    const int32_t* j1;
    const double* wx;
    const double* wy;
    const double* cos;       /* NULL (with sin): a map without rotation */
    const double* sin;
} csi_regrid_map;
int32_t csi_regrid_map_create(csi_context* ctx, const csi_regrid_map* desc, int32_t* map_id);
int32_t csi_regrid_map_destroy(csi_context* ctx, int32_t map_id);
/* Set a REGRIDDED series on one of the nineteen slots of csi_time_series_set.  ts: a series whose slices have the SOURCE shape
 * (src_ny rows of src_nx values; ld, slice_stride as before); both backends -- the HOST ring holds source-sized slices.  other == NULL:
 * a scalar (component must be 0).  Otherwise ts is the EAST series and other the NORTH series of a vector pair (one ring each on the
 * HOST backend; the two may have different times), component 0: the slot receives the x component and must lie at (Face, Center),
 * 1: the y component, at (Center, Face).  map_id: a map made for the slot's location, with the source extents of the series; a
 * source slice spans fewer than 2^31 doubles (ld * src_ny: the kernel forms 32-bit offsets).
 * Setting a slot replaces whichever kind of series it had; csi_time_series_set(ctx, slot, NULL) removes either kind.  A slot whose
 * bound array has changed its row stride or alignment since: csi_time_series_update fails; set the slot again. */
int32_t csi_time_series_set_regridded(csi_context* ctx, int32_t field_id, const csi_time_series* ts, int32_t map_id,
                                      const csi_time_series* other, int32_t component);
/* For tests: launches of k_time_series_regrid so far (a context without regridded slots never launches it; one per update with any
 * number of them) and the maps alive.  Either pointer may be NULL.  csi_time_series_status serves regridded slots too (a pair: the
 * east series). */
int32_t csi_regrid_stats(csi_context* ctx, int64_t* launches, int32_t* maps);

/* ---- device diagnostics: advection timescale, integrals, extrema, finite check ------------------------------------------------------
 * Scalars computed from the bound fields ON THE DEVICE, in two launches on the context's stream (a pass over the interior that
 * leaves one partial record per block of 64 x 64 cells, and one block that folds the records), followed by a copy of the 21 result
 * slots to page-locked host memory and a wait for the stream: no field crosses the bus.  Stands where the reference's root module has
 * cell_advection_timescale(model::SeaIceModel) (src/ClimaSeaIce.jl:63-69) and where its tests and validation scripts reduce fields on
 * the host (maximum(u), volume closure, progress lines).  No atomics, no flags, no hand-off between workgroups inside a launch: the
 * results -- the sums included -- are the same bits from call to call, in STRICT and in FAST mode (one code, compiled without
 * contraction), on every device.
 *
 * `what` is a mask of the groups below; only the arrays of a requested group are read, and each of them once, at i = 1 .. Nx,
 * j = 1 .. Ny (halo elements are never read, so whatever they hold -- NaN, stale images -- changes nothing).
 *
 * CSI_DIAG_VELOCITY (needs CSI_F_U, CSI_F_V; 16 B per cell):
 *   inv_timescale_max   max over i = 1 .. Nx, j = 1 .. Ny of (|u[i, j]| / dx^fc(i, j)) + (|v[i, j]| / dy^cf(i, j)): Oceananigans'
 *                       cell_advection_timescale^ccc with w = ZeroField, before its reciprocal.  STATUS: the formula is RECALLED --
 *                       Oceananigans is not vendored; this statement is the definition.
 *   advection_timescale 1 / inv_timescale_max, one division on the host: equal to the minimum over the cells of the per-cell
 *                       reciprocals (IEEE division is monotone); +Inf for ice at rest; 0 when a velocity of some cell is infinite; NaN
 *                       if and only if nan_u + nan_v > 0, as Julia's `minimum` propagates NaN (the device maxima themselves skip NaN).
 *   max_abs_u, max_abs_v  over each field's OWN interior: a Bounded x direction has Nx + 1 u faces, a Bounded y direction Ny + 1 v
 *                       faces.  (Those last faces enter the maxima and the counts; they belong to no cell's timescale.)
 *   nonfinite_u, nonfinite_v   elements of that interior that are NaN or +-Inf;  nan_u, nan_v: those that are NaN.
 * CSI_DIAG_TRACERS (needs CSI_F_H, CSI_F_A; reads CSI_F_HS if bound and the mask if set):
 *   over ACTIVE cells (every interior cell without a mask; mask byte != 0 with one):
 *   ice_volume = sum (h * aice) * Az     ice_area = sum aice * Az     ice_extent = sum Az over cells with aice >= extent_threshold
 *   snow_volume = sum (hs * aice) * Az   active_area = sum Az         (Az = Az^cc; products in the order written, uncontracted)
 *   min_h, max_h, min_aice, max_aice, max_hs   (no active cell: +Inf for a minimum, -Inf for a maximum; NaN elements are skipped;
 *                                               -0.0 and +0.0 compare equal and either may be returned when both occur)
 *   active_cells        their number
 *   over ALL interior cells, land included:  nonfinite_h, nonfinite_aice, nonfinite_hs.
 * Members of a group that was not requested -- and snow_volume, max_hs, nonfinite_hs without a bound CSI_F_HS (has_snow = 0) -- hold
 * the "not computed" values: NaN for a double, -1 for a count.
 *
 * SUMMATION ORDER (part of the interface; a function of (Nx, Ny) alone).  Blocks: nbx = ceil(Nx / 64), nby = ceil(Ny / 64); block
 * (bx, by) owns columns 64 bx + 1 .. 64 bx + 64 and rows 64 by + 1 .. 64 by + 64; a cell beyond Nx or Ny, and an inactive cell,
 * contributes the term +0.0.  With t(tx, row) the term of the block's column tx (0 .. 63) and row (0 .. 63):
 *   1. thread (tx, ty), ty = 0 .. 3:  s = +0.0; s = s + t(tx, ty); s = s + t(tx, ty + 4); ...; s = s + t(tx, ty + 60)   (sixteen rows, ascending)
 *   2. wave ty (its 64 threads, lane = tx): for off = 32, 16, 8, 4, 2, 1: s[lane] = s[lane] + s[lane xor off], all lanes at once
 *   3. block: S = s_wave0; S = S + s_wave1; S = S + s_wave2; S = S + s_wave3.  This is record r = by * nbx + bx.
 *   4. finishing block, thread t = 0 .. 255: s = +0.0; s = s + record[t]; s = s + record[t + 256]; ... (ascending, while < nbx * nby);
 *      then step 2 within each of its four waves (lane = t mod 64, wave = t / 64) and step 3.
 * Maxima, minima and counts take the same route with max, min and integer addition in place of +.
 *
 * Tiled contexts: the call is COLLECTIVE -- every rank of the decomposition calls it between the same two steps, with the same
 * arguments.  Each rank reduces its own interior (the interiors partition the global grid; the easternmost tile of a Bounded x
 * direction owns the faces i = Nx + 1, the northernmost of a Bounded y direction the faces j = Ny + 1), the ranks all-gather their
 * 21 slots over whatever joins them (RCCL communicator, in-process group, host-channel group) and EVERY rank combines them on the
 * host in rank order: a sum is S = slot_rank0; S = S + slot_rank1; ..., maxima / minima by max / min, counts added -- all ranks
 * return the same bits.  A rank that fails locally still takes part in the all-gather; then every rank returns an error.  Sums of a
 * tiled run differ from the untiled run's by rounding only (another tree over the same terms).
 *
 * Errors: CSI_ERR_NOT_BOUND naming the missing field of a requested group (u, v; h, aice); CSI_ERR_INVALID_ARGUMENT for what == 0 or
 * an unknown bit of `what`, and for an extent_threshold that is negative or not finite. */
#define CSI_DIAG_VELOCITY 1
#define CSI_DIAG_TRACERS 2
#define CSI_DIAG_ALL 3
typedef struct {
    int32_t what;                  /* echo of the request */
    int32_t has_snow;              /* 1: CSI_F_HS was bound and read */
    double advection_timescale, inv_timescale_max, max_abs_u, max_abs_v;
    int64_t nonfinite_u, nonfinite_v, nan_u, nan_v;
    double ice_volume, ice_area, ice_extent, snow_volume, active_area;
    double min_h, max_h, min_aice, max_aice, max_hs;
    int64_t nonfinite_h, nonfinite_aice, nonfinite_hs, active_cells;
    double extent_threshold;       /* echo */
} csi_diagnostics;
int32_t csi_diagnostics_compute(csi_context* ctx, int32_t what, double extent_threshold, csi_diagnostics* out);

/* ---- device-side output: packed snapshots, time averages, asynchronous copies ----------------------------------------------------------
 * Stands where the reference attaches an output writer to a Simulation (examples/ice_advected_by_anticyclone.jl:161-163: JLD2Writer
 * with IterationInterval(5); test/distributed_tests_utils.jl:159; test/test_netcdf_writer.jl).  An OUTPUT SET is a list of up to
 * CSI_OUTPUT_MAX_FIELDS bound fields (any slot of csi_field_bind).  csi_output_snapshot packs the INTERIOR of every field of the set
 * into one record in device memory with ONE launch on the context's stream and copies the record to page-locked host memory on a
 * copy stream of the library's own; it returns without waiting for the device, and the stepping goes on while the record crosses
 * the bus.  csi_output_accumulate adds the fields marked `averaged` into accumulators the library owns, so that a time average
 * never leaves the device before it is complete.  Nothing of this changes any other entry point: a context without output sets runs
 * exactly the launches it ran before.
 *
 * RECORD LAYOUT (a function of the field list and the grid alone; csi_output_plan_layout is the same rule as a pure host function).
 *   Field k of the set is a dense row-major (ny_k, nx_k) array of its OWN interior: nx_k = ni - 2Hx, ny_k = nj - 2Hy of the bound
 *   parent, i.e. Nx x Ny, one more column for a Face-in-x field whose high x side is Bounded, one more row for a Face-in-y field whose
 *   high y side is Bounded.  Halos are not part of it and are never read.  On a tile this is the ownership rule of the diagnostics:
 *   only the easternmost / northernmost tile of a Bounded direction has (and writes) the last face, and the interiors of the tiles
 *   partition the global field.  Element (i, j) of the field (1-based) sits at row j - 1, column i - 1.
 *   Elements are 8 bytes (CSI_OUT_F64) or 4 bytes (CSI_OUT_F32).  byte_offset_0 = 0; byte_offset_{k+1} = byte_offset_k + the bytes of
 *   field k, rounded up to a multiple of 256; record_bytes = the same expression behind the last field.  Padding bytes are undefined.
 * ELEMENTS.
 *   snapshot field   x, the array's element
 *   averaged field   acc / W: one IEEE division (no reciprocal) of the accumulator by the sum of the weights W = ((w_1 + w_2) + ...)
 *                    formed on the host in double; acc = ((+0.0 + (x_1 * w_1)) + (x_2 * w_2)) + ..., each product rounded before it
 *                    is added (no contraction).  The pack launch sets acc back to +0.0 and the call sets W back to 0.
 *   masked           a field with masked != 0 takes fill_value in the cells whose mask byte is 0, if a mask is set (csi_mask_set) at
 *                    the time of the snapshot.  (Center, Center) fields only; any other location: CSI_ERR_INVALID_ARGUMENT.
 *   CSI_OUT_F32      the value above converted to fp32, round to nearest even: overflow gives +-Inf, subnormal results are kept, the
 *                    sign of zero is kept, NaN stays NaN (its payload is not specified).
 * One code serves STRICT and FAST, compiled without contraction: both modes give the same bits.
 *
 * SLOTS.  A set has `slots` staging records on the device and as many in page-locked host memory.  csi_output_snapshot takes the free
 * slot with the lowest number (free -> in flight), queues the pack launch on the context's stream, records an event, makes the copy
 * stream wait for it, queues ONE device-to-host copy of the record and records the slot's event behind it.  Steps queued after the call
 * may overwrite the fields: the record is the state at the point of the call.  csi_output_test / csi_output_wait look at / wait for
 * that slot's event ONLY -- never for the context's stream --; after csi_output_wait, host_ptr points to record_bytes bytes that stay
 * valid until csi_output_release (in flight -> free).  With no free slot csi_output_snapshot fails (CSI_ERR_INVALID_ARGUMENT, "no
 * free slot"), changes nothing -- accumulators and W included -- and never overwrites a record that has not been released.  A slot is
 * reused only after its release, which follows its wait, so no further ordering between a pack launch and the previous copy out of
 * the same slot is needed.
 *
 * Errors: CSI_ERR_NOT_BOUND naming the field of the list that is not bound; CSI_ERR_INVALID_ARGUMENT for an unknown dtype or field id,
 * n outside 1 .. CSI_OUTPUT_MAX_FIELDS, slots outside 1 .. CSI_OUTPUT_MAX_SLOTS, a fifth set on a context, a bad handle, field
 * index or slot, a slot that is not in flight, a weight that is not finite and > 0, and csi_output_snapshot of a set with averaged
 * fields while W == 0.  Binding another array (or shape) to a field of a set, or calling csi_grid_set, after csi_output_create
 * INVALIDATES the set: every later call on it but csi_output_destroy fails with CSI_ERR_INVALID_ARGUMENT and says so.
 * csi_context_destroy frees the sets.  Tiled contexts: nothing here communicates; every rank packs its own interior. */
#define CSI_OUT_F64 0
#define CSI_OUT_F32 1
#define CSI_OUTPUT_MAX_FIELDS 16
#define CSI_OUTPUT_MAX_SETS 4
#define CSI_OUTPUT_MAX_SLOTS 64
typedef struct {
    int32_t field_id;              /* a slot of csi_field_bind */
    int32_t dtype;                 /* CSI_OUT_F64 | CSI_OUT_F32 */
    int32_t averaged;              /* 0: snapshot of the field, 1: time average (csi_output_accumulate) */
    int32_t masked;                /* 1: fill_value in inactive cells ((Center, Center) fields only) */
    double fill_value;
} csi_output_field;
/* The layout rule above for n fields of interior extents nx[k] x ny[k] and dtypes dtype[k]: byte_offsets[k] and *record_bytes.  Pure
 * host function (no context, no GPU).  Either output pointer may be NULL. */
int32_t csi_output_plan_layout(const int32_t* nx, const int32_t* ny, const int32_t* dtype, int32_t n, int64_t* byte_offsets,
                               int64_t* record_bytes);
/* handle: 1 .. CSI_OUTPUT_MAX_SETS.  Allocates the staging slots, the accumulators (zeroed) and, the first time on a context, the
 * copy stream. */
int32_t csi_output_create(csi_context* ctx, const csi_output_field* fields, int32_t n, int32_t slots, int32_t* handle);
int32_t csi_output_layout(csi_context* ctx, int32_t handle, int32_t k, int64_t* byte_offset, int32_t* nx, int32_t* ny);
int32_t csi_output_record_bytes(csi_context* ctx, int32_t handle, int64_t* bytes);
/* acc = acc + (x * w) for every averaged field, one launch on the context's stream (none if no field is averaged); W = W + w. */
int32_t csi_output_accumulate(csi_context* ctx, int32_t handle, double w);
int32_t csi_output_snapshot(csi_context* ctx, int32_t handle, int32_t* slot);
int32_t csi_output_test(csi_context* ctx, int32_t handle, int32_t slot, int32_t* done);
int32_t csi_output_wait(csi_context* ctx, int32_t handle, int32_t slot, void** host_ptr);
int32_t csi_output_release(csi_context* ctx, int32_t handle, int32_t slot);
/* Waits for the context's stream and the copy stream, then frees the set; its handle may be handed out again. */
int32_t csi_output_destroy(csi_context* ctx, int32_t handle);

/* ---- derived fields and energy budget integrals ---------------------------------------------------------------------------------------
 * What sea-ice dynamics runs are looked at through, computed on the device from the bound state: deformation maps (divergence, shear,
 * total deformation -- the strain-rate invariants _compute_evp_viscosities! forms and drops, elasto_visco_plastic_rheology.jl:247-260),
 * the ice speed, the stress state relative to the yield curve, the stress power, and the three sums of the reference's discrete energy
 * budget (test/test_rheology_energy_budget.jl:77-88).  Nothing here changes another entry point: a context that never makes these
 * calls launches exactly what it launched before.  One code serves STRICT and FAST, compiled without contraction, IEEE division and
 * square root: both modes give the same bits (tests/derived_ref.py restates every formula below in NumPy).
 *
 * DERIVED FIELDS.  Seven further (c,c) slots of csi_field_bind, numbered from CSI_F_COUNT_TOTAL on so that every older id and count keeps
 * its value.  The caller binds (Center, Center) parents to the slots it wants; csi_derived_compute(ctx, mask) fills the INTERIOR
 * i = 1 .. Nx, j = 1 .. Ny of every requested one in ONE launch on the context's stream (no atomics, no flags, no wait; their halos are
 * never written).  mask: bit (slot - CSI_F_D_DIVERGENCE), i.e. the CSI_DERIVED_* values.  With the reference's operators, in the
 * operation order of the library's strict-order kernels (csrc/evp_strict.hip; oracle/csi_oracle.c):
 *   e11 = strain_rate_xx(i, j), e22 = strain_rate_yy(i, j)              (elasto_visco_plastic_rheology.jl:365-375)
 *   e12(p, q) = strain_rate_xy at the corner (p, q), p = i, i + 1, q = j, j + 1
 *   Ixy(f) = ((f(i, j) + f(i + 1, j)) / 2 + (f(i, j + 1) + f(i + 1, j + 1)) / 2) / 2      (the order of epsilon12^ccc, :250)
 *   DIVERGENCE   = e11 + e22
 *   SHEAR        = sqrt((e11 - e22) * (e11 - e22) + 4 * (e12c * e12c)),  e12c = Ixy(e12)      (the reference's s^ccc, :259)
 *   DEFORMATION  = sqrt(DIVERGENCE * DIVERGENCE + SHEAR * SHEAR)      (defined here: NOT the reference's Delta, which carries e^-2 and a floor)
 *   SPEED        = sqrt(uc * uc + vc * vc),  uc = (u[i, j] + u[i + 1, j]) / 2,  vc = (v[i, j] + v[i, j + 1]) / 2
 *   stress group (needs CSI_F_S11, CSI_F_S22, CSI_F_S12, CSI_F_P: an EVP model; otherwise CSI_ERR_NOT_BOUND naming sigma11):
 *   SIGMA_I      = ((sigma11 + sigma22) / 2) / P
 *   SIGMA_II     = sqrt(((sigma11 - sigma22) / 2) * ((sigma11 - sigma22) / 2) + s12c * s12c) / P,  s12c = Ixy(sigma12)
 *                  P is the bound CSI_F_P as it stands -- the strength the stresses were relaxed against at the last momentum step --,
 *                  not recomputed from h and aice.  Where P == 0 both are +0.0.
 *   STRESS_POWER = (sigma11 * e11 + sigma22 * e22) + 2 * Ixy(sigma12 * e12)      (each corner's product rounded before the average)
 *   sigma12 is read as stored (no immersed conditional).  With a mask set (csi_mask_set) inactive centres receive +0.0 in every field.
 * HALO ELEMENTS READ (the entry point fills none): u at columns 1 .. Nx + 1, rows 0 .. Ny + 1; v at columns 0 .. Nx + 1, rows
 * 1 .. Ny + 1; sigma12 at columns 1 .. Nx + 1, rows 1 .. Ny + 1; sigma11, sigma22, P at the interior only; the mask at the interior
 * only.  On a Bounded high side column Nx + 1 / row Ny + 1 of a Face field is its last face, elsewhere the first halo element.  Nothing
 * else outside the interior is read, whatever it holds.  csi_update_state and every step entry point (csi_time_step_fe / _rk3, which end
 * each stage with update_state!; csi_time_step_momentum, whose velocity launches store their halo images and whose finalize_rheology!
 * fills sigma's locally and exchanges them between tiles, csrc/csi_launch.hip do_finalize) leave these elements valid: locally filled on
 * periodic, wall and fold sides, exchanged on connected sides.  (On a tiled context csi_time_step_momentum called on its own is followed
 * by csi_update_state, as everywhere: the velocities beyond a connected side are update_state!'s to exchange.)
 * Tiled contexts: the call is rank-local, no communication; on a north fold the halo images already carry the sign.
 * Errors: CSI_ERR_INVALID_ARGUMENT for mask == 0 or an unknown bit and for a grid without halo; CSI_ERR_NOT_BOUND naming u, v, sigma11
 * ..., or the derived slot ("divergence", "shear", "deformation", "speed", "sigma_I", "sigma_II", "stress_power") that is requested but
 * not bound.
 *
 * ENERGY BUDGET.  csi_budget_compute(ctx, what, out): sums over i = 1 .. Nx, j = 1 .. Ny, by the two-launch scheme of the device
 * diagnostics and in its SUMMATION ORDER (stated above; one term per cell and sum, formed as written here), followed by a copy of the
 * three slots to page-locked memory and a wait for the stream.
 * CSI_BUDGET_STRESS (needs u, v, sigma11, sigma22, sigma12):
 *   internal_work = sum ((u * d1) * Az^fc + (v * d2) * Az^cf),  d1 = d_j sigma_1j(i, j), d2 = d_j sigma_2j(i, j) of
 *                   ice_stress_divergence.jl:39-51 with its immersed conditionals (a stress at an immersed peripheral node counts as 0)
 *   stress_power  = sum (((sigma11 * e11) * Az^cc + (sigma22 * e22) * Az^cc) + ((2 * sigma12) * e12(i, j)) * Az^ff)
 *   On grids without a mask, with fields that vanish on and beyond the walls (or periodic ones), internal_work = -stress_power to
 *   rounding: the reference's adjoint identity (its test asserts |W + D| / max(|W|, |D|) < 1e-10).  With land it does not close.
 * CSI_BUDGET_KINETIC (needs u, v, h, aice; the density is csi_evp_params.sea_ice_density, 900 before csi_evp_params_set):
 *   kinetic_energy = sum (((0.5 * mu) * (u * u)) * Az^fc + ((0.5 * mv) * (v * v)) * Az^cf),  mu = (m[i - 1, j] + m[i, j]) / 2,
 *                    mv = (m[i, j - 1] + m[i, j]) / 2,  m = h * rho * aice as the velocity kernels form it (ClimaSeaIce.jl:42)
 * Members of a group that was not requested hold NaN.  Elements read outside the interior: u row 0, v column 0, sigma11 / sigma22 / h /
 * aice column 0 and row 0, sigma12 column Nx + 1 and row Ny + 1, the mask one element around (the same guarantee as above).
 * The work of the external stresses is not computed.  Tiled contexts: COLLECTIVE, all-gathered and added in rank order exactly as the
 * diagnostics' sums; all ranks return the same bits.  Errors by name as for the diagnostics.
 * csi_derived_stats: launches of the derived-field kernel and budget calls made on the context so far (tests; either pointer may be NULL). */
typedef enum {
    CSI_F_D_DIVERGENCE = CSI_F_COUNT_TOTAL,
    CSI_F_D_SHEAR,
    CSI_F_D_DEFORMATION,
    CSI_F_D_SPEED,
    CSI_F_D_SIGMA_I,
    CSI_F_D_SIGMA_II,
    CSI_F_D_STRESS_POWER,
    CSI_F_COUNT_DERIVED                     /* every slot csi_field_bind takes, the derived ones included */
} csi_derived_field_id;
#define CSI_DERIVED_DIVERGENCE 1
#define CSI_DERIVED_SHEAR 2
#define CSI_DERIVED_DEFORMATION 4
#define CSI_DERIVED_SPEED 8
#define CSI_DERIVED_SIGMA_I 16
#define CSI_DERIVED_SIGMA_II 32
#define CSI_DERIVED_STRESS_POWER 64
#define CSI_DERIVED_ALL 127
int32_t csi_derived_compute(csi_context* ctx, int32_t mask);
#define CSI_BUDGET_STRESS 1
#define CSI_BUDGET_KINETIC 2
#define CSI_BUDGET_ALL 3
typedef struct {
    int32_t what;                  /* echo of the request */
    int32_t reserved;
    double internal_work, stress_power;   /* CSI_BUDGET_STRESS */
    double kinetic_energy;                /* CSI_BUDGET_KINETIC */
} csi_budget;
int32_t csi_budget_compute(csi_context* ctx, int32_t what, csi_budget* out);
int32_t csi_derived_stats(csi_context* ctx, int64_t* derived_launches, int64_t* budget_calls);

/* ---- momentum balance terms, interface stresses and their power ------------------------------------------------------------------------
 * Which forces balance where, and what stress the ice puts on the ocean: every term of u_velocity_tendency / v_velocity_tendency
 * (SeaIceDynamics/momentum_tendencies_kernel_functions.jl:11-74) kept as a force per unit area (N m^-2) at its velocity point, the
 * reference's coupler-facing x_momentum_stress / y_momentum_stress (sea_ice_external_stress.jl:33-37, 162-174), and the power of each
 * term.  Nothing here changes another entry point: a context that never makes these calls launches exactly what it launched before.
 * One code serves STRICT and FAST, compiled without contraction, IEEE division and square root: both modes give the same bits
 * (tests/momentum_terms_ref.py restates every formula below in NumPy).  Every dynamics configuration the library steps is served:
 * EVP and ViscousRheology with either solver, free-drift dynamics (csi_dynamics_set), tiles and north folds.
 *
 * TERM FIELDS.  Ten further slots of csi_field_bind, numbered from CSI_F_COUNT_DERIVED on so that every older id and count keeps its
 * value: five per component, the _X slots at (Face, Center) with parent extents like u, the _Y slots at (Center, Face) like v.
 * csi_momentum_terms_compute(ctx, mask) fills the INTERIOR of every requested, bound slot -- i = 1 .. Nx (+ 1: the last face of a
 * Bounded x side), j = 1 .. Ny for _X; i = 1 .. Nx, j = 1 .. Ny (+ 1) for _Y -- in ONE launch on the context's stream (no atomics, no
 * flags, no wait; halos are never written).  mask: CSI_MTERM_* bits, a bit selects both components.  At the u point (i, j), in this
 * order (the v point analogous with j - 1 for i - 1, y_f_cross_U = f * Ixy(u) and the _2j operators):
 *   m_i  = (h[i-1, j] * rho * aice[i-1, j] + h[i, j] * rho * aice[i, j]) / 2          (u_velocity_tendency:28; rho: csi_evp_params
 *   a_i  = (aice[i-1, j] + aice[i, j]) / 2                                    (:29)     .sea_ice_density, 900 before csi_evp_params_set)
 *   Ixy(v) = ((v[i-1, j] + v[i, j]) / 2 + (v[i-1, j+1] + v[i, j+1]) / 2) / 2
 *   CORIOLIS_X = m_i * (-x_f_cross_U),  x_f_cross_U = -f * Ixy(v)      (the term with the sign it has in G^U; +0.0 without Coriolis)
 *   TOP_X      = -(a_i * tau_top)
 *   BOTTOM_X   = a_i * tau_bottom            (its negative is the stress the ocean receives)
 *   INTERNAL_X = d_j sigma_1j + immersed_d_j sigma_1j      (ice_stress_divergence.jl:36-44, 65-92: conditional fluxes and immersed flux
 *                boundary conditions as in the tendency; ViscousRheology: sigma = nu * delta u; free-drift dynamics: +0.0)
 *   (free-drift dynamics, csi_dynamics_set(ctx, CSI_DYNAMICS_FREE_DRIFT): StressBalanceFreeDrift carries neither a rheology nor a
 *    Coriolis term -- INTERNAL and CORIOLIS are +0.0 there, whatever csi_evp_params_set was given)
 *   FORCING_X  = m_i * model.forcing.u[i, j]      (CSI_F_FORCING_U, the user array only -- not the pseudo-time term of the EVP
 *                sum_of_forcing_u; +0.0 without arrays)
 *   tau = x_momentum_stress of the stress kind: CSI_STRESS_NONE 0; CSI_STRESS_CONST the number; CSI_STRESS_FIELD the array at the
 *         point; CSI_STRESS_SEMI_IMPLICIT ((rho_e * C_D) * sqrt(du * du + dv * dv)) * du, du = u_e[i, j] - u[i, j],
 *         dv = Ixy(v_e) - Ixy(v)      (:162-174: explicit - implicit * u in one product)
 *   Every slot is +0.0 where m_i <= 0 and at a peripheral velocity node (a wall face, a face next to land, the last face of a Bounded
 *   side).  With CSI_MTERM_RAW_STRESS in the mask the TOP and BOTTOM slots receive tau_top and tau_bottom themselves -- the interface
 *   stresses x_momentum_stress / y_momentum_stress, without the a_i factor and the sign, zero at the same points -- in the same launch.
 *   Output arrays never alias inputs.
 * HALO ELEMENTS READ (the entry point fills none): ONE RING around the own interior of u, v, h, aice, of sigma11, sigma22, sigma12
 * (INTERNAL on an EVP model), of the stress / external-velocity arrays (CSI_F_TOP_U .. CSI_F_BOT_V) and of the forcing arrays, and of the
 * mask; nothing beyond it, whatever it holds.  The step entry points (csi_time_step_fe / _rk3, free-drift dynamics included) and
 * csi_update_state after csi_time_step_momentum leave these elements valid, as for csi_derived_compute; the stress and forcing arrays'
 * rings are filled by every momentum step (update_external_stress!) or by csi_fill_halo_local.
 * Required: u, v, h, aice; with INTERNAL on an EVP model sigma11, sigma22, sigma12; the arrays the stresses name.  Errors:
 * CSI_ERR_NOT_BOUND naming the field, or the requested slot ("coriolis_x", ..., "forcing_y") that has no array;
 * CSI_ERR_INVALID_ARGUMENT for mask == 0, a mask without a term bit, unknown bits and a grid with halo < 1.
 * Tiled contexts: rank-local, no communication; on a north fold the halo images already carry the sign.
 *
 * POWER.  csi_momentum_budget_compute(ctx, what, out): for each term F the sum of (u * F_X) * Az^fc + (v * F_Y) * Az^cf over
 * i = 1 .. Nx, j = 1 .. Ny (the last face of a Bounded side is a peripheral node: its terms are 0 and it is not added), the terms
 * formed on the fly exactly as above (no slot needs to be bound; TOP and BOTTOM with the a_i factor and the sign).  The two-launch
 * scheme and the SUMMATION ORDER of the device diagnostics and of csi_budget_compute: records of 64 x 64 cells, then a single-block
 * fold -- a function of (Nx, Ny) alone.  what: CSI_MBUDGET_EXTERNAL (top, bottom), CSI_MBUDGET_BODY (coriolis, forcing),
 * CSI_MBUDGET_INTERNAL (the only group that loads sigma); members of a group that was not requested hold NaN.  The sum of the five is
 * the rate of change of kinetic energy the terms imply (no inertia term; an EVP sub-cycle does not close it per step).
 * Requirements and errors as above, INTERNAL meaning the group.  Tiled contexts: COLLECTIVE, all-gathered and added in rank order
 * exactly as csi_budget_compute; all ranks return the same bits; a rank that fails locally still reaches the all-gather.
 * csi_momentum_terms_stats: launches of the term kernel and power calls made on the context so far (either pointer may be NULL). */
typedef enum {
    CSI_F_M_CORIOLIS_X = CSI_F_COUNT_DERIVED,
    CSI_F_M_CORIOLIS_Y,
    CSI_F_M_TOP_X,
    CSI_F_M_TOP_Y,
    CSI_F_M_BOTTOM_X,
    CSI_F_M_BOTTOM_Y,
    CSI_F_M_INTERNAL_X,
    CSI_F_M_INTERNAL_Y,
    CSI_F_M_FORCING_X,
    CSI_F_M_FORCING_Y,
    CSI_F_COUNT_BINDABLE                    /* every slot csi_field_bind took before the slots of csi_thermo_linear_field_id */
} csi_momentum_term_field_id;
/* Five further (c,c) slots of csi_field_bind (csi_heat_fluxes_set: the LINEAR term's per-cell K and Ta, the per-cell bottom salinity,
 * the two used-flux outputs), numbered from CSI_F_COUNT_BINDABLE on so that every older id and count keeps its value. */
typedef enum {
    CSI_F_FLUX_COEFFICIENT = CSI_F_COUNT_BINDABLE,   /* K of the LINEAR top term, W m^-2 K^-1 */
    CSI_F_FLUX_REFERENCE_TEMPERATURE,                /* Ta of the LINEAR top term */
    CSI_F_BOTTOM_SALINITY,                           /* S of Tb = liq_T0 - liq_slope * S */
    CSI_F_TOP_HEAT_FLUX_USED,                        /* output: the top flux the last thermodynamic step used, W m^-2 */
    CSI_F_BOTTOM_HEAT_FLUX_USED,                     /* output: the bottom flux it used */
    CSI_F_COUNT_THERMO                               /* every slot csi_field_bind takes */
} csi_thermo_linear_field_id;
#define CSI_MTERM_CORIOLIS 1
#define CSI_MTERM_TOP 2
#define CSI_MTERM_BOTTOM 4
#define CSI_MTERM_INTERNAL 8
#define CSI_MTERM_FORCING 16
#define CSI_MTERM_ALL 31
#define CSI_MTERM_RAW_STRESS 32             /* flag: TOP / BOTTOM receive the interface stresses tau_top / tau_bottom */
int32_t csi_momentum_terms_compute(csi_context* ctx, int32_t mask);
#define CSI_MBUDGET_EXTERNAL 1
#define CSI_MBUDGET_BODY 2
#define CSI_MBUDGET_INTERNAL 4
#define CSI_MBUDGET_ALL 7
typedef struct {
    int32_t what;                  /* echo of the request */
    int32_t reserved;
    double coriolis, top, bottom, internal, forcing;      /* W: BODY, EXTERNAL, EXTERNAL, INTERNAL, BODY */
} csi_momentum_budget;
int32_t csi_momentum_budget_compute(csi_context* ctx, int32_t what, csi_momentum_budget* out);
int32_t csi_momentum_terms_stats(csi_context* ctx, int64_t* launches, int64_t* budget_calls);

/* ---- the slab-ocean mixed layer under the ice: frazil growth, basal melt ---------------------------------------------------------------
 * The reference leaves the ocean under the ice to a FluxFunction closure; its example examples/freezing_of_a_lake.jl:91-120 shows what
 * that closure does: a bucket of water with a temperature of its own, cooled by the atmosphere over the open-water fraction 1 - aice,
 * whose heat deficit below freezing becomes a negative bottom flux that grows ice.  What users write into that closure is a fixed form,
 * and a fixed form is data: a mixed-layer heat budget with frazil formation and a bulk ice-ocean heat flux, as every stand-alone
 * sea-ice code carries it (recalled from CICE's ocean_mixed_layer).  THIS TEXT IS THE DEFINITION.
 *
 * All heat fluxes are positive upward, like top_heat_flux.  Per interior cell:
 *   To   the mixed-layer temperature the step starts from (CSI_F_ML_TEMPERATURE, or its Psi^- copy CSI_F_ML_TEMPERATURE_M)
 *   a    the concentration the thermodynamic step starts from (CSI_F_A)
 *   Tf = liq_T0 - liq_slope * Sb, with the same Sb (csi_slab_params.bottom_salinity, or per cell CSI_F_BOTTOM_SALINITY under
 *        CSI_SOLVE_BOTTOM_SALINITY_ARRAY) that the ice step uses for Tb
 * The arithmetic is uncontracted, in exactly this order, and STRICT and FAST are alike:
 *   C   = (rho * c) * depth
 *   Qs  = Fo + (K * (To - Ta))          absent terms are not added: Fo alone, the bulk term alone, or 0
 *   Qow = Qs * (1 - a)                  open-water surface flux, per cell area
 *   dT  = To - Tf
 *   Qio = dT > 0 ? min(((gamma * (rho * c)) * dT) * a, (C * dT) / dt) : 0      basal melt flux, >= 0
 *   T1  = To + (dt * ((Qd - Qow) - Qio)) / C
 *   Qfr = T1 < Tf ? (C * (T1 - Tf)) / dt : 0                                   frazil, <= 0
 *   To' = T1 < Tf ? Tf : T1
 *   Qb  = Qio + Qfr                     the ice step's bottom external flux, per cell area
 * Fo (surface_heat_flux), K (coefficient), Ta (reference_temperature) and Qd (deep_heat_flux, heat from below the mixed layer) are
 * each a number or a (c,c) array: CSI_ML_SURFACE_ARRAY reads Fo from CSI_F_ML_SURFACE_HEAT_FLUX, CSI_ML_BULK_ARRAYS reads K and Ta
 * from CSI_F_ML_COEFFICIENT and CSI_F_ML_REFERENCE_TEMPERATURE (both or neither; a front end broadcasts the number), CSI_ML_DEEP_ARRAY
 * reads Qd from CSI_F_ML_DEEP_HEAT_FLUX.  CSI_ML_HAS_SURFACE / CSI_ML_HAS_BULK say which terms of Qs exist (an array flag implies its
 * term).  The same K, Ta and flux arrays may serve the ice top (CSI_FLUX_LINEAR) and the open water.  gamma (exchange_velocity,
 * m s^-1), rho (density), c (heat_capacity) and depth are numbers.  The budget C (To' - To) / dt = Qd - Qow - Qb holds to rounding.
 * Every interior cell is computed, land included, as the thermodynamic kernels do.  No halo element is read or written.
 *
 * ONE point-wise launch (mixed_layer.hip, k_mixed_layer) writes To' into CSI_F_ML_TEMPERATURE, Qb into the interior of the array
 * bound to CSI_F_BOTTOM_HEAT_FLUX -- which the ice step reads as the ARRAY bottom term it already knows; its kernels do not change --
 * and, where CSI_F_ML_SURFACE_FLUX_USED is bound, Qow there.
 * LIMIT: heat offered as Qio beyond what melts the cell's ice is lost where ice_volume_update clips, as any bottom flux is today.
 *
 * csi_mixed_layer_set(ctx, p): p == NULL removes the mixed layer.  CSI_ERR_INVALID_ARGUMENT, by name, for non-finite values, for
 *   density, heat_capacity or depth <= 0, for exchange_velocity < 0 and for unknown flag bits.
 * csi_mixed_layer_step(ctx, dt, from_cache): the launch above; from_cache != 0 reads To from CSI_F_ML_TEMPERATURE_M.  Refused by
 *   name: no csi_slab_params_set (it needs the liquidus and Sb; CSI_ERR_NOT_BOUND); bottom heat-flux terms other than exactly one
 *   ARRAY term (CSI_ERR_INVALID_ARGUMENT); an unbound slot that a flag names, CSI_F_ML_TEMPERATURE, CSI_F_A or CSI_F_BOTTOM_HEAT_FLUX
 *   (CSI_ERR_NOT_BOUND); from_cache without CSI_F_ML_TEMPERATURE_M (CSI_ERR_NOT_BOUND).
 * csi_mixed_layer_stats(ctx, &launches): launches of k_mixed_layer on the context so far.
 *
 * Where it runs: csi_time_step_fe and csi_time_step_rk3 run the step immediately before the thermodynamic step of every stage.  FE
 * uses from_cache = 0.  RK3 uses from_cache = 1 (CSI_F_ML_TEMPERATURE_M must be bound): every stage computes To from Psi^- with its
 * own stage step and the last stage (the whole step) is the step's result, exactly as h and aice behave -- without this To would
 * advance 11/6 of the step per step.  csi_cache_current_fields copies To into its Psi^- slot when both are bound, in the same single
 * launch.  csi_slab_thermo_step and csi_layered_thermo_step called on their own run what they ran before: a caller runs
 * csi_mixed_layer_step first.  The four input slots may be driven by time series (csi_time_series_set: eighteen slots, one launch); a
 * series on CSI_F_BOTTOM_HEAT_FLUX together with a mixed layer is refused by name (the step writes that array).  A context that never
 * calls csi_mixed_layer_set launches what it launched before.
 *
 * The seven slots are numbered from CSI_F_COUNT_THERMO on, so that every older id and count keeps its value. */
typedef enum {
    CSI_F_ML_TEMPERATURE = CSI_F_COUNT_THERMO,       /* (c,c) To, state */
    CSI_F_ML_TEMPERATURE_M,                          /* (c,c) its Psi^- copy */
    CSI_F_ML_SURFACE_HEAT_FLUX,                      /* (c,c) Fo per cell, W m^-2 */
    CSI_F_ML_COEFFICIENT,                            /* (c,c) K per cell, W m^-2 K^-1 */
    CSI_F_ML_REFERENCE_TEMPERATURE,                  /* (c,c) Ta per cell */
    CSI_F_ML_DEEP_HEAT_FLUX,                         /* (c,c) Qd per cell, W m^-2 */
    CSI_F_ML_SURFACE_FLUX_USED,                      /* (c,c) optional output: Qow */
    CSI_F_COUNT_MIXED_LAYER                          /* every slot csi_field_bind takes */
} csi_mixed_layer_field_id;
#define CSI_ML_SURFACE_ARRAY 1
#define CSI_ML_BULK_ARRAYS 2
#define CSI_ML_DEEP_ARRAY 4
#define CSI_ML_HAS_SURFACE 8
#define CSI_ML_HAS_BULK 16
typedef struct {
    double density;                    /* rho, 1026 kg m^-3 */
    double heat_capacity;              /* c, 3991 J kg^-1 K^-1 */
    double depth;                      /* m */
    double exchange_velocity;          /* gamma, 6e-5 m s^-1 */
    double surface_heat_flux;          /* Fo, W m^-2 */
    double coefficient;                /* K, W m^-2 K^-1 */
    double reference_temperature;      /* Ta, in the unit of To */
    double deep_heat_flux;             /* Qd, W m^-2 */
    int32_t flags;                     /* CSI_ML_* */
    int32_t reserved;                  /* 0 */
} csi_mixed_layer_params;
int32_t csi_mixed_layer_set(csi_context* ctx, const csi_mixed_layer_params* p);
int32_t csi_mixed_layer_step(csi_context* ctx, double dt, int32_t from_cache);
int32_t csi_mixed_layer_stats(csi_context* ctx, int64_t* launches);

/* ---- absorbed shortwave radiation with a temperature-dependent (stepped) albedo ------------------------------------------------------
 * The fifth top heat-flux term of the reference's examples/arctic_basin_seasonal_cycle.jl (Semtner 1976), which writes it into a
 * FluxFunction closure: Q * (1 - alpha) with alpha = ifelse(Ts < -0.1, 0.75, 0.64).  As data it is CSI_FLUX_SHORTWAVE = 4, a fifth
 * csi_heat_flux_kind: top only, at most one per model, and it takes its place in the right-nested sum like any other term.  Its value at
 * surface temperature T is formed in exactly this order, uncontracted, in STRICT and FAST alike:
 *     alpha = (T < threshold) ? cold : warm          strict <: T == threshold takes warm
 *     Q     = (F * (1 - alpha)) * w                  w as for LINEAR: CSI_WEIGHT_NONE no product, CSI_WEIGHT_CONCENTRATION w = aice[i, j]
 *                                                    at the start of the step, CSI_WEIGHT_ICE_PRESENT (aice == 0) ? 0 : F * (1 - alpha)
 * F (flux, W m^-2, positive upward like every heat flux here: sunlight reaching the ice is negative) is a number, or with per_cell = 1
 * is read per cell from the (c,c) array bound to CSI_F_SHORTWAVE.  The layered step uses the second triple (snow_cold, snow_warm,
 * snow_threshold) in cells whose hs at the start of the step is > 0 -- the condition under which it sets Tm = 0; with has_snow_pair = 0
 * the ice triple serves both.  The parameters do not fit csi_heat_flux_term, whose size and offsets do not change: they travel in
 * csi_shortwave through csi_shortwave_set, and the term in the tuple is {kind = CSI_FLUX_SHORTWAVE}, which marks the position in the
 * sum (its other members are ignored).  csi_shortwave_set(ctx, NULL) removes the setting.
 *   CSI_ERR_INVALID_ARGUMENT, by name: a SHORTWAVE term in csi_heat_fluxes_set (or at a step) without the set call; a set call whose
 *   per_cell flag finds no array bound to CSI_F_SHORTWAVE; an albedo outside [0, 1]; a non-finite value; an unknown weighting;
 *   reserved != 0.  CSI_ERR_UNSUPPORTED: the term at the bottom, two SHORTWAVE terms.
 * The term makes Qx depend on T.  Under MeltingConstrainedFluxBalance every consolidated cell runs the secant solve of
 * csi_heat_fluxes_set, with the same tol and maxiters and no closed form; Qx is then evaluated once at the capped temperature, so a
 * cell capped at Tm >= threshold melts with the warm albedo.  Under PrescribedTemperature the term is evaluated at the prescribed
 * temperature.  Qx is discontinuous at the threshold: where the balance has no root on either branch the iterates step across the jump
 * and the solve ends, by its |x1 - x0| < tol rule, within tol of the threshold.
 * Where the solve's two points straddle the threshold with nearly equal residuals it can also end by that rule away from balance (9 of
 * the 200 000 cells below).  LIMIT: beside terms that leave the balance LINEAR in T (no RadiativeEmission) f is two parallel lines with
 * a jump between them, and once the two points lie on different sides the secant can cycle until maxiters; the last iterate is then the
 * root, as for any unconverged solve.  A surface balance with emission, like the example's, curves and does not cycle.  All of this is
 * the reference's solver applied to the reference's closure; nothing is substituted.
 * NOT OFFERED: a continuous ramp albedo, linear in T between two temperatures.  On 200 000 random cells (h 0.05-4 m, shortwave
 * 0-320 W m^-2, other downward fluxes 120-330 W m^-2, emission, Tu- in -30...0) the stepped form converged everywhere in at most 135
 * updates; a ramp over -1...0 left 246 cells cycling until maxiters = 1000.  A term the reference's solver cannot solve is not offered.
 * Neither are: an albedo that depends on thickness or snow depth, shortwave penetration, albedo parameters per cell, melt ponds.
 *
 * One optional OUTPUT slot, CSI_F_ALBEDO_USED: when bound and a SHORTWAVE term is set, the thermodynamic step writes the alpha it used
 * at the temperature it solved (or was prescribed) into its interior.  A model with the term runs the flux kernels already.
 * CSI_F_TOP_HEAT_FLUX_USED includes the absorbed shortwave, since it is Qx(Tu).  CSI_F_SHORTWAVE may be driven by a time series
 * (csi_time_series_set: nineteen slots, one launch).
 *
 * The two slots are numbered from CSI_F_COUNT_MIXED_LAYER on, so that every older id and count keeps its value. */
typedef enum {
    CSI_F_SHORTWAVE = CSI_F_COUNT_MIXED_LAYER,       /* (c,c) F per cell, W m^-2 */
    CSI_F_ALBEDO_USED,                               /* (c,c) optional output: alpha */
    CSI_F_COUNT_SHORTWAVE                            /* every slot csi_field_bind takes */
} csi_shortwave_field_id;
typedef struct {
    double flux;                       /* F, W m^-2 (ignored with per_cell) */
    double cold, warm, threshold;      /* alpha = (T < threshold) ? cold : warm; 0.75, 0.64, -0.1 */
    double snow_cold, snow_warm, snow_threshold;   /* the same for cells with hs > 0 (layered step, has_snow_pair) */
    int32_t weighting;                 /* csi_flux_weighting */
    int32_t per_cell;                  /* 1: F per cell from CSI_F_SHORTWAVE */
    int32_t has_snow_pair;             /* 1: the snow triple is used where hs > 0 */
    int32_t reserved;                  /* 0 */
} csi_shortwave;
int32_t csi_shortwave_set(csi_context* ctx, const csi_shortwave* p);

/* ---- rheology and momentum solver (SeaIceMomentumEquation(grid; rheology, solver), sea_ice_momentum_equations.jl:67-94) ------------
 * Defaults: CSI_RHEOLOGY_EVP with CSI_SOLVER_SPLIT_EXPLICIT -- the library's EVP path, unchanged by these calls.  The scalars both
 * rheologies share (minimum mass / concentration, sea_ice_density, FPlane f) still come from csi_evp_params_set, which marks the model
 * as having dynamics; the EVP fields of that struct are ignored by a viscous model.  (csi_dynamics_set(ctx, CSI_DYNAMICS_FREE_DRIFT)
 * needs none of it.)
 *
 * CSI_RHEOLOGY_VISCOUS: ViscousRheology(nu) with a Number nu (Rheologies/viscous_rheology.jl:1-22): stresses nu * delta u computed
 *   inline from the velocities, no auxiliary fields (the ten EVP slots need not be bound), sub-step Delta t / substeps, sum_of_forcing_*
 *   = the user forcing alone, initialize_rheology! / compute_stresses! / finalize_rheology! no-ops (Rheologies.jl:42-55).  A Field- or
 *   function-valued nu is not supported (its face interpolation lives in un-vendored Oceananigans).
 *   Split-explicit sub-cycle: per sub-step a u launch and a v launch in the parity order of split_explicit_momentum_equations.jl:178,
 *   each writing its halo images with its stores (2 x substeps launches, at most one device copy at the end).  DELIBERATE DEPARTURE:
 *   the reference's velocity kernel writes u[i, j] in place while its viscous stencil reads u at the neighbouring points, a race whose
 *   result depends on scheduling; here each launch reads only the OLD values of its own component (separate input and output arrays,
 *   ping-ponged between the bound array and a context-owned scratch) -- Jacobi within a component, Gauss-Seidel between the two.
 * CSI_SOLVER_EXPLICIT: ExplicitSolver (explicit_momentum_equations.jl): csi_compute_momentum_tendencies writes G^n.u / G^n.v
 *   (CSI_F_GU / CSI_F_GV) from the current state -- with EVP from the STORED sigma (compute_stresses! is never called) and the
 *   (u^n - u) / Delta t / Ixᶠᵃᵃ(alpha) forcing term with u^n as it stands --; csi_time_step_momentum then sets
 *   u = select((u^- + dt G) / (1 + dt tau_i), free drift, 0) and the same for v (u^- = Psi^-.u when rk_reset != 0, the current u otherwise),
 *   no `* active` factor, no m <= 0 guard on tau_i; three launches, each velocity launch writing its halo images.  csi_time_step_fe /
 *   _rk3 call both where the reference does (sea_ice_fe_step.jl:19-22, sea_ice_rk_substep.jl:84-87).  The values the local fill and
 *   update_state! leave on wall faces and immersed faces are recalled fill semantics, not pinned (as for the fold).
 * Both: csi_set_fusion levels are ignored (no fused kernels on these paths); STRICT is the reference's operation order, FAST uses
 * explicit FMAs and reciprocals.  Tiled contexts (connected topologies / csi_tile_set) and north-fold topologies return
 * CSI_ERR_UNSUPPORTED for a rheology other than EVP or a solver other than the split-explicit one. */
typedef enum { CSI_RHEOLOGY_EVP = 0, CSI_RHEOLOGY_VISCOUS = 1 } csi_rheology_kind;
typedef enum { CSI_SOLVER_SPLIT_EXPLICIT = 0, CSI_SOLVER_EXPLICIT = 1 } csi_momentum_solver_kind;
/* nu: ViscousRheology's nu (m^2 s^-1 as the reference scales it; ignored for EVP) */
int32_t csi_rheology_set(csi_context* ctx, int32_t kind, double nu);
int32_t csi_momentum_solver_set(csi_context* ctx, int32_t kind);
/* compute_momentum_tendencies!(model, dynamics, dt): explicit_momentum_equations.jl:85-113 for CSI_SOLVER_EXPLICIT (needs CSI_F_GU,
 * CSI_F_GV); a no-op for the split-explicit solver (SeaIceDynamics.jl:41). */
int32_t csi_compute_momentum_tendencies(csi_context* ctx, double dt);

/* FAST mode only.  level 0: always the three-kernel path.  level 1: a sub-step is ONE launch of the fused
 * kernel (stress + both velocity updates, ring recomputation per wavefront, double-buffered u, v, sigma in
 * library scratch) whenever the configuration allows it (no immersed mask, forcing given by numbers;
 * csrc/evp_fused.hip).  level 2 (default): in addition
 * TWO consecutive sub-steps share one launch (csrc/evp_fused2.hip: the first sub-step's results stay in
 * registers; immersed masks, array-valued top stress and array-valued ocean velocities in the bottom drag
 * supported) where the halo is >= 4 (and N >= 2 halo) and, on tiles, the exchange
 * interval is even; an odd trailing sub-step uses the level-1 kernel, or -- with masks, array forcing or per-point metrics -- one more launch
 * of the same kernel whose second wave stores the first sub-step's results instead of computing a second one.  All paths execute the same
 * floating-point operations and give bit-identical results. */
/* (Round 2 built a level 3 -- three sub-steps per launch, three waves per tile chained through two LDS rings; it traded a third of
 * the HBM traffic for 10 % more arithmetic and measured slower than level 2 at every size but 3072^2, so round 4 removed it:
 * DESIGN.md section 3.)  Levels other than 0, 1, 2 are refused. */
int32_t csi_set_fusion(csi_context* ctx, int32_t level);

/* Tile activity (round 6; default on).  Where the ice mass h rho aice is exactly zero -- land after mask_immersed_field_xy!
 * (src/sea_ice_model.jl:379-384), ice-free ocean -- the EVP sub-step is an exact no-op: sigma += ifelse(m > 0, ..., 0)
 * (src/Rheologies/elasto_visco_plastic_rheology.jl:343-347) and the velocity select's zero branch
 * (src/SeaIceDynamics/split_explicit_momentum_equations.jl:217-228, 251-263).  On untiled grids advanced by the two-sub-steps
 * kernel the library tests, before the first launch of every sub-cycle, which 56-column tiles of the launch have no ice mass in
 * or one cell around them (and no -0.0 among their stresses); the first two launches and the last one run every tile, the
 * launches in between only the live ones, on a finer tiling chosen so that the live tiles fill the GPU once.  Results are
 * bit-identical with skipping off (tests/test_gpu_activity.py) as long as the fields are finite.
 * csi_tile_activity: the newest counts that have arrived from the device (tiles of the live launches, live ones among them;
 * -1 live: none yet), and whether the last sub-cycle used live launches (1; 2: its first two launches also left out the tiles that
 * were quiescent from the start -- no ice mass, velocities +0.0 already, no halo image to store --, which takes one copy of u, v,
 * sigma per sub-cycle and is done once a sample has shown quiescent tiles) -- call csi_sync first for the last sub-cycle's counts. */
int32_t csi_set_tile_skipping(csi_context* ctx, int32_t on);
int32_t csi_tile_activity(csi_context* ctx, int32_t* tiles, int32_t* live, int32_t* used);

/* CSI_METRIC_FULL grids, row-constant rows (round 6; default on, rtol 0).  A TripolarGrid is a latitude-longitude grid south of
 * its bipolar cap: there every metric plane holds one value per row.  The library marks the rows in which all Nx + 2Hx + 1
 * columns of all twelve coefficient planes (and of a per-point Coriolis parameter) are EQUAL BIT FOR BIT and lets the
 * two-sub-steps kernel read those rows' values from per-row vectors -- the same operands, the same operations, 96 B per cell and
 * launch less HBM traffic; results are unchanged.  rtol > 0 (at most 1e-6) also marks rows whose columns agree with the first
 * interior column to that relative distance and uses that column's value for the row: for grids whose row-constant part
 * carries rounding noise (metrics computed per point); this CHANGES results at the rtol level and is the caller's decision.
 * csi_row_constant_rows: how many of the Ny + 2Hy + 1 plane rows are marked. */
int32_t csi_set_row_constant(csi_context* ctx, int32_t on, double rtol);
int32_t csi_row_constant_rows(csi_context* ctx, int32_t* rows);

/* RCCL halo exchange of u, v every k sub-steps with width 2k (needs halo >= 2k).  k = 0 (default): automatic -- the peer
 * transport below where it applies, else the largest k <= 16 the halo allows; k >= 1 selects the RCCL exchange with that
 * interval (k = 1: every sub-step); the reference is the k = substeps extreme (halo 2*substeps+3,
 * split_explicit_momentum_equations.jl:51-64). */
int32_t csi_set_exchange_interval(csi_context* ctx, int32_t k);

/* Halo transport of the sub-cycle on tiles (FAST mode, two sub-steps per launch; an odd count ends with one single-sub-step launch
 * of the same kernel).
 * CSI_TRANSPORT_PEER (default): peer-direct halo writes over xGMI.  The neighbouring tiles' u, v, sigma (and alpha, zeta, Delta)
 * arrays are mapped into this process (HIP IPC handles, exchanged once over the context's RCCL communicator); a connected side
 * then behaves like a Periodic one whose halo lives on another GPU: the kernel that owns a cell next to the side stores its halo
 * image straight into the neighbour's array, and per-tile flags in device memory order the launches of neighbouring ranks (only
 * the tiles next to a connected side wait, the interior of a launch overlaps the neighbours' edges).  No pack / unpack kernels,
 * no RCCL kernel inside the sub-cycle, no widened halo: the halo 4 of an untiled run suffices, and one RCCL exchange per
 * sub-cycle remains (what BASELINE.json's north star asks for; the reference's own design is one exchange per sub-cycle with a
 * 2 * substeps + 3 halo, split_explicit_momentum_equations.jl:51-64).  Needs tiles of equal shape (their row strides may differ: the easternmost tile of a Bounded x partition); set up
 * collectively at the first sub-cycle (and again when bound arrays change -- bind on all ranks together); if any rank cannot
 * (no IPC, a tile the two-sub-steps kernel does not take), every rank stays on RCCL.  A tile that waits 3 s for a neighbour gives up, the next csi_sync
 * returns CSI_ERR_COMM.
 * CSI_TRANSPORT_RCCL: pack -> grouped ncclSend / ncclRecv -> unpack of width-2k strips every k sub-steps
 * (csi_set_exchange_interval); what every other path (three kernels, STRICT) uses anyway.
 * Both give results bit-identical to the untiled run.  csi_halo_transport: what the last sub-cycle used. */
enum { CSI_TRANSPORT_RCCL = 0, CSI_TRANSPORT_PEER = 1 };
int32_t csi_set_halo_transport(csi_context* ctx, int32_t kind);
int32_t csi_halo_transport(csi_context* ctx, int32_t* kind);
/* Run-time tiers of the peer transport's memory-ordering protocol.  Every rank of a decomposition must set the SAME tier.
 *  -1 (default): automatic -- tier 1 whenever a neighbour lives in another process or on another device (one process per GPU, the
 *      host-channel group), tier 0 for a tile connected to itself and for the tiles of an in-process group on one device;
 *   0: halo images are write-through stores at system scope, flags follow the drained store queue; a waiting tile loads nothing
 *      before it has seen the flags and issues no cache maintenance (measured fastest).  It rests on an
 *      argument about what CANNOT be cached on the receiving GPU; that argument has only ever run inside one L2 domain, and a
 *      passing tiled == untiled check does not prove it (a violation would be a rare, timing-dependent stale line): across
 *      devices tier 0 is an explicit opt-in (bench.py --peer-tier 0), never the default;
 *   1: + a system-scope acquire fence (buffer_inv sc0 sc1) in every waiting tile once the flags have been seen (edge tiles only);
 *   2: + a system-scope release fence (buffer_wbl2 sc0 sc1) before a tile publishes its flags -- the textbook protocol.
 * csi_peer_tier returns the tier the kernels run (automatic resolved).
 * A wait that gives up after 3 s makes its workgroup leave without storing or publishing, sets this rank's error word and the
 * abort word of every neighbour's flag array; every entry point that advances the model and csi_sync report CSI_ERR_COMM -- and
 * keep reporting it (the error is STICKY: the flags cannot recover by themselves) until the caller has re-armed the transport on
 * EVERY rank with csi_set_halo_transport (CSI_TRANSPORT_PEER: the next sub-cycle runs the collective set-up again, which clears
 * flags, abort words and launch numbers once all ranks have arrived; CSI_TRANSPORT_RCCL: the message exchange) or csi_comm_init*.
 * csi_validate_all spreads the status to ranks that are not neighbours of the one that gave up. */
int32_t csi_set_peer_tier(csi_context* ctx, int32_t tier);
int32_t csi_peer_tier(csi_context* ctx, int32_t* tier);

/* Index ranges (1-based, inclusive: i0, i1, j0, j1) the launch loop uses for a grid of this shape and
 * topology when `valid_width` (V >= 2) layers of u, v beyond the owned cells are valid on connected sides:
 * [0..3] stress kernel (Auxiliaries kernel parameters -H+2:N+H-1, elasto_visco_plastic_rheology.jl:145, on
 * local sides; 2-V : N+V-1 on connected sides), [4..7] the u step when u is updated first, [8..11] the v step
 * when v is updated first, [12..15] the velocity updated second (cf. split_explicit_kernel_size,
 * split_explicit_momentum_equations.jl:40-46).  Pure host function. */
int32_t csi_plan_ranges(int32_t Nx, int32_t Ny, int32_t Hx, int32_t Hy, int32_t topo_x, int32_t topo_y,
                        int32_t valid_width, int32_t* out16);

/* The halo-exchange plan of one tile for one field, eight directions in the library's fixed order
 * (dy outer, dx inner, both -1..1, (0,0) skipped).  For k = 0..7, out40[5k..5k+4] = peer rank (-1: none),
 * i0, j0, ni, nj (1-based start and extents of the strip).  halo = 0: the owned strips this tile SENDS, in
 * send order; halo = 1: the halo strips it RECEIVES, in the order the matching sends were issued (message k
 * arrives from the neighbour in direction -k).  Pure host function: the CPU multi-process tests drive a gloo
 * exchange with exactly the plan the RCCL path uses. */
int32_t csi_plan_exchange(int32_t Nx, int32_t Ny, int32_t Hx, int32_t Hy, int32_t topo_x, int32_t topo_y,
                          int32_t rank_x, int32_t rank_y, int32_t Rx, int32_t Ry, int32_t periodic_x, int32_t periodic_y,
                          int32_t width, int32_t halo, int32_t* out40);

/* ---- introspection used by bench.py / tests ------------------------------------------------ */
/* Device time (ms) of the last csi_evp_subcycle / csi_time_step_momentum call measured with HIP
 * events on the context's stream; valid after csi_sync. */
int32_t csi_last_subcycle_ms(csi_context* ctx, double* ms);
/* Device time of ALL sub-cycles between the two calls (HIP events on the context's stream around every sub-step loop; _end
 * synchronises): their sum in ms, their number and the number of kernel launches inside them -- what bench.py divides to get the
 * dominant kernel's average launch time over the TIMED region itself (at most 4096 sub-cycles are kept). */
int32_t csi_subcycle_stats_begin(csi_context* ctx);
int32_t csi_subcycle_stats_end(csi_context* ctx, double* total_ms, int32_t* cycles, int32_t* launches);
/* How the launch loop would run one PAIR of sub-steps (csi_set_fusion level 2) at position m (even) of an exchange
 * batch of k sub-steps on a grid of this shape: out32[0] = 1 if the pair kernel applies (0: the rest is zero),
 * [1..3] wave-tile geometry (56-column strips, row chunks, rows per chunk), then six index ranges (i0, i1, j0, j1):
 * [4..7] rows / columns the first sub-step computes, [8..11] the second sub-step's compute range (what the wave tiles
 * decompose), [12..15] cells whose stresses are stored, [16..19] / [20..23] first velocity stored when the second
 * sub-step is u-first / v-first, [24..27] second velocity stored; [28] = 1 if a side is a wall.  Periodic and wall
 * sides store the interior (the wall corners of sigma12 included) and refresh halos as images of those stores;
 * connected sides store the ring the next pair needs.  Pure host function. */
int32_t csi_plan_pair(int32_t Nx, int32_t Ny, int32_t Hx, int32_t Hy, int32_t topo_x, int32_t topo_y, int32_t k, int32_t m,
                      int32_t* out32);
/* How a pair launch of the PEER transport cuts a tile of this shape into chunks of rows (pure host function; periodic f-plane tile,
 * sides as the launch loop sees them): out8 = {applies, strips, chunks, rows per chunk, rows of the first chunk (0: as the others),
 * rows kept for the last chunk (0: what is left), chunks in the south side's tile set, in the north side's}; rows_out[2q], [2q + 1]
 * = first / last row of chunk q (at most max_chunks of them).  peer_south / peer_north: a neighbour beyond that y side -- its chunk
 * is four rows shorter, never shorter than the halo. */
int32_t csi_plan_peer_chunks(int32_t Nx, int32_t Ny, int32_t Hx, int32_t Hy, int32_t peer_south, int32_t peer_north, int32_t cus,
                             int32_t* out8, int32_t* rows_out, int32_t max_chunks);

/* Per-phase device time: runs `substeps` (2..64) further EVP sub-steps from the current state with HIP
 * events between the launches on the context's stream and returns the average milliseconds of
 * [0] the stress phase (or, when the fused path is active, one LAUNCH of the fused kernel -- one or two
 *     sub-steps, see csi_last_launches -- then [1] = [2] = 0),
 * [1] the u step, [2] the v step, [3] the halo exchange (0 on an untiled grid).
 * Synchronises; for bench.py's roofline only, never on the timed path. */
int32_t csi_profile_substeps(csi_context* ctx, double dt, int32_t substeps, double* out_ms4);
/* Which path the last sub-cycle took: three kernels (0), fused kernel (1), fused pairs of sub-steps (2); the
 * halo-exchange interval k and the number of exchanges issued.  Any pointer may be NULL. */
int32_t csi_last_path(csi_context* ctx, int32_t* fused, int32_t* exchange_interval, int32_t* exchanges);
/* The layout of the last advection launch (csi_compute_tracer_tendencies, a time step with advection): tracers per thread (1 / 2),
 * the cells of a flux tile in x and y -- the block has one more thread each way, for the tile's east / north faces --, and whether
 * the launch was a whole RK stage of an advection-only model (tendencies + tracer update, 1) or the tendencies alone (0).  What the
 * launch code used, recorded when it launched; all zero before the first one.  Any pointer may be NULL. */
int32_t csi_last_advection(csi_context* ctx, int32_t* tracers_per_thread, int32_t* tile_x, int32_t* tile_y, int32_t* stage_fused);
/* The kernel of the last thermodynamic launch (csi_slab_thermo_step, csi_layered_thermo_step, a time step with thermodynamics).
 * step: 0 none yet, 1 k_slab, 2 k_layered (the numeric kernels), 3 k_slab_flux, 4 k_layered_flux (the flux-term kernels, which run once
 * a side has terms, the prescribed temperature, the snowfall or the bottom salinity is an array, or a used-flux output is bound).
 * shortwave: the SHORTWAVE term's state the kernel was compiled for -- 0 none, 1 the flux a number, 2 the flux per cell.  index: the
 * kernel's number within that family (-1 for the numeric kernels),
 *     slab      flux_bits                       + 16 * (linear + 3 * per-cell bottom salinity)
 *     layered   (flux_bits | per-cell snowfall << 4) + 32 * (linear + 3 * per-cell bottom salinity)
 * flux_bits = top ARRAY term | bottom ARRAY term << 1 | RadiativeEmission << 2 | per-cell surface temperature read << 3; linear: 0 no
 * LINEAR term, 1 its K and Ta numbers, 2 per cell.  What the launch code used, returned by the launcher when it launched.  Any pointer
 * may be NULL. */
int32_t csi_last_thermo(csi_context* ctx, int32_t* step, int32_t* shortwave, int32_t* index);
/* Kernel launches and sub-steps of the last fused sub-cycle (sub-steps / launches = sub-steps per launch). */
int32_t csi_last_launches(csi_context* ctx, int32_t* launches, int32_t* substeps);
/* Number of kernel launches issued for one sub-step in the current configuration (upper bound). */
int32_t csi_launches_per_substep(csi_context* ctx, int32_t* n);

/* ---- enthalpy-method column model: sub-steps fused on chip ----------------------------------------------------------------------------
 * The reference's EnthalpyMethodSeaIceModel with MolecularDiffusivity (src/EnthalpyMethodSeaIceModel.jl;
 * examples/diffusive_ice_column_model.jl; test/runtests.jl:9-28): Nx * Ny independent columns of Nz levels, stepped explicitly.  A
 * model of its own: an opaque csi_enthalpy made from a context for its device, stream and error text; it shares nothing else with the
 * context's sea-ice model, and a process that never creates one launches what it launched before.  Every entry runs on the context's
 * stream and none waits for the device.
 *
 * ARRAYS.  H, T, phi, kappa: caller-owned, contiguous (Nz + 2, Ny, Nx) doubles in device memory; level k = 1 .. Nz is the interior,
 * levels 0 and Nz + 1 are the z halos.  The library never reads (or writes) the halo levels of H and phi.  There are no horizontal
 * halos: the model has no horizontal operator.  Parameters: ice_heat_capacity c, water_heat_capacity (stored, never read, as in the
 * reference), fusion_enthalpy L, kappa_ice, kappa_water.
 *
 * SEMANTICS, mirrored from the reference on purpose (none of these is a fix):
 *   set T          (set!(model; T), :80-98, :146-159)  H[k] = c * T[k] + L * phi[k] with the phi held at that moment (zero for a
 *                  fresh model); two products and a sum.  T's halos are not touched.
 *   set H          (set!(model; H), :132-144)          T[k] = H[k] / c, then T's halos from its boundary conditions at `time`.
 *   Neither set updates phi or kappa: a fresh model has kappa = 0 until update_state runs, and a bare time step of it changes nothing.
 *   update_state   (:161-166), in this order:  T[k] = H[k] / c and T's halos at `time` (latent heat is ignored here, as upstream
 *                  ignores it);  phi[k] = (T[k] < 0) ? 1 : 0;  kappa[k] = kappa_ice * (1 - phi[k]) + kappa_water * phi[k], then
 *                  kappa[0] = kappa[1], kappa[Nz + 1] = kappa[Nz].  Frozen cells (phi = 1) take kappa_WATER: the reference's assignment.
 *   time step      (:168-185)  G from the current T and kappa, halos included; H[k] = H[k] + dt * G[k]; update_state at the time the
 *                  step STARTED from; then the clock t = t + dt, one addition per step.  So the boundary values that enter T's halos
 *                  after step s are those of the step's start time, not of the time it ends at.  H's own boundary conditions are
 *                  the default zero flux and contribute nothing.
 * OPERATORS (STATUS: RECALLED -- Oceananigans is not vendored; this statement is the definition, like the time indexing and the
 * fold), k = 1 .. Nz, faces k = 1 .. Nz + 1, zf the Nz + 1 faces given at creation:
 *   zc[k]   = (zf[k] + zf[k + 1]) / 2                 dzc[k] = zf[k + 1] - zf[k]
 *   dzf[k]  = zc[k] - zc[k - 1] inside the column;    dzf[1] = dzc[1] and dzf[Nz + 1] = dzc[Nz] (a Bounded stretched grid repeats its
 *                                                     end spacing)
 *   flux[k] = ((kappa[k] + kappa[k - 1]) / 2) * ((T[k] - T[k - 1]) / dzf[k])
 *   G[k]    = (flux[k + 1] - flux[k]) / dzc[k]
 *   value condition Tb at the bottom / Tt at the top:  T[0] = 2 * Tb - T[1],  T[Nz + 1] = 2 * Tt - T[Nz];  no condition (no flux):
 *   the halo takes its neighbour's value.
 * No contraction, IEEE division (three per cell and step), one arithmetic for both library modes (STRICT = FAST, as for the time
 * series and the diagnostics).
 *
 * BOUNDARY TEMPERATURES, per side: none, a number, a (Ny, Nx) device array, or a time series whose slices are scalars or (Ny, Nx)
 * planes in device memory (CSI_SERIES_DEVICE; the HOST ring backend is refused by name).  For a series the host evaluates
 * csi_time_series_plan at every sub-step's start time and hands the kernel (n1, n2, frac) per sub-step and side as kernel
 * arguments; the kernel forms (n1 == n2) ? psi_1 : psi_2 * frac + psi_1 * (1 - frac).  Any condition on H, and a flux or gradient
 * condition on T, is CSI_ERR_UNSUPPORTED.
 *
 * KERNEL FORMS (enthalpy.hip, k_enthalpy_steps: one thread per column, lanes along x, every level one coalesced plane; a thread
 * marches k upward in place, carrying the lower face's flux and the old T[k], kappa[k] in registers; no barrier, no cross-lane
 * operation):
 *   CSI_ENTH_ON_CHIP   H[1 .. Nz] and T[0 .. Nz + 1] of a wave's 64 columns live in LDS as [level][lane], (2 Nz + 2) * 512 bytes
 *                      per wave (one wave per block); one launch runs up to CSI_ENTH_MAX_SUBSTEPS sub-steps, longer requests loop
 *                      launches.  The first sub-step of a launch reads kappa from memory (the held kappa need not be the one T
 *                      implies), later ones derive it from T; after the last, H, T, phi, kappa are stored once, the halo levels
 *                      of T and kappa included.  Memory sees the state once in and once out per launch.
 *   CSI_ENTH_PER_STEP  the same body on the caller's arrays, one launch per step, for columns too deep for LDS.
 * CHOOSING RULE (csi_enthalpy_plan; pure host function, no context, no GPU): lds = (2 Nz + 2) * 512; waves = floor(163840 / lds),
 * the waves a CU's 160 KiB hold; ON_CHIP iff waves >= CSI_ENTH_MIN_WAVES_PER_CU = 2 (Nz <= 79): the smallest residency taken is two
 * waves per CU, half a wave per SIMD -- the sub-step loop is a dependent chain of IEEE divisions, and what is bought is the absent
 * memory traffic, not latency hiding.  The compiler's register count allows 8 waves per SIMD for every kernel of the unit; on chip
 * the LDS image sets the residency: waves per CU as above (Nz = 20: 7).  forced_path (the environment's CSI_ENTH_PATH, read when the
 * CONTEXT is created: 0 auto, 1 per step, 2 on chip; any other value fails csi_context_create) overrides the rule;
 * 2 where waves < 1 is CSI_ERR_UNSUPPORTED.
 *
 * ICE THICKNESS (k_enthalpy_thickness; one thread per column, a (Ny, Nx) array).  The example's diagnostic
 * (diffusive_ice_column_model.jl:115-127) made total -- this definition is OURS: kw = the number of levels from the bottom up whose
 * T >= Tm, stopping at the first that is not.  kw == 0: -zf[1].  kw == Nz: 0.  Otherwise, with ki = kw + 1,
 *   dTdz = (T[ki] - T[kw]) / dzf[ki];   z = zc[kw] + (Tm - T[kw]) / dTdz;   thickness = -z.
 * On profiles that decrease monotonically upward it equals the example's binary search.
 *
 * ERRORS: unbound arrays CSI_ERR_NOT_BOUND; dt not finite, n < 1, faces not finite or not strictly increasing, extents < 1, a
 * parameter that is not finite, c == 0: CSI_ERR_INVALID_ARGUMENT; the conditions above CSI_ERR_UNSUPPORTED.
 * csi_context_destroy frees the models that survive; a csi_enthalpy must not be used after its context is gone.
 * NOT BUILT: horizontal coupling; tiles or multi-GPU; output sets over column fields; a reciprocal-multiply FAST arithmetic; a
 * register-resident variant templated on Nz; the HOST series backend; any coupling to the sea-ice model of the context. */
typedef struct csi_enthalpy csi_enthalpy;
typedef enum { CSI_ENTH_H = 0, CSI_ENTH_T = 1, CSI_ENTH_PHI = 2, CSI_ENTH_KAPPA = 3 } csi_enthalpy_array;
typedef enum { CSI_ENTH_T_BOTTOM = 0, CSI_ENTH_T_TOP = 1, CSI_ENTH_H_BOTTOM = 2, CSI_ENTH_H_TOP = 3 } csi_enthalpy_side;
typedef enum {
    CSI_ENTH_BC_NONE = 0,            /* the default: no flux, halo = neighbour */
    CSI_ENTH_BC_NUMBER = 1,
    CSI_ENTH_BC_ARRAY = 2,           /* dev_array: (Ny, Nx) doubles */
    CSI_ENTH_BC_SERIES_SCALAR = 3,   /* ts: nt scalars, slice_stride doubles apart (ld is ignored) */
    CSI_ENTH_BC_SERIES_PLANE = 4,    /* ts: nt (Ny, Nx) planes, rows ld apart, slices slice_stride apart */
    CSI_ENTH_BC_FLUX = 5,            /* refused: CSI_ERR_UNSUPPORTED */
    CSI_ENTH_BC_GRADIENT = 6         /* refused: CSI_ERR_UNSUPPORTED */
} csi_enthalpy_bc_kind;
enum { CSI_ENTH_PER_STEP = 1, CSI_ENTH_ON_CHIP = 2 };
enum { CSI_ENTH_MAX_SUBSTEPS = 64, CSI_ENTH_MIN_WAVES_PER_CU = 2, CSI_ENTH_LDS_PER_CU = 163840 };
typedef struct {
    int32_t Nx, Ny, Nz;                /* each >= 1 */
    int32_t reserved;                  /* 0 */
    const double* z_faces;             /* host, Nz + 1 values, strictly increasing; copied */
    double ice_heat_capacity;          /* c */
    double water_heat_capacity;        /* stored, never read */
    double fusion_enthalpy;            /* L */
    double kappa_ice, kappa_water;
} csi_enthalpy_params;
typedef struct {
    int32_t form;                      /* CSI_ENTH_PER_STEP | CSI_ENTH_ON_CHIP; 0: no time step yet */
    int32_t launches;                  /* of the last csi_enthalpy_time_step */
    int32_t substeps_per_launch;       /* of its first launch: min(n, CSI_ENTH_MAX_SUBSTEPS) on chip, 1 per step */
    int32_t lds_bytes;                 /* per block; 0 per step */
} csi_enthalpy_launch;
/* The choosing rule.  Any output pointer may be NULL.  Nz < 1 or forced_path outside 0 .. 2: CSI_ERR_INVALID_ARGUMENT. */
int32_t csi_enthalpy_plan(int32_t Nz, int32_t forced_path, int32_t* form, int64_t* lds_bytes, int32_t* waves_per_cu,
                          int32_t* max_substeps);
int32_t csi_enthalpy_create(csi_context* ctx, const csi_enthalpy_params* p, csi_enthalpy** out);
int32_t csi_enthalpy_destroy(csi_enthalpy* e);
int32_t csi_enthalpy_bind(csi_enthalpy* e, int32_t which, void* dev);
/* kind NUMBER reads `number`, ARRAY `dev_array`, the SERIES kinds `ts` (times are copied; the data stay the caller's). */
int32_t csi_enthalpy_boundary_set(csi_enthalpy* e, int32_t side, int32_t kind, double number, const void* dev_array,
                                  const csi_time_series* ts);
/* which: CSI_ENTH_T or CSI_ENTH_H -- the set semantics above, applied to what the caller wrote into that bound array. */
int32_t csi_enthalpy_set(csi_enthalpy* e, int32_t which, double time);
int32_t csi_enthalpy_update_state(csi_enthalpy* e, double time);
/* n steps of dt from `time`; *time_out (may be NULL): the clock after them, n additions. */
int32_t csi_enthalpy_time_step(csi_enthalpy* e, double dt, int32_t n, double time, double* time_out);
int32_t csi_enthalpy_last_launch(csi_enthalpy* e, csi_enthalpy_launch* out);
int32_t csi_enthalpy_ice_thickness(csi_enthalpy* e, double Tm, void* dev_out);

/* ---- Lagrangian ice drifters --------------------------------------------------------------------------------------------------------
 * Points that move with the ice: buoy tracks, "where did this floe come from".  Oceananigans gives its ocean models LagrangianParticles;
 * SeaIceModel has no counterpart in the reference, so THIS COMMENT IS THE DEFINITION (tests/drifters_ref.py restates it in NumPy, and
 * csrc/drifters_dev.h, a host-and-device header, is the one C statement of it: the kernels and the host function below call it).
 * Nothing here changes another entry point: a context that never makes these calls launches exactly what it launched before.  One code
 * serves STRICT and FAST, compiled without contraction; every division below is an IEEE division: both modes give the same bits.
 *
 * POSITION.  A drifter has an index-space position (xi, eta) in doubles, xi in [0, Nx], eta in [0, Ny].  Cell (i, j) (1-based, as
 * everywhere) covers [i - 1, i) x [j - 1, j); u[i, j] sits at (i - 1, j - 1/2), v[i, j] at (i - 1/2, j - 1), cell centres at
 * (i - 1/2, j - 1/2).  The arrays xi, eta (double) and status (int32) are the CALLER's device arrays, n entries each, handed over in a
 * csi_drifters at every call: the library keeps no drifter state.
 *
 * RATES, in cells per second:  A[i, j] = u[i, j] / dx^fc[i, j],  B[i, j] = v[i, j] / dy^cf[i, j]  (the metrics every operator reads at
 * the u and v points, at all three metric kinds).  Each is ONE correctly rounded division of two stored doubles, so its value does not
 * depend on whether it is formed where it is used (as the kernel does) or in a pass of its own.
 *
 * LOCATE.  With fl(x, lo, hi) = fmin(fmax(floor(x), lo), hi) -- the clamps are applied to the DOUBLE, before the conversion to an
 * integer, and fmax / fmin return their other argument for a NaN, so every input value, NaN and +-Inf included, gives an index inside
 * the one ring named below.  This is part of the contract, not an optimisation.
 *   A at (xi, eta):  fx = fl(xi, 0, Nx - 1), sx = xi - fx;  t = eta - 0.5, fy = fl(t, -1, Ny - 1), sy = t - fy;
 *                    columns ia = fx + 1, ia + 1;  rows ja = fy + 1, ja + 1  (rows 0 and Ny + 1, the first halo ring, are read);
 *                    a = (1 - sy) * ((1 - sx) * A[ia, ja] + sx * A[ia + 1, ja]) + sy * ((1 - sx) * A[ia, ja + 1] + sx * A[ia + 1, ja + 1])
 *   B at (xi, eta):  the same with the roles of x and y exchanged:  gy = fl(eta, 0, Ny - 1), ry = eta - gy;  s = xi - 0.5,
 *                    gx = fl(s, -1, Nx - 1), rx = s - gx;  columns ib = gx + 1, ib + 1;  rows jb = gy + 1, jb + 1;
 *                    b = (1 - rx) * ((1 - ry) * B[ib, jb] + ry * B[ib, jb + 1]) + rx * ((1 - ry) * B[ib + 1, jb] + ry * B[ib + 1, jb + 1])
 *   rate(xi, eta) = (a, b).  Every product and sum is rounded on its own, in the order written (no contraction).
 *   The CONTAINING CELL of (xi, eta) is (ic, jc) = (fl(xi, 0, Nx - 1) + 1, fl(eta, 0, Ny - 1) + 1): a point on the last face belongs
 *   to the last cell.
 * csi_drifters_locate(Nx, Ny, xi, eta, idx, w) is that rule as a pure host function (no context, no GPU): idx[6] = {ia, ja, ib, jb, ic,
 * jc}, w[4] = {sx, sy, rx, ry}.  Nx < 1 or Ny < 1 or a NULL pointer: CSI_ERR_INVALID_ARGUMENT; any xi, eta is accepted.
 *
 * NORM, of one coordinate x in a direction of N cells; it returns the coordinate and may raise a status bit.
 *   Periodic:  r = x - N * floor(x / N);  where r >= N or r < 0, r = 0.  (A tiny negative x gives r == N exactly after rounding, and a
 *              quotient that rounds up to a whole number gives a tiny negative r: both stand for the seam, 0.  A NaN stays a NaN.)
 *   Bounded:   r = x < 0 ? 0 : (x > N ? N : x);  CSI_DRIFTER_CLAMPED_X / _Y is raised when r != x.  (A NaN stays a NaN, no bit.)
 *
 * ONE SUB-STEP of length tau (midpoint rule; the velocities are frozen at the state the call finds):
 *   (a1, b1) = rate(xi, eta)
 *   xm = norm_x(xi + (tau / 2) * a1),  ym = norm_y(eta + (tau / 2) * b1)
 *   (a2, b2) = rate(xm, ym)
 *   X = xi + tau * a2,  Y = eta + tau * b2;  xn = norm_x(X),  yn = norm_y(Y)          (the bits of all four norms are kept)
 *   LOST:  where X, Y, xn or yn is not finite, the drifter becomes (NaN, NaN), CSI_DRIFTER_LOST is raised and the advance ends for it.
 *   LAND:  otherwise, with a mask set (csi_mask_set), if the byte of the containing cell of (xn, yn) is 0 the drifter keeps (xi, eta)
 *          and CSI_DRIFTER_HELD is raised; each sub-step is judged on its own.  Otherwise (xi, eta) = (xn, yn).
 * csi_drifters_advance(ctx, d, dt, substeps) runs m = substeps sub-steps of tau = dt / m (formed once, on the host) in ONE launch on
 * the context's stream, one thread per drifter: position and status are read once and stored once.  A drifter with a non-finite
 * coordinate at entry is INACTIVE: nothing is read for it, its position is left as it is and its status becomes CSI_DRIFTER_INACTIVE.
 * For every other drifter status becomes the OR of the bits its sub-steps raised (0: it moved freely).  Hence, for the POSITIONS,
 * advance(dt, m) gives the bits of m calls advance(dt / m, 1) while the velocities stand still.
 *
 * HALO ELEMENTS READ (the entry points fill none): u and dx^fc at columns 1 .. Nx + 1, rows 0 .. Ny + 1; v and dy^cf at columns
 * 0 .. Nx + 1, rows 1 .. Ny + 1; the mask, h, aice, hs at the interior only.  On a Bounded high side column Nx + 1 / row Ny + 1 of a
 * Face field is its last face, elsewhere the first halo element.  Nothing else outside the interior is read, whatever it holds.
 * csi_update_state and every step entry point leave these elements valid, as stated for csi_derived_compute above.
 *
 * SAMPLING.  csi_drifters_sample(ctx, d, columns, dev_out, ld) writes, in ONE launch, the requested columns at the current positions:
 * column k (the k-th set bit of `columns`, counted from bit 0) of drifter q at dev_out[k * ld + q], doubles, ld >= n: the layout is a
 * function of the column mask alone.  XI, ETA: the position.  U, V: the bilinear form above with the weights of A / of B applied to
 * u / to v themselves (m/s along the grid's local directions).  H, A, HS: the containing cell's value of CSI_F_H, CSI_F_A, CSI_F_HS,
 * copied.  An inactive drifter (non-finite coordinate) receives NaN in every column.
 *
 * Neither entry waits for the device.  n == 0 is a no-op without a launch.  csi_drifters_stats: launches of the two kernels made on
 * the context so far (tests; the pointer may be NULL).
 * ERRORS, by name.  CSI_ERR_NOT_BOUND: the grid; u or v; h, aice or hs where their column is requested.  CSI_ERR_INVALID_ARGUMENT:
 * d == NULL, n < 0, a NULL array with n > 0, dt not finite, substeps < 1, columns == 0 or an unknown bit, dev_out == NULL, ld < n, a
 * grid with halo < 1.  CSI_ERR_UNSUPPORTED: a tiled context (a drifter would have to migrate between ranks) and the RIGHT_FOLDED
 * topologies (crossing the fold re-orients the drifter).
 * NOT BUILT: tiles; the fold; sorting or binning the drifters by cell; deformation from drifter triplets; sampling of derived or
 * momentum term fields; asynchronous staging of the sampled records. */
#define CSI_DRIFTER_CLAMPED_X 1
#define CSI_DRIFTER_CLAMPED_Y 2
#define CSI_DRIFTER_HELD 4
#define CSI_DRIFTER_LOST 8
#define CSI_DRIFTER_INACTIVE 16
#define CSI_DRIFTER_COL_XI 1
#define CSI_DRIFTER_COL_ETA 2
#define CSI_DRIFTER_COL_U 4
#define CSI_DRIFTER_COL_V 8
#define CSI_DRIFTER_COL_H 16
#define CSI_DRIFTER_COL_A 32
#define CSI_DRIFTER_COL_HS 64
#define CSI_DRIFTER_COL_ALL 127
typedef struct {
    int64_t n;                         /* drifters; >= 0 */
    double* xi;                        /* device, n doubles */
    double* eta;                       /* device, n doubles */
    int32_t* status;                   /* device, n int32: rewritten by every advance */
} csi_drifters;
int32_t csi_drifters_locate(int32_t Nx, int32_t Ny, double xi, double eta, int32_t* idx, double* w);
int32_t csi_drifters_advance(csi_context* ctx, const csi_drifters* d, double dt, int32_t substeps);
int32_t csi_drifters_sample(csi_context* ctx, const csi_drifters* d, int32_t columns, void* dev_out, int64_t ld);
int32_t csi_drifters_stats(csi_context* ctx, int64_t* launches);

/* ---- per-region ice integrals and extrema ---------------------------------------------------------------------------------------------
 * The tracer group of csi_diagnostics_compute, per region of a caller-supplied map, in ONE call: Arctic and Antarctic extent, extent and
 * volume per basin, totals per latitude band.  Stands where users of the reference copy h, aice, hs and the metrics to the host and bin
 * them there (a wait for the stream, whole parents over the bus, sums in the host library's order).
 *
 * A REGION MAP is a device array of int32 laid out like a (c,c) parent with leading dimension ld -- as the mask of csi_mask_set is: the
 * id of cell (i, j) at ids[(i + Hx - 1) + (j + Hy - 1) * ld].  Only i = 1 .. Nx, j = 1 .. Ny are read, whatever the halo elements hold.
 * n_regions is between 1 and CSI_REGIONS_MAX = 64.  A cell BELONGS TO REGION r when its id equals r and it is active (no mask set, or
 * its mask byte != 0).  An id outside 0 .. n_regions - 1 -- negative ids, INT32_MIN and INT32_MAX included -- belongs to no region; the
 * ACTIVE cells with such an id are counted in *unassigned_cells.  No id value forms an address: ids are compared, never used as an index.
 * The caller's array is passed at every call; the library keeps no map (as with csi_drifters).
 *
 * out[r], r = 0 .. n_regions - 1 (HOST memory), holds the tracer group restricted to the cells of region r:
 *   ice_volume = sum (h * aice) * Az     ice_area = sum aice * Az     ice_extent = sum Az over cells with aice >= extent_threshold
 *   snow_volume = sum (hs * aice) * Az   region_area = sum Az         (Az = Az^cc; products in the order written, uncontracted)
 *   min_h, max_h, min_aice, max_aice, max_hs   (NaN elements are skipped; -0.0 and +0.0 compare equal and either may be returned)
 *   cells               the number of cells of r
 * exactly as stated for CSI_DIAG_TRACERS above.  snow_volume and max_hs without a bound CSI_F_HS hold the "not computed" value NaN.
 * A region with no cell returns +0.0 for the sums, +Inf for the minima, -Inf for the maxima and 0 for cells.
 *
 * SUMMATION ORDER: the one stated for csi_diagnostics_compute above, a function of (Nx, Ny) alone -- it does not depend on the map.  A
 * cell that does not belong to r contributes the identity to r's record: +0.0 to a sum, +Inf to a minimum, -Inf to a maximum, 0 to
 * cells.  Hence out[r] equals, BIT FOR BIT, what csi_diagnostics_compute(CSI_DIAG_TRACERS) returns on the same fields when the mask is
 * replaced by `mask AND (id == r)` (region_area = its active_area, cells = its active_cells).
 *
 * Two launches on the context's stream -- a pass over the interior that leaves, per block of 64 x 64 cells, one record per region (a
 * block folds only the regions that occur in its tile; the others get identity records) and a finishing launch of n_regions + 1 blocks,
 * block r folding region r's records as step 4 above, the last one the count of the cells of no region --, one copy of the folded slots
 * to page-locked host memory and one wait for the stream.  No atomics in device memory, no flags, no hand-off between workgroups inside
 * a launch: the same bits from call to call, in STRICT and FAST mode.  The record buffer is the context's, allocated at the first call
 * and only growing; csi_regions_layout(Nx, Ny, n_regions, &records, &bytes) is its size as a pure host function (no context, no GPU):
 *   records = ceil(Nx / 64) * ceil(Ny / 64)     bytes = records * (n_regions + 1) * 11 * 8
 * (Nx < 1, Ny < 1 or n_regions outside 1 .. 64: CSI_ERR_INVALID_ARGUMENT; either output pointer may be NULL.)  csi_regions_stats:
 * launches made by csi_regions_compute on this context so far (two per call); a model that never asks makes none.
 *
 * Tiled contexts: the call is COLLECTIVE, exactly like csi_diagnostics_compute.  Each rank passes ITS piece of the map (laid out like
 * its own (c,c) parents), reduces its own interior, the ranks all-gather n_regions x 11 slots and the count, and every rank combines
 * them on the host in rank order: all ranks return the same bits, and sums differ from the untiled run's by rounding only.  A rank that
 * fails locally still takes part in the all-gather; then every rank returns an error.
 *
 * Errors, by name: CSI_ERR_NOT_BOUND for a missing h or aice (and the grid); CSI_ERR_INVALID_ARGUMENT for r == NULL, NULL ids or out,
 * n_regions outside 1 .. 64, ld < Nx + 2 Hx, an extent_threshold that is negative or not finite, reserved != 0.
 * NOT BUILT: more than 64 regions per call (call again with another map); overlapping regions; the velocity group or the non-finite
 * counts per region; regional energy or momentum budgets; region maps as bound slots or as time series. */
#define CSI_REGIONS_MAX 64
typedef struct {
    const int32_t* ids;                /* device, laid out like a (c,c) parent */
    int64_t ld;                        /* >= Nx + 2 Hx */
    int32_t n_regions;                 /* 1 .. CSI_REGIONS_MAX */
    int32_t reserved;                  /* 0 */
} csi_regions;
typedef struct {
    double ice_volume, ice_area, ice_extent, snow_volume, region_area;
    double min_h, max_h, min_aice, max_aice, max_hs;
    int64_t cells;
} csi_region_record;
int32_t csi_regions_layout(int32_t Nx, int32_t Ny, int32_t n_regions, int64_t* records, int64_t* bytes);
int32_t csi_regions_compute(csi_context* ctx, const csi_regions* r, double extent_threshold, csi_region_record* out, int64_t* unassigned_cells);
int32_t csi_regions_stats(csi_context* ctx, int64_t* launches);

/* ---- advected ice tracers and ice age ---------------------------------------------------------------------------------------------------
 * Properties carried WITH the ice: a dye, the age of the ice.  SeaIceModel(grid; tracers = ...) of the reference makes its tracers
 * prognostic fields (sea_ice_model.jl:151, 164-189) but never steps them: its tendency kernel ignores the argument
 * (tracer_tendency_kernel_functions.jl:27-45).  So THIS COMMENT IS THE DEFINITION.  It is not free-floating: the reference has exactly
 * one generic third tracer, the snow thickness hs -- tendency -horizontal_div_Uc(hs) (:49-52), update max(0, hs^- + dt G), zero where
 * aice <= 0 (sea_ice_fe_step.jl:86-94) -- and a PLAIN tracer follows that rule statement for statement; tests/tracers_ref.py restates
 * both halves below in NumPy with G taken from the oracle's hs.
 * Nothing here changes another entry point: a context without tracers launches exactly what it launched before.
 *
 * Up to CSI_TRACERS_MAX = 8 tracers.  Each is a (Center, Center) device array of the CALLER's with the parent shape of the array bound to
 * CSI_F_H (same leading dimension, rows, halos); G[k], where given, likewise.  Per tracer:
 *   weighting    CSI_TRACER_PLAIN (0) | CSI_TRACER_BY_CONCENTRATION (1)
 *   nonnegative  0 | 1
 *   source       a rate per second (finite)
 *
 * One stage with stage step dtau uses BASE fields c^-, aice^-: under RK3 (from_cache) the base is Psi^- -- c^- a library-owned copy
 * made by csi_cache_current_fields, aice^- = CSI_F_AM --, under FE the current fields.
 *
 * FIRST HALF (csi_tracers_tendencies).  It runs where compute_tracer_tendencies! runs: after the h / aice tendency launch and BEFORE the
 * momentum step, so it sees the velocities, scheme, weight dtype and mode h sees.
 *   PLAIN:             G = -horizontal_div_Uc(c);   c* = c^- + dtau * G
 *   BY_CONCENTRATION:  q = aice * c at every stencil point (ONE rounded product, never contracted into the reconstruction);
 *                      G = -horizontal_div_Uc(q);
 *                      aice* = aice^- + dtau * Ga, Ga the array bound to CSI_F_GA as just written: the tracer update's own expression
 *                      BEFORE its clips;
 *                      c* = aice* > 0 ? ((aice^- * c^-) + dtau * G) / aice* : 0, an IEEE division in both modes.
 *                      Ridging (aice* > 1 -> 1) therefore leaves c unchanged.
 *   c* goes to a library-owned interior array; G goes to the caller's G[k] where one is given (NULL: not stored).
 *   scheme == 0: G = 0 and no stencil launch is made (c* is formed by one point-wise launch, counted with the update launches).
 * SECOND HALF (csi_tracers_update).  It runs at the end of the stage, after the thermodynamic step and before update_state!, and reads
 * the stage-final aice:
 *   x = nonnegative ? jmax(0, c*) : c*           (jmax: Julia's max, NaN if either is NaN)
 *   c = (aice > 0 and the cell is active) ? x + dtau * source : 0
 *   and the store writes the local halo images, as hs gets them.
 * Without thermodynamics and with source = 0, nonnegative = 1, PLAIN this is dynamic_step_snow! followed by update_state!'s mask, bit
 * for bit.  STRICT: the oracle's operations; FAST: the reconstructions of the FAST h / aice tendencies (|dG| <= 1e-12 max|G|), the
 * update's arithmetic the same code in both modes.
 * RK3: every stage restarts from Psi^- with its own dtau, so the LAST stage is the step's result and a source accrues dt per step, not
 * 11/6 of it (the argument made for the mixed layer above).  For that to hold for ice that MOVES as well, the source of one stage must not
 * travel with the next stage's fluxes: from the second stage on, the stencil of a tracer with source != 0 reads the stage before WITHOUT
 * its source -- the second half also stores  (aice > 0 and the cell is active) ? x : 0  with its halo images into a library-owned array,
 * and that array is the stencil's input until the next csi_cache_current_fields.  (Otherwise ice that enters an ice-free cell brings the
 * earlier stages' increments with it and ends the step with 11/6 dt of age.)  The first stage, ForwardEuler and tracers without a source
 * read the tracer itself.  Hence 0 <= age <= t under both steppers for a scheme whose reconstruction is a convex combination, and to the
 * WENO-Z inhomogeneity (about 2e-8 per stencil evaluation for WENO7) otherwise.
 * STATED LIMITS.  Growth does not dilute c.  There is no volume weighting: V = h aice is not transported conservatively by the
 * reference, so q / V would not keep a uniform field uniform.  PLAIN tracers are densities: in divergent flow a uniform plain tracer
 * does not stay uniform -- the reference's hs behaviour.
 *
 * csi_tracers_set(ctx, t) copies the struct (t == NULL removes the tracers).  csi_time_step_fe / _rk3 then run both halves where
 * stated, csi_cache_current_fields also copies c -> c^- (a copy batch of its own), csi_update_state images and masks the tracers as it
 * does hs, and a context with tracers takes the general stage loop (csi_last_advection reports stage_fused = 0).
 * csi_tracers_stats: launches of the stencil kernel / of the point-wise kernels so far; csi_tracers_last: what the last stencil launch
 * used -- tracers per thread (1, 2 or 4), the cells of a flux tile, the tracer groups (blockIdx.z).  Results do not depend on them.
 * Output: csi_output_field.field_id also accepts CSI_TRACER_FIELD(k) once tracers are set (snapshot, average, masked fill, as for any
 * (Center, Center) field); csi_tracers_set after csi_output_create invalidates such a set, like a re-bind.
 * ERRORS, by name.  CSI_ERR_INVALID_ARGUMENT: n outside 1 .. 8, a NULL c[k], an unknown weighting or nonnegative value, a non-finite
 * source, arrays that alias each other or h, aice, hs as bound at the call (fields bound later and the tendency arrays Gh, Ga are not
 * checked), an array whose device allocation ends before a whole parent of h behind the pointer -- a sub-allocating allocator's large
 * blocks pass this test: it catches a gross mistake, not every short array --, a dt that is not finite.  CSI_ERR_NOT_BOUND: the grid, h, aice (their shape is
 * the tracers'), and at a step u, v, CSI_F_GA (BY_CONCENTRATION), CSI_F_AM (from_cache).  CSI_ERR_UNSUPPORTED: tiled contexts, whichever
 * of csi_tile_set / csi_tracers_set comes second.
 * NOT BUILT: tiles and multi-GPU; tracer integrals in diagnostics or regions; per-tracer schemes; time-series or array-valued sources;
 * volume weighting; tracers in the fused advection-only stage launch; tracers as bound slots. */
#define CSI_TRACERS_MAX 8
#define CSI_TRACER_PLAIN 0
#define CSI_TRACER_BY_CONCENTRATION 1
#define CSI_TRACER_FIELD(k) (4096 + (k))
typedef struct {
    int32_t n;                             /* 1 .. CSI_TRACERS_MAX */
    double* c[CSI_TRACERS_MAX];            /* device, parent shape of CSI_F_H */
    double* G[CSI_TRACERS_MAX];            /* device, the same shape; NULL: the tendency is not stored */
    int32_t weighting[CSI_TRACERS_MAX];
    int32_t nonnegative[CSI_TRACERS_MAX];
    double source[CSI_TRACERS_MAX];
} csi_tracers;
int32_t csi_tracers_set(csi_context* ctx, const csi_tracers* t);
int32_t csi_tracers_tendencies(csi_context* ctx, int32_t scheme, double dt, int32_t from_cache);
int32_t csi_tracers_update(csi_context* ctx, double dt);
int32_t csi_tracers_stats(csi_context* ctx, int64_t* stencil_launches, int64_t* update_launches);
int32_t csi_tracers_last(csi_context* ctx, int32_t* tracers_per_thread, int32_t* tile_x, int32_t* tile_y, int32_t* groups);

#ifdef __cplusplus
}
#endif
#endif /* CSI_H */
