// csi_ctx.h -- the host side of libcsi_hip.so: the context, the tile groups and what the translation units of the host code share.
//   csi_core.hip    context helpers, index ranges, launch geometries of the fused kernels
//   csi_group.hip   halo exchange: RCCL, the in-process tile group, the host-channel group (csi_hostgroup.hip)
//   csi_peer.hip    peer halo transport: set-up (IPC mapping, flag arrays), tile sets, kernel tables
//   csi_fold.hip    north fold: the three-kernel band beside the pair launches
//   csi_launch.hip  launch loops: sub-cycle, finalize, time_step_momentum!, tracer steps, update_state!, csi_profile_substeps
//   csi_step.hip    whole steps: the checks both steppers share, one step stage, the one-launch RK stages, cache_current_fields!
//   csi_abi.hip     the C ABI (include/csi.h): argument checks, binding, settings, the entry points
//   csi_thermo.hip  thermodynamics: parameter structs, the choice of kernel and its binding checks, the mixed layer's launch, their entry points
//   csi_time_series.hip   forcing time series: time indexing, the device ring of a host-resident series, the interpolation launch
//   csi_diagnostics.hip   device diagnostics: the two launches, the result copy, the combine over the ranks of a decomposition
//   csi_output.hip        device-side output: output sets, their staging slots, the copy stream and the slot events
//   csi_derived.hip       derived fields and energy budget integrals: binding checks, the launches, the budget's combine over the ranks
//   csi_momentum_terms.hip   momentum balance terms and their power: binding checks, the launches, the power sums' combine over the ranks
//   csi_enthalpy.hip      the enthalpy-method column model: the choosing rule, the model object, its launches
//   csi_drifters.hip      Lagrangian ice drifters: the locate rule on the host, argument and binding checks, the two launches
//   csi_regions.hip       per-region ice integrals: argument and binding checks, the two launches, the combine over the ranks
//   csi_tracers.hip       advected ice tracers: argument checks, the library-owned c* and Psi^- arrays, the two halves of a stage
//   csi_slots.h     the field slots: id, display name, location and roles of each, one row per slot
//   csi_mem.h       DeviceBuf / PinnedBuf: the owner of every allocation the library makes
#pragma once
#include "../../include/csi.h"
#include "csi_dev.h"
#include "csi_slots.h"
#include "csi_kernels.h"
#include "momentum_dev.h"
#include "csi_hostgroup.h"
#include "csi_comm.h"
#include "csi_mem.h"
#include <rccl/rccl.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <vector>
#include <algorithm>
#include <initializer_list>

using namespace csi;

namespace csi_host {


struct Bound {
    double* p = nullptr;
    int64_t ld = 0;
    int ni = 0, nj = 0;
};

extern std::string g_create_error;      // csi_context_create failures (no context to hold the message)

// A library array that shadows the parent array of a bound field: as many elements (ld * nj), the same row stride, and a view
// whose element (i, j) is the field's.  `zeroed`: cleared on the context's stream whenever it is (re)allocated -- for arrays with
// cells that no kernel ever writes but some kernel reads.
struct ScratchField {
    int fid;
    bool zeroed;
    DeviceBuf<double> buf;
    ScratchField(int field, bool zero) : fid(field), zeroed(zero) {}
    double* get() const { return buf.get(); }
    // sized for c->f[fid] as it is bound now (Buf::ensure: no HIP call while the size stays)
    hipError_t ensure(const csi_context* c, hipStream_t also = nullptr, bool* fresh = nullptr);
    FRef view(const csi_context* c) const;
};
constexpr bool kZeroed = true, kRaw = false;


}  // namespace csi_host
using namespace csi_host;

// ---- in-process tile group (csi_local_group_create / csi_comm_init_local) --------------------------------------------------
// Several contexts of ONE process, one host thread each, exchange halos through device-to-device copies: what RCCL's grouped
// ncclSend / ncclRecv do between processes, with the same matching rule (messages between a pair of ranks match in the order
// they were posted).  Host-synchronous -- a sender waits for its pack kernel before it posts, a receiver for its copies before
// it acknowledges -- because it exists for correctness runs of real decompositions on one GPU (RCCL refuses two ranks on one
// device), not for speed.  The peer halo transport on such a group addresses the neighbours' arrays directly.
struct csi_local_group {
    struct Msg { const double* ptr; size_t count; };
    int world = 0;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::deque<Msg>> box;              // [src * world + dst]
    std::vector<long> posted, consumed;            // per sender: messages posted / copied out of its send buffer
    // collectives (all ranks call them in the same order)
    std::vector<std::vector<uint8_t>> payload;
    long arrived = 0, generation = 0;
    int joined = 0;
    std::vector<int> device;                       // per rank: the HIP device of its context (-1: not joined); peer_effective_tier
};

// One forcing time series (csi_time_series_set): the caller's description, and for the HOST backend the device ring with its slot table.
struct TimeSeries {
    int fid = -1;
    int nt = 0, indexing = 0, backend = 0, window = 0;
    double period = 0.0;
    std::vector<double> times;           // copied: the caller's array need not outlive the call
    const double* data = nullptr;        // device (DEVICE) / host (HOST) pointer to all nt slices, the caller's
    int64_t ld = 0, slice_stride = 0;    // doubles between rows / slices of `data`
    int nx = 0, ny = 0;                  // slice shape: the interior of the bound field
    // ---- HOST backend
    DeviceBuf<double> ring;              // `window` slices, rows ring_ld apart, slices ring_stride apart, first element at ring_off
    int64_t ring_ld = 0, ring_stride = 0, ring_off = 0;
    bool data_pinned = false;            // the caller's host memory is page-locked: slices are copied from it directly
    PinnedBuf<double> stage;             // else: one packed nx * ny staging slice per ring slot
    struct Slot {
        int slice = -1;                  // the slice the slot holds (-1: none)
        long used = 0;                   // the update that last read it (eviction: least recently used)
        hipEvent_t uploaded = nullptr;   // recorded on the copy stream behind the slot's upload
        bool pending = false;            // the context's stream has not yet been made to wait for `uploaded`
        bool staged = false;             // the slot's staging slice has been the source of a copy (wait for `uploaded` before rewriting it)
    };
    std::vector<Slot> slots;
    int64_t uploads = 0;                 // slice uploads since csi_time_series_set
    int cur[2] = {-1, -1}, next = -1;    // the newest update's pair and the slice wanted after it (series_prefetch)
};

// One regridding map (csi_regrid_map_create): the caller's arrays, validated and kept on the host, and their device layout
// (csi_kernels.h RegridDesc), packed when the first slot that needs it is set: a layout per alignment pattern of the destination rows
// (the first interior row starts on a 16-byte boundary or 8 bytes behind one; the row stride is even or odd).
struct RegridMap {
    bool live = false;
    int location = 0, nx = 0, ny = 0, src_nx = 0, src_ny = 0;
    bool rotation = false;
    std::vector<unsigned long long> idx;         // {i0, i1, j0, j1} as uint16, ny * nx
    std::vector<double> wx, wy, cs, sn;
    int64_t mld = 0, plane = 0;                  // entries between rows / planes of a device layout
    DeviceBuf<unsigned long long> dev[4];        // [head of row 0 * 2 + (ld odd)]
};

// One regridded slot (csi_time_series_set_regridded): a scalar's source series, or the east and the north series of a vector pair
// -- each a TimeSeries whose slices have the source shape, with a ring of its own on the HOST backend.
struct RegridSeries {
    int fid = -1, map = -1, parts = 1, component = 0;
    int variant = 0;                     // which device layout of the map the bound array's rows select
    int64_t dst_ld = 0;                  // ... and the row stride it was chosen for
    TimeSeries part[2];
};

// One output set (csi_output_create): the caller's field list, what the fields were bound to then, the record layout, the averaged
// fields' accumulators and the staging slots on both sides of the bus.
struct OutputSet {
    bool live = false;
    int n = 0, slots = 0;
    csi_output_field f[kMaxOutputFields];
    Bound sig[kMaxOutputFields];         // the binding of each field at creation: another one since invalidates the set
    long grid_gen = 0;                   // ... and the csi_grid_set count then
    int nx[kMaxOutputFields], ny[kMaxOutputFields];
    int64_t off[kMaxOutputFields];       // byte offset of field k in a record (a multiple of 256)
    int64_t record_bytes = 0;            // a multiple of 256
    int64_t acc_off[kMaxOutputFields];   // averaged fields: first element of the accumulator in `acc` (doubles, even)
    DeviceBuf<double> acc;               // zeroed at creation and by every pack launch
    DeviceBuf<uint8_t> stage;            // slots records
    PinnedBuf<uint8_t> host;             // slots records, page-locked
    std::vector<hipEvent_t> packed;      // per slot: recorded on the context's stream behind the pack launch
    std::vector<hipEvent_t> done;        // per slot: recorded on the copy stream behind the copy to `host`
    std::vector<int> in_flight;          // per slot: 0 free, 1 from csi_output_snapshot to csi_output_release
    double W = 0.0;                      // sum of the weights since the last snapshot
    bool any_averaged = false;
};
constexpr int kMaxOutputSets = 4;

struct csi_context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    bool grid_set = false, evp_set = false;
    int Nx = 0, Ny = 0, Hx = 0, Hy = 0, topo_x = 0, topo_y = 0, metric_kind = 0;
    GridDev g{};
    DeviceBuf<double> dev_metrics;   // 8 vectors of length Ny + 2Hy + 1 (PER_J) or 12 planes (FULL)
    DeviceBuf<double> dev_coef;      // FAST per-row stencil coefficients [Ny + 2Hy + 1][FC_COUNT]
    DeviceBuf<double> dev_coef2;     // FAST per-point stencil coefficients of a CSI_METRIC_FULL grid, C2_COUNT planes
    FastCoef coef{};
    std::vector<double> coef_host;       // host copy of the per-row table built from PER_J metrics (empty: uniform metrics)
    std::vector<double> fcor_rows[2];    // csi_coriolis_rows_set: f per row at u / v points (empty: FPlane scalar)
    DeviceBuf<double> dev_fcor;          // the same on the device (STRICT kernels), 2 x (Ny + 2Hy + 1)
    DeviceBuf<double> dev_fcor2;         // csi_coriolis_points_set: two planes (u points, v points) of ni x nj
    long fcor2_ld = 0, fcor2_plane = 0;
    bool cor_dirty = true;               // Coriolis columns of the FAST table need (re)building
    double cor_synced = 0.0;             // FPlane value they were built with
    Bound f[kSlotCount];
    csi_evp_params evp{};
    csi_stress stress[2]{};
    int mode = CSI_MODE_STRICT;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // csi_subcycle_stats_begin / _end: one more event pair around every sub-step loop while `on` (bench.py's timed region)
    struct Stats { bool on = false; std::vector<hipEvent_t> ev; std::vector<int> launches; } stats;
    // What the last sub-cycle did (csi_last_subcycle_ms, csi_last_path, csi_last_launches, csi_launches_per_substep).  A path assigns the
    // whole record in ONE statement and names there what it carries over from the record before.
    struct LastPath {
        bool timed = false;              // ev0 / ev1 bracket a sub-cycle
        int fused = 0;                   // level: 0 three kernels (or another rheology / solver), 1 one sub-step per launch, 2 pairs
        int per_substep = 0;             // launches per sub-step, the halo exchange's included
        int launches = 0, substeps = 0;  // kernel launches / sub-steps
        int exchanges = 0, k = 1;        // halo exchanges, sub-steps per exchange
    } last;
    int last_used_pairs = 0;             // run_fused: the sub-cycle ran pair launches
    // multi-GPU tiles
    TileInfo tile;
    ncclComm_t comm = nullptr;
    csi_local_group* local = nullptr;      // in-process tile group instead of an RCCL communicator (csi_comm_init_local)
    HostGroup* hostg = nullptr;            // host-channel group of PROCESSES (shared memory + HIP IPC, csi_comm_init_host): RCCL-free runs of several ranks on one GPU
    int world = 1, rank = 0;
    DeviceBuf<double> sendbuf, recvbuf;    // pack buffers of the message exchange: they only grow, both to the same size (exchange_refs)
    // Halo transport of the two-sub-steps kernel on tiles.  "peer" (default where it can be set up): the neighbouring tiles'
    // arrays are mapped into this process (HIP IPC; xGMI peer access) and a connected side behaves like a periodic one whose halo
    // lives on another GPU -- the owner's stores write the halo images straight into the neighbour's arrays, and flags in
    // device memory order the launches of neighbouring ranks (evp_fused2.hip): no pack, no RCCL kernel, no unpack, no widened
    // halo.  "rccl": ncclSend / ncclRecv of width-2k strips every k sub-steps (the fallback, and what every other path uses).
    struct Peer {
        static constexpr int NARR = 14;      // u, v, sigma11, sigma22, sigma12 (caller's), the same five (library's ping-pong copies), alpha, zeta_c, zeta_f, Delta
        static constexpr int SLOTS = kPeerSlots;   // flag slots per direction (the last one is the block's abort word)
        int want = 1;                        // csi_set_halo_transport: 1 peer where possible, 0 RCCL only
        int dld[8][2] = {};                  // per direction x {Center, Face in x}: the neighbour's row stride minus this tile's, bytes
        int nbr_wait[8] = {};                // flags to wait for per direction: the size of the NEIGHBOUR's opposite set (its own geometry)
        int ny_below = 0;                    // rows of the tile below (all tiles of a decomposition have this tile's UNCUT height)
        bool ready = false, failed = false;  // set up (collectively) / cannot be set up (stays on RCCL)
        const void* sig[NARR] = {};          // the local arrays the set-up was made for
        int set_sig[8] = {};                 // ... and the sizes of this rank's tile sets then (the launch geometry depends on the forcing kinds too)
        int img_rank[8], sync_rank[8];       // per direction: the rank whose arrays receive this tile's images there; the neighbour to wait for (-1: none)
        void* arr[8][NARR] = {};             // that rank's arrays as this process addresses them
        unsigned long long* nbr_slots[8] = {};   // its flag array
        DeviceBuf<unsigned long long> slots; // this rank's flag array: 8 directions x SLOTS
        DeviceBuf<unsigned> err;             // device word set by a wait that timed out
        PinnedBuf<unsigned> err_host;        // pinned copy, refreshed after every sub-cycle
        unsigned long long seq = 0;          // launches of the flag protocol so far (the same number on every rank)
        std::vector<void*> opened;           // IPC mappings
        DeviceBuf<uint8_t> xbuf;             // device staging of the set-up's all-gather (bytes; only grows)
        int last = 0;                        // the last sub-cycle used the peer transport
        int tier = -1;                       // protocol tier asked for (csi_set_peer_tier; -1: automatic -- peer_effective_tier: 1 as soon as a
                                             // neighbour lives in another process or on another device, 0 for a tile connected to itself / an in-process group)
        bool aborted = false;                // a wait of the flag protocol gave up (here or at a neighbour): the transport is refused until every rank has
                                             // called csi_set_halo_transport / csi_comm_init* again (sticky: the flags cannot recover, csi_abi.hip peer_check)
        bool local_queues_ok = true;         // in-process tile group: GPU_MAX_HW_QUEUES > tiles (csi_comm_init_local)
    } peer;
    ExPlan pending_rp;                   // the receive plan of an exchange that has been begun
    // fused sub-step kernel: ping-pong copies of u, v, sigma11, sigma22, sigma12
    DeviceBuf<FusedTable> dev_tables;   // uniform-input tables of the fused kernel
    // pinned staging ring for their upload: the host never waits for the stream (a slot is reused after its own copy
    // has completed, four sub-cycles later)
    static constexpr int kRing = 4;
    PinnedBuf<FusedTable> host_ring;
    hipEvent_t ring_ev[kRing] = {nullptr, nullptr, nullptr, nullptr};
    bool ring_used[kRing] = {false, false, false, false};
    unsigned ring_pos = 0;
    // (not zeroed: run_fused / run_fused_peer copy the whole parents in before the first launch wherever a cell is not rewritten by
    //  every launch.  The neighbours of a peer-connected tile hold IPC mappings of these five: Peer::sig)
    ScratchField alt[5] = {{CSI_F_U, kRaw}, {CSI_F_V, kRaw}, {CSI_F_S11, kRaw}, {CSI_F_S22, kRaw}, {CSI_F_S12, kRaw}};
    // RK stages of an advection-only model in one launch each: (h, a) x 2 rotating copies.  (Not zeroed: a new array is filled with a
    // copy of the state -- beyond walls the halo holds mirror images the stores rewrite, cells nobody writes start as the state's)
    ScratchField adv_buf[4] = {{CSI_F_H, kRaw}, {CSI_F_A, kRaw}, {CSI_F_H, kRaw}, {CSI_F_A, kRaw}};
    // north fold (FoldBand): the band's own copies of u, v, sigma and of the four diagnostics, its stream and the two events
    // that order it against the pair launches
    // (zeroed: only the rows from M - 7 on are ever written, the band's stencils reach the cells around them -- those stay defined and
    //  the same from run to run; used on band_stream as well as on the context's stream: ensure_band)
    ScratchField band[9] = {{CSI_F_U, kZeroed}, {CSI_F_V, kZeroed}, {CSI_F_S11, kZeroed}, {CSI_F_S22, kZeroed}, {CSI_F_S12, kZeroed},
                            {CSI_F_ALPHA, kZeroed}, {CSI_F_ZETA_C, kZeroed}, {CSI_F_ZETA_F, kZeroed}, {CSI_F_DELTA, kZeroed}};
    hipStream_t band_stream = nullptr;
    hipEvent_t band_ev_pair = nullptr, band_ev_band = nullptr;
    // Forcing scratch, filled once per sub-cycle at every point whose stencil stays inside the parents.  Zeroed: those launches never
    // write the outermost layer of the parent, which the four-point averages of the kernels that read these arrays reach.
    ScratchField fbar[2] = {{CSI_F_V, kZeroed}, {CSI_F_U, kZeroed}};       // ocean ubar at v points, vbar at u points (array-valued bottom drag)
    ScratchField fbar_top[2] = {{CSI_F_V, kZeroed}, {CSI_F_U, kZeroed}};   // the same of the air velocities (array-valued wind drag)
    ScratchField fd[2] = {{CSI_F_U, kZeroed}, {CSI_F_V, kZeroed}};         // free-drift velocities at u / v points (StressBalanceFreeDrift)
    ScratchField xd[2] = {{CSI_F_U, kZeroed}, {CSI_F_V, kZeroed}};         // stress divergence of the immersed flux boundary conditions at u / v points (two-sub-steps kernel)
    int free_drift = 0;                     // csi_free_drift_set: csi_free_drift_kind.  Non-zero: the kernels read P.ufd / P.vfd; 1: the library
                                            // computes them from the stresses first (fd[]); 2: they ARE the arrays bound to CSI_F_FREE_DRIFT_U / _V
    int dynamics = CSI_DYNAMICS_MOMENTUM_EQUATION;   // csi_dynamics_set: CSI_DYNAMICS_FREE_DRIFT = StressBalanceFreeDrift as the whole dynamics
    bool slab_set = false;   // thermodynamic step inside csi_time_step_fe / _rk3
    SlabDev slab{};
    int vel_bc_on[2][2] = {{0, 0}, {0, 0}};          // csi_velocity_bc_set: [u | v][low | high] ValueBoundaryCondition
    double vel_bc_value[2][2] = {{0, 0}, {0, 0}};
    bool snow_set = false;   // layered (snow + ice) step instead of the bare-ice one
    SnowDev snow{};
    // csi_mixed_layer_set (csi_thermo.hip, mixed_layer.hip): the slab-ocean mixed layer, stepped before the thermodynamic step of every stage
    bool ml_set = false;
    csi_mixed_layer_params ml{};
    int64_t ml_launches = 0;             // csi_mixed_layer_stats
    // csi_shortwave_set: the SHORTWAVE top term's setting (sw.mode == SW_NONE: none); heat_has_shortwave: the top's tuple has the term
    ShortwaveDev sw{};
    bool heat_has_shortwave = false;
    HeatFluxDev heat{};      // csi_heat_fluxes_set / csi_surface_solve_set (thermo_flux.hip); heat.top.n = heat.bot.n = 0: numbers only
    // csi_time_series_set / _update (csi_time_series.hip): at most one series per eligible slot; the copy stream of the HOST backend's
    // uploads and the event recorded behind every interpolation launch (an upload into a ring slot waits for it), both made once
    std::vector<TimeSeries> series;
    hipStream_t series_stream = nullptr;
    hipEvent_t series_launched = nullptr;
    bool series_launched_valid = false;
    bool series_prefetch_pending = false;    // the newest update's look-ahead uploads have not been issued yet
    long series_updates = 0;
    // csi_regrid_map_create / csi_time_series_set_regridded: the maps (a map's id is its index) and the regridded slots, at most one
    // series of either kind per slot; they share the copy stream, the event and the look-ahead with the series above
    std::vector<RegridMap> maps;
    std::vector<RegridSeries> regrid;
    int64_t regrid_launches = 0;         // csi_regrid_stats
    // the ordered reductions (csi_diagnostics_compute, csi_budget_compute, csi_momentum_budget_compute; reduce_begin in
    // csi_diagnostics.hip): ONE device buffer -- the partial records followed by the result slots, sized by the grid alone for the
    // largest slot count, so alternating calls never reallocate -- and ONE page-locked copy of the result; every such call ends in a
    // wait, so they never overlap.  gather_buf: the device staging of an all-gather over an RCCL communicator (only grows)
    DeviceBuf<double> reduce_part;
    PinnedBuf<double> reduce_host;
    DeviceBuf<uint8_t> gather_buf;
    // the calls made so far (csi_derived_stats, csi_momentum_terms_stats)
    int64_t derived_launches = 0, budget_calls = 0;
    int64_t drifter_launches = 0;        // csi_drifters_advance / _sample (csi_drifters.hip): launches of the two kernels
    // csi_regions_compute (csi_regions.hip): the partial records followed by the folded slots (sized by csi_regions_layout, only
    // grows), ONE page-locked copy of the folded slots, the launches made so far (csi_regions_stats).  Empty until the first call
    DeviceBuf<double> regions_part;
    PinnedBuf<double> regions_host;
    int64_t region_launches = 0;
    // csi_tracers_set (csi_tracers.hip): the caller's description, the parent of h it was checked against, the dense c* of a stage and
    // the Psi^- copies c^- (n parents), both allocated by csi_tracers_set; the launches so far and the last stencil launch's layout
    struct Tracers {
        bool set = false;
        csi_tracers t{};
        Bound shape;
        long grid_gen = 0;
        DeviceBuf<double> star, base;
        DeviceBuf<double> free_;             // RK3: the stage before, without its source (n parents; empty while no tracer has a source)
        bool free_valid = false;             // ... has been written since csi_cache_current_fields (the second stage on)
        bool star_from_cache = false;        // the pending first half was an RK3 stage's
        int64_t star_ld = 0, star_plane = 0;
        bool star_valid = false;             // a first half has run since the last second half
        bool base_valid = false;             // csi_cache_current_fields has copied c -> c^- since csi_tracers_set
        int64_t stencil_launches = 0, update_launches = 0;
        TracerLayout last{0, 0, 0, 0};
    } trc;
    int64_t mterm_launches = 0, mterm_budget_calls = 0;
    // csi_output_* (csi_output.hip): the sets and the copy stream their records leave on, made at the first csi_output_create
    OutputSet out_sets[kMaxOutputSets];
    hipStream_t out_stream = nullptr;
    // csi_enthalpy_create (csi_enthalpy.hip): the column models made from this context that have not been destroyed yet
    std::vector<csi_enthalpy*> enthalpies;
    long grid_gen = 0;                   // csi_grid_set calls so far
    int weno_w32 = 0;     // csi_set_weno_weight_dtype: 1 = WENO weights in single precision (upstream's FT2 = Float32, recalled)
    // csi_rheology_set / csi_momentum_solver_set (csi_momentum.hip): ViscousRheology, ExplicitSolver
    int rheology = CSI_RHEOLOGY_EVP;
    double nu = 1000.0;
    int solver = CSI_SOLVER_SPLIT_EXPLICIT;
    // the viscous sub-cycle's second u / v arrays (ping-pong with the bound ones).  Not zeroed: viscous_subcycle copies the parents in
    // unless every cell is rewritten by every launch
    ScratchField vis_alt[2] = {{CSI_F_U, kRaw}, {CSI_F_V, kRaw}};
    int fusion = 1;       // 1: use the fused sub-step kernel when the configuration allows it
    int pairing = 1;      // 1: two sub-steps per launch where supported (csi_set_fusion level 2)
    AdvLayout last_adv{0, 0, 0};     // csi_last_advection: what the last tendency / stage launch of k_tendencies used (0: none yet)
    int last_adv_stage = 0;          // ... and whether it was a whole RK stage in one launch
    ThermoLaunch last_thermo{0, 0, -1};      // csi_last_thermo: what the last thermodynamic launch used, as its launcher returned it (step 0: none yet)
    double ibc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};   // csi_immersed_flux_bc_set: [u | v][west, east, south, north]
    int exch_k = 0;       // sub-steps per halo exchange (0 = auto: the largest k with 2k <= halo, at most 4)
    // Tile activity (csi_activity.hip, run_fused): the live-tile list of the current sub-cycle and, read back asynchronously, how many
    // tiles were live in earlier ones -- the launch geometry of the NEXT sub-cycles is refined so that the live tiles fill one round
    // (correctness never depends on that estimate: the list is made afresh, on the device, before every sub-cycle's first launch)
    struct Activity {
        static constexpr int kSamples = 4;
        int enabled = 1;                     // csi_set_tile_skipping
        DeviceBuf<int> flags;                // device: one int per tile
        DeviceBuf<int> list;                 // device: {live, tiles, the live tiles' numbers}
        DeviceBuf<int> list0;                // device: the same for the first two launches (all but the tiles quiescent from the start)
        PinnedBuf<int> host;                 // pinned, device-visible: {seqlock, live, tiles, sample id} written by k_activity_compact
        int* host_dev = nullptr;             // ... as the device addresses it (not owned)
        double sample_scale[kSamples] = {1, 1, 1, 1};      // the geometry scale of sample id % kSamples
        unsigned seq = 0;                    // sample ids handed out
        int seen_id = -1;                    // the newest sample the host has taken
        double scale = 1.0;                  // tiles of a live launch relative to the one-round geometry (pair_geom's tile_scale)
        int last_live = -1, last_tiles = 0;  // the newest sample that has arrived
        int last_used = 0;                   // the last sub-cycle ran live launches
        int since_probe = 0;                 // sub-cycles since the last test while nothing is quiescent (run_fused: probed every 32nd)
    } act;
    // CSI_METRIC_FULL: rows whose twelve coefficient planes (and per-point Coriolis planes) hold one value per row (ensure_row_constant)
    std::vector<double> coef2_host, fcor2_host;      // host copies of the planes the marks are made from
    DeviceBuf<double> dev_c2row;         // (C2_COUNT + 2) vectors of nj doubles
    DeviceBuf<int> dev_rcsum;            // nj + 1 prefix sums
    bool rc_dirty = true;
    int rc_enabled = 1;                  // csi_set_row_constant(ctx, on, rtol)
    double rc_rtol = 0.0;                // 0: bitwise-equal columns only (results unchanged); > 0: columns within this relative distance of column 1 count as equal -- CHANGES results at that level
    int rc_rows = 0;                     // rows marked
    int geom_band = 0;    // the pair launches being laid out run beside a fold band (FoldCut / PeerView of a fold tile): see pair_geom
    int geom_peer = 0;    // ... are launches of the peer transport (PeerView): shorter chunks next to the connected y sides (bit 0; bits 1 / 2: both x / y sides connected)
    // tuning aids (A/B runs), read from the environment ONCE, when the context is created; -1 = not set
    struct Tuning { int fused_rows = -1, pair_tiles = -1, pair_target = -1, row_target_1024 = 0, pair_minrows = -1, pair_rows = -1, pair_common = -1, peer_kernel = -1, peer_edge = -1, write_through = -1,
                    adv_nt = -1,           // CSI_ADV_NT: tracers per thread of the advection tendency kernel (1 / 2; default by grid size)
                    adv_shape = -1,        // CSI_ADV_SHAPE: block shape where two tracers share a thread (1 / 2 / 3: 64 x 8 / 63 x 7 / 63 x 11; default by grid size)
                    band_fused = -1,      // CSI_BAND_FUSED=0: the fold band on the three kernels + two copies per step (rounds 4-6a); default: six launches per step without copies, loads hoisted (csi_fold.hip band_substeps_fused)
                    band_event_flags = -1,   // CSI_BAND_EVENT_FLAGS (csi_fold.hip ensure_band)
                    enth_path = 0,         // CSI_ENTH_PATH: the form of the enthalpy-method column model's step kernel (0 by the rule, 1 per step, 2 on chip)
                    trc_ntr = -1,          // CSI_TRACERS_NTR: tracers per thread of the tracer stencil kernel (1 / 2 / 4; default by the number of tracers)
                    no_geom_sig = -1;      // debugging aid (CSI_DEBUG_NO_GEOM_SIG=1): skip the launch-geometry check of the peer set-up (tests/test_gpu_local_tiles.py)
      long adv_stage_max_cells = 1L << 40;      // advection-only models: one launch per RK stage up to this many cells (advect_stage_supported; no cut since round 6)
    } tune;
};

namespace csi_host {

#define HIP_TRY(c, expr)                                                                        \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(c, CSI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

#define NCCL_TRY(c, expr)                                                                       \
    do {                                                                                        \
        ncclResult_t r_ = (expr);                                                               \
        if (r_ != ncclSuccess)                                                                  \
            return fail(c, CSI_ERR_COMM, std::string(#expr) + ": " + ncclGetErrorString(r_));   \
    } while (0)

// Element (0, 0) in reference indexing of a parent array with row stride ld -- (i, j) is then p[i + j * ld]: bound fields (ref_of),
// library arrays that shadow them (ScratchField::view), the mask and the per-point metric / coefficient / Coriolis planes
template <class T>
static inline T* origin_of(const csi_context* c, T* parent, int64_t ld) { return parent + (c->Hx - 1) + (int64_t)(c->Hy - 1) * ld; }
inline hipError_t ScratchField::ensure(const csi_context* c, hipStream_t also, bool* fresh) {
    const Bound& b = c->f[fid];
    return buf.ensure((size_t)b.ld * (size_t)b.nj, c->stream, zeroed, also, fresh);
}
inline FRef ScratchField::view(const csi_context* c) const { return FRef{origin_of(c, buf.get(), c->f[fid].ld), (int)c->f[fid].ld}; }

static inline int nxf_of(int k) { return k > 1 ? 5 : 2; }     // sigma travels with u, v when k > 1 (see do_subcycle)

struct FoldBand;
// ---- functions shared by the translation units (definitions: see the list at the top) ----
static const int kPing[5] = {CSI_F_U, CSI_F_V, CSI_F_S11, CSI_F_S22, CSI_F_S12};
// (elo / ehi: rows of the FIRST / LAST chunk where they differ from `rows` -- shorter tiles next to a peer-connected y side,
//  pair_geom; elo == rows and ehi == 0: every chunk `rows` rows, the last one what is left)
struct FusedGeom { Range rs; int nstrips, nchunks, rows; int elo = 0, ehi = 0; int wt = 0; };      // wt: write-through result stores (FI_WT)
// rows [ja, jb] of chunk q (the kernels' formula: evp_fused2.hip)
static inline void chunk_rows(const FusedGeom& G, int q, int* ja, int* jb) {
    const int elo = G.elo > 0 ? G.elo : G.rows;
    const bool last_short = G.ehi > 0 && q == G.nchunks - 1 && q > 0;
    *ja = last_short ? G.rs.j1 - G.ehi + 1 : G.rs.j0 + (q == 0 ? 0 : elo + (q - 1) * G.rows);
    *jb = q == 0 ? std::min(*ja + elo - 1, G.rs.j1) : (q == G.nchunks - 1 ? G.rs.j1 : std::min(*ja + G.rows - 1, G.rs.j1 - G.ehi));
}
constexpr int kMaxExchangeInterval = 16;
struct SideV { int xlo, xhi, ylo, yhi; };
static const int kPeerDx[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, kPeerDy[8] = {0, 0, -1, 1, -1, -1, 1, 1};
static const int kPeerOpp[8] = {1, 0, 3, 2, 7, 6, 5, 4};
struct PeerSets { int nW, nE, nS, nN, size[8], n[8]; };
struct PeerRec {                 // what a rank tells the others about one of its buffers
    hipIpcMemHandle_t handle;    // of the allocation that holds it
    uint64_t offset;             // of the buffer inside that allocation
    int64_t ld;                  // leading dimension (images use the sender's strides: they must agree)
    int32_t ok, pad;
    uint64_t local_ptr;          // in-process tile group: the buffer itself (same address space)
    int32_t set_size[8];         // (record 0) tiles of this rank's launches in each direction's set: what the neighbour waits for
};
constexpr int kPeerRecs = csi_context::Peer::NARR + 1;      // + the flag array
// The grid descriptor the launches of the peer transport see: connected sides count as periodic ones; a fold tile is cut below
// its three-kernel band (FoldBand), whose side then counts as "connected" (halo rows = interior rows of the same arrays).
struct PeerView {
    csi_context* c; GridDev g; int Ny;
    explicit PeerView(csi_context* cc) : c(cc), g(cc->g), Ny(cc->Ny), peer_was(cc->geom_peer) {
        c->geom_peer = 1 | (c->g.xlo == SIDE_CONNECTED && c->g.xhi == SIDE_CONNECTED ? 2 : 0) | (c->g.ylo == SIDE_CONNECTED && c->g.yhi == SIDE_CONNECTED ? 4 : 0);
        for (int* side : {&c->g.xlo, &c->g.xhi, &c->g.ylo, &c->g.yhi}) if (*side == SIDE_CONNECTED) *side = SIDE_PERIODIC;
        if (c->g.yhi == SIDE_FOLD) { const int M = c->Ny - c->Hy - 4; c->Ny = M; c->g.Ny = M; c->g.yhi = SIDE_CONNECTED; band = c->geom_band; c->geom_band = 1; }
    }
    int band = -1, peer_was = 0;
    ~PeerView() { c->g = g; c->Ny = Ny; if (band >= 0) c->geom_band = band; c->geom_peer = peer_was; }
};
// The ranges of one three-kernel sub-step at one valid halo width V: stress on rs; then u on ru1 and v on r2 (u first), or v on rv1
// and u on r2
struct SubstepRanges {
    Range rs, ru1, rv1, r2;
    // rows >= jlo of the stress, >= jlo + 1 of the velocities (the fold band)
    SubstepRanges from_row(int jlo) const {
        SubstepRanges R = *this;
        R.rs.j0 = std::max(R.rs.j0, jlo);
        for (Range* r : {&R.ru1, &R.rv1, &R.r2}) r->j0 = std::max(r->j0, jlo + 1);
        return R;
    }
};
struct FoldBand {
    int M;
    bool tiled;                     // the fold tile of a y partition: its south side is connected
    int k;                          // exchange interval (tiled; 2 otherwise: one pair launch per band step)
    GridDev g_full, g_cut;          // the tile as it is / with the band cut off and the north side "connected"
    int Ny_full;
    EvpDev P;                       // the whole grid (fold geometry)
    ImageSpec imu, imv;
    SubstepRanges R;                // the three kernels' ranges on the whole grid
};
struct FoldCut {        // RAII: the tile with the band cut off (rows 1 .. M, north side "connected")
    csi_context* c; GridDev g; int Ny, band;
    FoldCut(csi_context* cc, int M) : c(cc), g(cc->g), Ny(cc->Ny), band(cc->geom_band) { c->Ny = M; c->g.Ny = M; c->g.yhi = SIDE_CONNECTED; c->geom_band = 1; }
    ~FoldCut() { c->g = g; c->Ny = Ny; c->geom_band = band; }
};

int32_t fail(csi_context* c, int32_t code, const std::string& msg);
int side_lo(int topo);
int side_hi(int topo);
int img_of(int side, int loc);
ImageSpec image_spec(const csi_context* c, int fid);
int32_t fill_width_check(csi_context* c, int fid);      // CSI_ERR_UNSUPPORTED where a local fill of this field would need more than one image per side
FRef ref_of(const csi_context* c, int fid);
// a local halo fill of bound slots in one batch
static inline void halo_add(const csi_context* c, HaloBatch& B, int fid) { B.f[B.n] = ref_of(c, fid); B.im[B.n] = image_spec(c, fid); ++B.n; }
static inline HaloBatch halo_batch(const csi_context* c, std::initializer_list<int> fids) { HaloBatch B{}; for (int fid : fids) halo_add(c, B, fid); return B; }
void set_sides(GridDev& g, int topo_x, int topo_y);      // the four sides of a grid descriptor from the two topologies
int32_t need(csi_context* c, std::initializer_list<int> ids);
// every id bound, or CSI_ERR_NOT_BOUND "<who>: <group>needs field <name> (not bound<hint>)" (group: empty, or with its trailing blank)
int32_t need_named(csi_context* c, const char* who, const char* group, std::initializer_list<int> ids, const char* hint);
// the host side of an ordered reduction (ordered_reduce.h), csi_diagnostics.hip.  reduce_begin: sizes the context's reduction buffers
// and hands out the partial records, their count and the place of the result; the caller queues its partial and finishing kernel on
// the context's stream; reduce_end: copies the n result slots to page-locked memory, waits ONCE and copies them to slots[n].
// reduce_ranks: on a tiled context the all-gather of every rank's (status, slots) and the
// combine of slots q0 .. q1 - 1 in rank order (combine == nullptr: every slot a sum); rc: this rank's status so far -- a rank that
// has failed locally (a missing field, a HIP error) still enters the collective, with a status word that makes every other rank
// return CSI_ERR_COMM "<who>: rank r ... failed locally": an early return would strand the others inside it (as in csi_peer.hip
// peer_setup).  Returns rc, with its message, if set.
int32_t reduce_begin(csi_context* c, double** part, long* nrec, double** result);
int32_t reduce_end(csi_context* c, int n, const double* result, double* slots);
int32_t reduce_ranks(csi_context* c, const char* who, int32_t rc, int n, int q0, int q1, double (*combine)(int q, double a, double b), double* slots);
StressDev stress_dev(const csi_context* c, int side);
int32_t check_stress_fields(csi_context* c, int side);
int32_t sync_coriolis(csi_context* c);
EvpDev evp_dev(const csi_context* c, double dt);
Range stress_range(const csi_context* c, int V = 2);
Range first_u_range(const csi_context* c, int V = 2);
Range first_v_range(const csi_context* c, int V = 2);
Range second_range(const csi_context* c, int V = 2);
SubstepRanges substep_ranges(const csi_context* c, int V = 2);
// ONE sub-step on the three kernels (split_explicit_momentum_equations.jl:178-187).  fc == nullptr: STRICT (viscosities, stress, the
// strict velocity steps: four launches)
void launch_substep(const EvpDev& P, const FastCoef* fc, const SubstepRanges& R, const ImageSpec& imu, const ImageSpec& imv, bool ufirst, hipStream_t st);
int32_t copy_ping(csi_context* c, bool to_alt);      // the five whole parents of kPing: bound arrays -> c->alt (to_alt) or back
// A batch of whole-array copies built entry by entry.  copy_batch_aligned() starts one whose aligned16 stays 1 while every pointer added
// is 16-byte aligned; a batch started as CopyBatch{} keeps aligned16 == 0 whatever is added (the fold band's, csi_fold.hip)
static inline CopyBatch copy_batch_aligned() { CopyBatch B{}; B.aligned16 = 1; return B; }
static inline void copy_add(CopyBatch& B, const double* src, double* dst, long n) {
    B.src[B.count] = src; B.dst[B.count] = dst; B.n[B.count] = n; ++B.count;
    if ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) B.aligned16 = 0;
}
// the halo a scheme's stencil needs (0: no such scheme), and the check of a scheme against the grid's halo
static inline int advect_halo(int scheme) {
    switch (scheme) {
        case CSI_ADVECT_UPWIND1: return 1;
        case CSI_ADVECT_WENO3: case CSI_ADVECT_UPWIND3: return 2;
        case CSI_ADVECT_WENO5: case CSI_ADVECT_UPWIND5: return 3;
        case CSI_ADVECT_WENO7: return 4;
        default: return 0;
    }
}
static inline bool advect_fits(const csi_context* c, int scheme) { const int h = advect_halo(scheme); return h > 0 && c->Hx >= h && c->Hy >= h; }
int32_t advect_scheme_check(csi_context* c, int scheme);
bool is_tiled(const csi_context* c);
int32_t exchange(csi_context* c, const int* fids, int nf, int W);
int32_t local_allgather(csi_context* c, const void* mine, size_t nb, std::vector<uint8_t>& out);
int32_t local_allreduce_min(csi_context* c, int* v);
// rank r's `nb` bytes end up in out[r * nb ...] on every rank, over whatever joins the ranks; no communicator: out = mine
int32_t comm_allgather(csi_context* c, const void* mine, size_t nb, std::vector<uint8_t>& out);
int32_t comm_allreduce_max(csi_context* c, int* v);      // over whatever joins the ranks (RCCL communicator, in-process group, host-channel group)
int peer_effective_tier(const csi_context* c);
int32_t local_wait_consumed(csi_context* c);
int32_t local_sendrecv(csi_context* c, const long* soff, const long* scnt, const int* speer, const long* roff, const long* rcnt, const int* rpeer);
int32_t exchange_refs(csi_context* c, const FRef* fr, int nf, int W);
int32_t fill_halo(csi_context* c, int fid);
int32_t copy_parent(csi_context* c, int dst, int src);
int32_t do_initialize(csi_context* c);
static inline FRef alt_ref(const csi_context* c, int k) { return c->alt[k].view(c); }
FusedGeom fused_geom(const csi_context* c, int V);
void velocity_ranges(const csi_context* c, bool ufirst, int V, Range& r1, Range& r1c, Range& r2);
int32_t ensure_alt(csi_context* c);
int exchange_interval(const csi_context* c);
SideV pair_side_v(const csi_context* c, int v_connected, int v_periodic);
Range v_first_range(const csi_context* c, const SideV& v, bool ufirst);
Range clip_store(const csi_context* c, Range r, bool sigma);
bool has_walls(const csi_context* c);
bool offsets_fit_32bit(int Nx, int Ny, int Hx, int Hy, int64_t max_ld);
int64_t max_bound_ld(const csi_context* c);
bool pair_supported(const csi_context* c);
FusedGeom pair_geom(const csi_context* c, const Range& dec, double tile_scale = 1.0);
int32_t ensure_row_constant(csi_context* c);
bool activity_sample(csi_context* c);
PeerSets peer_wait_counts(const csi_context* c, const FusedGeom& G);
void peer_local_arrays(const csi_context* c, const void* out[csi_context::Peer::NARR]);
void peer_release(csi_context* c);
bool fold_cut_possible(const csi_context* c);
bool peer_tile_supported(csi_context* c, const EvpDev& Pfull);
PeerSets peer_my_sets(csi_context* c);
int32_t peer_setup(csi_context* c, bool local_ok);
int32_t peer_decide(csi_context* c, const EvpDev& P, int substeps, bool* use);
int32_t peer_fill_table(csi_context* c, const FusedGeom& G, bool out_is_alt, FusedTable* t);
static inline FRef band_ref(const csi_context* c, int q) { return c->band[q].view(c); }
int32_t ensure_band(csi_context* c);
int32_t band_substep(csi_context* c, const FoldBand& bd, const FastCoef& fc, const FRef* b, const FRef* d, bool ufirst, int jlo, bool last, hipStream_t st);
int32_t band_substeps(csi_context* c, const FoldBand& bd, const FastCoef& fc, int cur, int s, int n, bool last);
int band_launches(const csi_context* c, int n);
int32_t run_fused(csi_context* c, const EvpDev& P, const FastCoef& fc, int substeps, int first, bool peer = false, const FoldBand* band = nullptr);
int32_t run_fused_peer(csi_context* c, double dt, const FastCoef& fc, int substeps, int first);
bool fold_band_supported(csi_context* c, const EvpDev& Pfull, int substeps);
int32_t run_fused_fold(csi_context* c, const EvpDev& Pfull, const FastCoef& fc, int substeps, int first);
FoldBand fold_band(const csi_context* c, const EvpDev& Pfull, bool tiled, int k);      // everything but g_cut, of the tile as it is
int32_t do_subcycle(csi_context* c, double dt, int substeps, int first);
int32_t do_finalize(csi_context* c);
int32_t need_evp(csi_context* c);
int32_t need_dynamics_common(csi_context* c);
int32_t do_time_step_momentum(csi_context* c, double dt, int substeps, int rk_reset);
FastCoef fast_coef(const csi_context* c, const EvpDev& P, double dt);
// csi_momentum.hip: the rheology / solver dispatch (EVP + split-explicit: need_evp / do_time_step_momentum, unchanged)
int32_t momentum_config_check(csi_context* c);
int32_t need_momentum(csi_context* c);
int32_t do_momentum(csi_context* c, double dt, int substeps, int rk_reset);
int32_t do_momentum_tendencies(csi_context* c, double dt);
int32_t free_drift_fields(csi_context* c, double dt);      // (shared with the EVP sub-cycle and time_step_momentum!, csi_launch.hip)
int32_t reset_velocities(csi_context* c);
int32_t fill_forcing_halos(csi_context* c);
int32_t update_external_stress(csi_context* c);          // fill_forcing_halos + their exchange between tiles
static inline bool has_dynamics(const csi_context* c) { return c->evp_set || c->dynamics == CSI_DYNAMICS_FREE_DRIFT; }
AdvDev adv_dev(const csi_context* c, int scheme, double dt, int from_cache);
int32_t do_update_state(csi_context* c, bool in_step = false, bool tracers_filled = false);
int32_t do_tendencies(csi_context* c, int scheme);
int32_t do_tendencies_or_zero(csi_context* c, int scheme);
int32_t do_tracer_step(csi_context* c, double dt, int from_cache, bool fill_images = false);
// csi_step.hip
int32_t step_checks(csi_context* c, bool dynamics, bool rk3);
int32_t step_stage(csi_context* c, double dt, int substeps, int scheme, bool dynamics, int from_cache);
bool advect_stage_supported(const csi_context* c, int scheme);
int32_t rk3_advection_only(csi_context* c, double dt, int scheme);
int32_t cache_current_fields(csi_context* c);
int32_t do_thermo(csi_context* c, double dt, int from_cache = 0);      // csi_thermo.hip: thermodynamic_time_step! of a stage (the mixed layer first, from Psi^- if from_cache)
int extra_x(const csi_context* c, int fid);
int extra_y(const csi_context* c, int fid);
Range interior_range(const csi_context* c);
Range parent_range(const csi_context* c);
bool has_comm(const csi_context* c);
Range v_stress_range(const csi_context* c, const SideV& v);
Range v_second_range(const csi_context* c, const SideV& v);
static inline const Bound& band_bound(const csi_context* c, int q) { return c->f[c->band[q].fid]; }
int32_t series_prefetch(csi_context* c);                 // ... the look-ahead uploads of the newest csi_time_series_update, once (no-op otherwise)
void series_release(csi_context* c);                     // csi_time_series.hip: events, copy stream, rings (the streams have been drained)
bool series_drives(const csi_context* c, int fid);       // ... a series of either kind (model grid, regridded) is set on the slot
void enthalpy_release(csi_context* c);                   // csi_enthalpy.hip: every surviving column model (the context's stream has been drained)
void output_release(csi_context* c);                     // csi_output.hip: every set, the copy stream (the context's stream has been drained)
// csi_tracers.hip: the halves of a stage (include/csi.h), the Psi^- copies, update_state!'s mask and halo fill outside a step, and
// CSI_TRACER_FIELD(k) as an output field
int32_t tracers_first_half(csi_context* c, int scheme, double dt, int from_cache);
int32_t tracers_second_half(csi_context* c, double dt);
int32_t tracers_cache(csi_context* c);
int32_t tracers_update_state(csi_context* c);
bool tracer_field_id(int32_t id, int* k);
Bound tracer_bound(const csi_context* c, int k);
int32_t peer_check_entry(csi_context* c);      // (csi_abi.hip: the error word of the peer transport, checked at every entry point)

}  // namespace csi_host

