// csi_launch.hip -- launch loops: the EVP sub-cycle on every path, finalize_rheology!, time_step_momentum!, tracer steps, update_state!,
// csi_profile_substeps.  The three-kernel sub-step, its ranges, the ping copies and the batch builders they call are stated once in
// csi_core.hip / csi_ctx.h; whole steps are sequenced in csi_step.hip.  (Split out of csi_abi.hip in round 4; see csi_ctx.h)
#include "csi_ctx.h"

namespace csi_host {

// csi_subcycle_stats_*: an extra event behind ev0 / ev1 of every sub-step loop while the statistics are on
static int32_t stats_mark(csi_context* c) {
    if (!c->stats.on || c->stats.ev.size() >= 2 * 4096) return CSI_OK;
    hipEvent_t e;
    HIP_TRY(c, hipEventCreate(&e));
    HIP_TRY(c, hipEventRecord(e, c->stream));
    c->stats.ev.push_back(e);
    return CSI_OK;
}
static void stats_launches(csi_context* c, int n) { if (c->stats.on && c->stats.launches.size() * 2 < c->stats.ev.size()) c->stats.launches.push_back(n); }

// The newest activity sample the device has written into the pinned words (k_activity_compact's seqlock): true when a new one was taken.
bool activity_sample(csi_context* c) {
    csi_context::Activity& a = c->act;
    if (!a.host) return false;
    volatile int* w = a.host.get();
    const int s1 = w[0];
    if (s1 & 1) return false;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const int live = w[1], tiles = w[2], id = w[3];
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (w[0] != s1 || s1 == 0 || id == a.seen_id) return false;
    a.seen_id = id; a.last_live = live; a.last_tiles = tiles;
    return true;
}

// The per-call members of the FAST kernels' coefficient block (everything else in it belongs to the grid: c->coef)
FastCoef fast_coef(const csi_context* c, const EvpDev& P, double dt) {
    FastCoef fc = c->coef;
    const double ie = 1.0 / P.ecc;
    fc.em2 = ie * ie;
    fc.ca_dt = 0.5 * (P.ca * dt); fc.hkc = fc.ca_dt * fc.uni[FC_RAZC]; fc.hkf = fc.ca_dt * fc.uni[FC_RAZF]; fc.hk1 = 0.5 * (1.0 - ie * ie);
    fc.rdt = 1.0 / dt;
    fc.Dmin2 = P.Dmin * P.Dmin; fc.rDmin = 1.0 / P.Dmin;
    fc.amin2 = P.amin * P.amin; fc.amax2 = P.amax * P.amax; fc.ramin = 1.0 / P.amin; fc.ramax = 1.0 / P.amax;
    return fc;
}

// ==== run_fused: one sub-cycle on the fused kernels, in four stages =========================================================
// tables: singles (position in the exchange batch) x (which buffer is current) x (u first / v first), then
// pairs (pair position) x (buffer) x (first sub-step u first / v first)
constexpr int KMAX = kMaxExchangeInterval, NSINGLE = KMAX * 4, NPAIR = (KMAX / 2) * 4;

// ---- stage 1, forcing scratch: what the array-forcing instantiations of the pair kernel read besides the bound arrays, computed
// once per sub-cycle into library arrays
struct ForcingScratch {
    bool force = false;         // array-valued forcing: two-sub-steps kernel only
    bool wind = false;          // ... with array-valued air velocities
    bool extra = false;         // model.forcing arrays / immersed flux boundary conditions (the EXTRA instantiations)
    int extra_kind = 0;         // which family of array-forcing instantiations
    int common_forcing = 0;     // the kernels' compile-time forcing kinds (below)
    FRef ubar_v{nullptr, 0}, vbar_u{nullptr, 0};      // ocean velocities' cross averages (bottom drag)
    FRef tbar_v{nullptr, 0}, tbar_u{nullptr, 0};      // the air velocities' (wind drag)
    FRef xd_u{nullptr, 0}, xd_v{nullptr, 0};          // divergence of the immersed fluxes
};
static int32_t scratch_views(csi_context* c, ScratchField (&s)[2], FRef* a, FRef* b) {
    for (ScratchField& f : s) HIP_TRY(c, f.ensure(c));
    *a = s[0].view(c); *b = s[1].view(c);
    return CSI_OK;
}
static int32_t forcing_scratch(csi_context* c, const EvpDev& P, ForcingScratch* out) {
    ForcingScratch F;
    int32_t rc;
    F.force = pair_forcing_kind(P) == 1;
    // number-valued top stress (or none) and a bottom SemiImplicitStress with number-valued ocean velocities: the kernels'
    // compile-time forcing kinds
    auto ocean_at_rest = [](int kind, double value) { return kind == 0 || (kind == 1 && value == 0.0 && !std::signbit(value)); };   // (-0.0 would flip signed zeros)
    F.common_forcing = !F.force && P.top.kind <= 1 && P.bot.kind == 3 && P.bot.ue_kind != 2 && P.bot.ve_kind != 2 &&
                       P.pressure_kind == 0;            // ... and the default ReplacementPressure
    if (F.common_forcing && ocean_at_rest(P.bot.ue_kind, P.bot.ue) && ocean_at_rest(P.bot.ve_kind, P.bot.ve))
        F.common_forcing = 2;                           // ZeroField ocean velocities (the reference's default)
    if (c->tune.pair_common >= 0 && F.common_forcing > c->tune.pair_common) F.common_forcing = c->tune.pair_common;   // A/B knob (CSI_PAIR_COMMON)
    if (F.force && P.bot.kind == 3 && (P.bot.ue_kind == 2 || P.bot.ve_kind == 2)) {
        // cross components of the ocean velocity averaged to the velocity points (ubar lives at v points, vbar at u points)
        if ((rc = scratch_views(c, c->fbar, &F.ubar_v, &F.vbar_u))) return rc;
        launch_forcing_bars(P, F.ubar_v, F.vbar_u, c->stream);
    }
    F.wind = F.force && P.top.kind == 3 && (P.top.ue_kind == 2 || P.top.ve_kind == 2);
    F.extra_kind = P.extra ? 1 : ((F.wind || (F.force && P.bot.kind == 2)) ? 2 : 0);
    if (F.wind) {
        if ((rc = scratch_views(c, c->fbar_top, &F.tbar_v, &F.tbar_u))) return rc;
        launch_forcing_bars(P, F.tbar_v, F.tbar_u, c->stream, true);
    }
    // the divergence of the immersed fluxes is a function of the mask and the metrics only
    F.extra = P.extra != 0;
    bool any_ibc = false;
    for (int q = 0; q < 4; ++q) any_ibc |= (P.ibc_u[q] != 0.0) | (P.ibc_v[q] != 0.0);
    if (F.extra && P.g.has_mask && any_ibc) {
        if ((rc = scratch_views(c, c->xd, &F.xd_u, &F.xd_v))) return rc;
        launch_immersed_div(P, F.xd_u, F.xd_v, c->stream);
    }
    *out = F;
    return CSI_OK;
}

// ---- stage 2, activity plan (csi_activity.hip): untiled grids (a fold band beside them or not) advanced by pair launches.  The first
// two pair launches and the last launch of the sub-cycle run every tile on the one-round geometry; the launches in between run the LIVE
// tiles of a finer geometry GA -- so many more tiles as the newest sample of the live fraction says fit one round.
// (peer-connected tiles: the tiles of the direction sets always run -- they publish their flags whatever they hold --, the interior
//  ones may go quiet; the launch geometry stays the one the transport was set up for)
// The plan is made ONCE, after GA has been checked: the table entries, the copy before the first launch, the test launch and the
// launch loop's write_diag bits all read this one value, so no launch can ask for a list that was not built.
struct ActivityPlan {
    bool on = false;       // the test runs and the launches in between read its list of live tiles
    bool q0 = false;       // ... and the first two launches leave out the tiles quiescent from the start (only with `on`)
    FusedGeom GA{};        // the geometry of those launches
};
// candidate: the configuration takes the cut at all; dec / GP0: the first pair position's decomposition and one-round geometry
static int32_t plan_activity(csi_context* c, bool candidate, bool peer, const Range& dec, const FusedGeom& GP0, ActivityPlan* out) {
    csi_context::Activity& a = c->act;
    ActivityPlan p;
    p.on = candidate;
    if (p.on) {
        if (!a.list) {
            HIP_TRY(c, a.flags.alloc(kMaxActTiles));
            HIP_TRY(c, a.list.alloc(kMaxActTiles + 2));
            HIP_TRY(c, a.list0.alloc(kMaxActTiles + 2));
            HIP_TRY(c, a.host.alloc(4, hipHostMallocMapped));
            memset(a.host.get(), 0, sizeof(int) * 4);
            HIP_TRY(c, hipHostGetDevicePointer((void**)&a.host_dev, a.host.get(), 0));
        }
        // the newest sample the device has written (seqlock; no API call, no synchronisation): live tiles / tiles on the geometry of its sub-cycle
        if (activity_sample(c) && a.last_tiles > 0) {
            const double s_scale = a.sample_scale[(unsigned)a.seen_id % csi_context::Activity::kSamples];
            const double f = (double)std::max(a.last_live, 1) / (double)a.last_tiles;
            // keep the geometry while the live tiles fill 90 .. 100 % of a round; otherwise aim at 97 %
            if (f >= 0.97) a.scale = 1.0;
            else if (s_scale * f > 1.0 || s_scale * f < 0.90 || a.scale != s_scale) a.scale = std::min(4.0, 0.97 / f);
        }
    }
    // (Almost) nothing quiescent in the newest sample -- the headline's grid: no land, ice everywhere but one patch of open water, 987
    // of 999 tiles live --: the test, the scan, the copy below and the list-mapped launches cost 3 % of such a sub-cycle (measured: 7.12
    // against 6.89 ms at 2048^2, scripts/ab_headline_skip.sh) and leaving a dozen tiles out of a one-round launch buys nothing.  So
    // unless fewer than nine tiles in ten are live the grid is only PROBED, every kProbeEvery-th sub-cycle, and the sub-cycles in
    // between run the plain launches.  Ice-free ocean that spreads is found within that many sub-cycles; while the cut is in use the
    // test runs before every sub-cycle (it must: the list decides what is skipped).
    const bool something_quiescent = a.last_live >= 0 && 10L * a.last_live < 9L * a.last_tiles;
    if (p.on && a.last_live >= 0 && !something_quiescent) {
        constexpr int kProbeEvery = 32;
        if (++a.since_probe < kProbeEvery) p.on = false;
        else a.since_probe = 0;
    } else {
        a.since_probe = 0;
    }
    if (p.on) {
        p.GA = pair_geom(c, dec, peer ? 1.0 : a.scale);
        // (more tiles than the list holds -- a forced CSI_PAIR_TILES, a huge grid --, or another chunk layout than the tables describe: the plain launches)
        if (p.GA.nstrips * p.GA.nchunks > kMaxActTiles || p.GA.elo != GP0.elo || p.GA.ehi != GP0.ehi || p.GA.wt != GP0.wt) p.on = false;
    }
    // Tiles quiescent FROM THE START (no ice mass, velocities +0.0 already, no halo image to store): with the two buffers equal before
    // the first launch even the first two launches may leave them out.  Worth the copy that takes only when the newest sample says that
    // something is quiescent at all; not on peer-connected tiles (their copy is made before the sub-cycle's exchange, run_fused_peer).
    p.q0 = p.on && !peer && something_quiescent;
    *out = p;
    return CSI_OK;
}
// which tiles of GA are live: h, aice (constant over the sub-cycle) and the sign bits of the current stresses.  pair_tables: the pair
// tables just filled (peer: the direction sets)
static void launch_activity_test(csi_context* c, const ActivityPlan& act, const EvpDev& P, const FRef* orig, bool peer, const FusedTable* pair_tables) {
    const FusedGeom& GA = act.GA;
    ActivityArgs A{};
    A.h = ref_of(c, CSI_F_H); A.a = ref_of(c, CSI_F_A);
    A.s11 = orig[2]; A.s22 = orig[3]; A.s12 = orig[4]; A.u = orig[0]; A.v = orig[1];
    A.rho = P.rho;
    A.dec = GA.rs;
    A.nstrips = GA.nstrips; A.nchunks = GA.nchunks; A.rows = GA.rows; A.elo = GA.elo; A.ehi = GA.ehi;
    // (band: the arrays are those of the whole grid, c->Ny is the cut one -- the parents' own extents)
    auto extent = [&](int fid) { const Bound& b = c->f[fid]; return Range{1 - c->Hx, b.ni - c->Hx, 1 - c->Hy, b.nj - c->Hy}; };
    A.pc = extent(CSI_F_H); A.pf = extent(CSI_F_S12); A.pu = extent(CSI_F_U); A.pv = extent(CSI_F_V);
    A.Nx = c->Nx; A.Ny = c->Ny; A.Hx = c->Hx; A.Hy = c->Hy;      // (band: the cut grid -- the tiles next to the band count as edge tiles)
    if (peer) {
        for (int q = 0; q < 4; ++q) A.pset[q] = pair_tables->I[FI_PSET + q];
        A.pmask = pair_tables->I[FI_PMASK];
    }
    csi_context::Activity& a = c->act;
    const int id = (int)(a.seq++ & 0x3fffffffu);
    a.sample_scale[(unsigned)id % csi_context::Activity::kSamples] = a.scale;
    launch_tile_activity(A, a.flags.get(), a.list.get(), act.q0 ? a.list0.get() : nullptr, a.host_dev, id, c->stream);
    a.last_used = act.q0 ? 2 : 1;
}

// ---- stage 3, table fill: what every table of one sub-cycle shares, and the one function that fills a table of the two-sub-steps kernel
struct TableFill {
    csi_context* c; const EvpDev& P; const FastCoef& fc; const FRef *orig, *alt; const ForcingScratch& F;
    bool peer, band;
    ImageSpec imu, imv, ims11, ims22, ims12;
    // vs: the valid halo widths the STORE ranges follow (a pair: its second sub-step's), ufirst: that sub-step's order; dec: the compute
    // (stress) range the tiles decompose, a_j0 .. a_j1: the first sub-step's stress rows; G: the launch geometry; cur: the buffer read
    int32_t pair_table(const SideV& vs, bool ufirst, const Range& dec, int a_j0, int a_j1, const FusedGeom& G, int cur, FusedTable* t) const {
        Range rs = clip_store(c, dec, true), r1 = clip_store(c, v_first_range(c, vs, ufirst), false), r2 = clip_store(c, v_second_range(c, vs), false);
        if (band) {         // rows above M are the band's: it stores them into the same buffer meanwhile
            rs.j1 = std::min(rs.j1, c->Ny); r1.j1 = std::min(r1.j1, c->Ny); r2.j1 = std::min(r2.j1, c->Ny);
        }
        fused_fill_table(P, fc, cur == 0 ? orig : alt, cur == 0 ? alt : orig, rs, r1, r1, r2, imu, imv, t);
        fused_fill_pair_extra(dec, a_j0, a_j1, ims11, ims22, ims12, t, G.elo, G.ehi, G.wt);
        if (F.force) { fused_fill_forcing(P, F.ubar_v, F.vbar_u, t); if (F.wind) fused_fill_forcing_top(P, F.tbar_v, F.tbar_u, t); }
        if (F.extra) fused_fill_extra(P, F.xd_u, F.xd_v, t);
        return peer ? peer_fill_table(c, G, cur == 0, t) : CSI_OK;
    }
};

// ---- stage 4, the driver and its launch loop.
// peer: the caller (run_fused_peer) has turned the connected sides of c->g / P.g into periodic ones: the launch loop is that of an
// untiled periodic grid, the halo images of those sides go to the neighbouring tiles' arrays and every pair launch carries a
// number of the flag protocol.  band: the caller (run_fused_fold) has cut the rows next to a north fold off c->g / P.g.
int32_t run_fused(csi_context* c, const EvpDev& P, const FastCoef& fc, int substeps, int first, bool peer, const FoldBand* band) {
    int32_t rc;
    if ((rc = ensure_alt(c))) return rc;
    if (band && (rc = ensure_band(c))) return rc;
    const bool tiled = band ? band->tiled : is_tiled(c);
    const int k = band ? band->k : exchange_interval(c), W = 2 * k;
    // (band: the halo exchange of the fold tile is that of the tile as it is -- its north side has no neighbour)
    auto exchange_tile = [&](const FRef* fr) -> int32_t {
        if (band) { c->g = band->g_full; c->Ny = band->Ny_full; }
        const int32_t r = exchange_refs(c, fr, nxf_of(k), W);
        if (band) { c->g = band->g_cut; c->Ny = band->M; }
        return r;
    };
    const bool masked = P.g.has_mask != 0;
    const bool pairs = peer || (pair_supported(c) && (!tiled || k % 2 == 0));
    ForcingScratch F;
    if ((rc = forcing_scratch(c, P, &F))) return rc;
    const int kb = tiled ? k : (pairs ? 2 : 1);             // batch length: positions 0 .. kb-1
    FRef orig[5], alt[5];
    for (int q = 0; q < 5; ++q) { orig[q] = ref_of(c, kPing[q]); alt[q] = alt_ref(c, q); }
    if (tiled && (rc = exchange_tile(orig))) return rc;
    // both buffers start identical, so cells no sub-step ever writes (wall halos, the outermost halo layer of sigma
    // under the one-sub-step kernel) agree in both.  A fully periodic, untiled grid advanced by pair launches only
    // rewrites every cell of the five parents -- interior and all halo images -- at every launch: no copy needed.
    const bool every_cell_written = pairs && !tiled && !has_walls(c) && substeps % 2 == 0;
    if (k > KMAX) return fail(c, CSI_ERR_UNSUPPORTED, "exchange interval too large for the fused path");
    if (!c->dev_tables) HIP_TRY(c, c->dev_tables.alloc(NSINGLE + NPAIR));
    // configurations only the two-sub-steps kernel takes (masks, array forcing, per-point metrics): a single sub-step (the odd
    // trailing one) runs through that kernel too, its consumer wave storing stage A's results (evp_fused2.hip, `single`)
    const bool single_by_pair = pairs && (masked || F.force || c->metric_kind == CSI_METRIC_FULL || peer || band);      // (peer: the flag protocol lives in this kernel only; band: its cut tile)
    // launch geometries (host arithmetic): singles per batch position, pairs per pair position
    FusedGeom G[KMAX], GP[KMAX / 2];
    auto single_v = [&](int m) { return tiled ? W - 2 * m : 2; };
    auto pair_dec = [&](int mp) { return v_stress_range(c, pair_side_v(c, W - 4 * mp - 2, 2)); };
    for (int m = 0; m < kb; ++m)
        G[m] = single_by_pair ? pair_geom(c, v_stress_range(c, pair_side_v(c, single_v(m), 2))) : fused_geom(c, single_v(m));
    for (int mp = 0; pairs && 2 * mp + 1 < kb; ++mp) GP[mp] = pair_geom(c, pair_dec(mp));
    ActivityPlan act;
    if ((rc = plan_activity(c, c->act.enabled != 0 && pairs && !tiled && substeps >= 8, peer, pair_dec(0), GP[0], &act))) return rc;
    if ((!every_cell_written || act.q0) && !peer && (rc = copy_ping(c, true))) return rc;      // (peer: run_fused_peer has made the copy, BEFORE its exchange)
    // the tables, through the pinned ring
    if (!c->host_ring) {
        HIP_TRY(c, c->host_ring.alloc((size_t)(NSINGLE + NPAIR) * csi_context::kRing, hipHostMallocDefault));
        for (int q = 0; q < csi_context::kRing; ++q) HIP_TRY(c, hipEventCreateWithFlags(&c->ring_ev[q], hipEventDisableTiming));
    }
    const int slot = (int)(c->ring_pos++ % csi_context::kRing);
    if (c->ring_used[slot]) HIP_TRY(c, hipEventSynchronize(c->ring_ev[slot]));
    FusedTable* host = c->host_ring.get() + (size_t)slot * (NSINGLE + NPAIR);
    const TableFill T{c, P, fc, orig, alt, F, peer, band != nullptr, image_spec(c, CSI_F_U), image_spec(c, CSI_F_V),
                      image_spec(c, CSI_F_S11), image_spec(c, CSI_F_S22), image_spec(c, CSI_F_S12)};
    for (int m = 0; m < kb; ++m)
        for (int cur = 0; cur < 2; ++cur)
            for (int uf = 0; uf < 2; ++uf) {
                FusedTable* t = &host[(m * 2 + cur) * 2 + uf];
                if (single_by_pair) {
                    const SideV vs = pair_side_v(c, single_v(m), 2);
                    const Range dec = v_stress_range(c, vs);
                    if ((rc = T.pair_table(vs, uf != 0, dec, dec.j0, dec.j1, G[m], cur, t))) return rc;
                } else {
                    Range r1, r1c, r2;
                    velocity_ranges(c, uf != 0, single_v(m), r1, r1c, r2);
                    fused_fill_table(P, fc, cur == 0 ? orig : alt, cur == 0 ? alt : orig, G[m].rs, r1, r1c, r2, T.imu, T.imv, t);
                }
            }
    for (int mp = 0; pairs && 2 * mp + 1 < kb; ++mp) {
        const SideV vb = pair_side_v(c, W - 4 * mp - 2, 2);
        const Range dec = pair_dec(mp), ra = v_stress_range(c, pair_side_v(c, W - 4 * mp, 4));
        for (int cur = 0; cur < 2; ++cur)
            for (int auf = 0; auf < 2; ++auf) {
                FusedTable* t = &host[NSINGLE + (mp * 2 + cur) * 2 + auf];
                if ((rc = T.pair_table(vb, auf == 0, dec, ra.j0, ra.j1, GP[mp], cur, t))) return rc;      // (auf == 0: the second sub-step has the other order)
                if (act.on) { t->P[FP_ACT_LIVE] = (unsigned long)c->act.list.get(); t->P[FP_ACT_LIVE0] = (unsigned long)c->act.list0.get(); }
            }
    }
    HIP_TRY(c, hipMemcpyAsync(c->dev_tables.get(), host, sizeof(FusedTable) * (NSINGLE + NPAIR), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(c->ring_ev[slot], c->stream));
    c->ring_used[slot] = true;
    unsigned long long peer_dld_bit = 0ull;      // neighbours with other row strides: the DLD instantiation (bit 63 of the launch number)
    if (peer)
        for (int d = 0; d < 8; ++d) if (c->peer.dld[d][0] | c->peer.dld[d][1]) peer_dld_bit = 1ull << 63;
    c->act.last_used = 0;
    if (act.on) launch_activity_test(c, act, P, orig, peer, host + NSINGLE);
    int cur = 0;   // 0: the caller's arrays hold the current state
    int m = 0, nex = 0, nlaunch = 0, npair = 0;
    const int end = first + substeps;
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    if ((rc = stats_mark(c))) return rc;
    if (band) {
        HIP_TRY(c, hipEventRecord(c->band_ev_pair, c->stream));      // the first band starts behind everything queued so far
        HIP_TRY(c, hipEventRecord(c->band_ev_band, c->stream));      // (nothing for the first pair launch to wait for)
    }
    // the band's step beside a launch of n sub-steps: the launch waits for the previous band (its rows M + 1 .. M + 4)
    auto band_beside = [&](int s, int n) -> int32_t {
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->band_ev_band, 0));
        const int32_t r = band_substeps(c, *band, fc, cur, s, n, s + n == end);
        nlaunch += band_launches(c, n);
        return r;
    };
    const int metric = c->metric_kind == CSI_METRIC_FULL ? 2 : (c->coef.uniform != 0 ? 0 : 1);
    const bool walls_variant = has_walls(c) || masked || F.force || peer_dld_bit != 0;
    auto launch_pair_kernel = [&](int table, bool ufirst, const FusedGeom& g, int write_diag, unsigned long long seq) {
        launch_fused_pair(c->dev_tables.get() + table, metric, ufirst, walls_variant, masked, F.force, P.free_drift != 0, F.extra_kind,
                          F.common_forcing, g.nstrips, g.nchunks, g.rows, write_diag, seq, c->stream);
    };
    for (int s = first; s < end;) {
        const bool ufirst = (s % 2) == 0;                  // split_explicit_momentum_equations.jl:178
        const int tab = (cur * 2) + (ufirst ? 1 : 0);      // (buffer, order) within a position's four tables
        if (pairs && end - s >= 2 && m + 1 < kb) {
            const int mp = m / 2;
            if (band && (rc = band_beside(s, 2))) return rc;
            // (write_diag bit 2: the live tiles of GA only -- not in the first two pair launches, which bring BOTH buffers to the
            //  quiescent tiles' fixed point, halo images included, nor in the last launch, which stores every tile's diagnostics)
            const bool live_only = act.on && npair >= 2 && s + 2 != end;
            const bool start_only = act.q0 && npair < 2 && s + 2 != end;      // (the first two launches: all but the tiles quiescent from the start)
            launch_pair_kernel(NSINGLE + mp * 4 + tab, ufirst, (live_only || start_only) ? act.GA : GP[mp],
                               (s + 2 == end ? 1 : 0) | (live_only ? 4 : 0) | (start_only ? 8 : 0),
                               peer ? (++c->peer.seq | peer_dld_bit) : (c->tune.peer_kernel > 0 ? 1ull : 0ull));
            ++npair;
            if (band) HIP_TRY(c, hipEventRecord(c->band_ev_pair, c->stream));
            m += 2; s += 2;
        } else if (single_by_pair) {
            // one sub-step through the two-sub-steps kernel (write_diag bit 1): masks, array forcing, per-point metrics
            if (band && (rc = band_beside(s, 1))) return rc;
            launch_pair_kernel(m * 4 + tab, ufirst, G[m], 2 | (s + 1 == end ? 1 : 0), peer ? (++c->peer.seq | peer_dld_bit) : 0ull);
            if (band) HIP_TRY(c, hipEventRecord(c->band_ev_pair, c->stream));
            m += 1; s += 1;
        } else if (masked || F.force || c->metric_kind == CSI_METRIC_FULL) {
            // (no pair kernel for this grid -- halo < 4, tiny tiles: the three kernels in place on whichever buffer is current)
            EvpDev Q = P;
            const FRef* b = cur == 0 ? orig : alt;
            Q.u = b[0]; Q.v = b[1]; Q.s11 = b[2]; Q.s22 = b[3]; Q.s12 = b[4];
            Q.write_diag = (s + 1 == end);
            launch_substep(Q, &fc, substep_ranges(c, single_v(m)), T.imu, T.imv, ufirst, c->stream);
            m += 1; s += 1;
            cur ^= 1;           // undone below: this sub-step did not switch buffers
            nlaunch += 2;
        } else {
            launch_fused_substep(c->dev_tables.get() + m * 4 + tab, c->coef.uniform != 0, ufirst, G[m].nstrips, G[m].nchunks, G[m].rows, s + 1 == end, c->stream);
            m += 1; s += 1;
        }
        cur ^= 1;
        ++nlaunch;
        if (tiled && (m == kb || s == end)) {
            if ((rc = exchange_tile(cur == 0 ? orig : alt))) return rc;
            m = 0;
            ++nex;
        } else if (m >= kb) {
            m = 0;
        }
    }
    if (band) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->band_ev_band, 0));
    if (peer) {
        // the neighbours' last launch wrote into this rank's halos: wait for all of it before anything later on this stream
        // (the copy back, finalize_rheology!, the next exchange) reads them
        launch_wait_peers(c->peer.slots.get(), c->peer.sync_rank, csi_context::Peer::SLOTS, c->peer.nbr_wait, c->peer.seq, c->peer.err.get(), c->stream);
        HIP_TRY(c, hipMemcpyAsync(c->peer.err_host.get(), c->peer.err.get(), sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    if ((rc = stats_mark(c))) return rc;
    stats_launches(c, nlaunch);
    if (cur == 1 && (rc = copy_ping(c, false))) return rc;      // the result sits in the library's buffers
    HIP_TRY(c, hipGetLastError());
    c->last = csi_context::LastPath{c->last.timed, c->last.fused, c->last.per_substep, nlaunch, substeps, nex, k};      // (the first three: do_subcycle's)
    c->last_used_pairs = pairs && substeps >= 2;
    return CSI_OK;
}


// One sub-cycle on the peer transport: an RCCL exchange of u, v, sigma brings the halos up to date (and orders this rank behind
// whatever its neighbours did last), then the connected sides count as periodic ones for the launch loop.
int32_t run_fused_peer(csi_context* c, double dt, const FastCoef& fc, int substeps, int first) {
    int32_t rc;
    FRef orig[5];
    for (int q = 0; q < 5; ++q) orig[q] = ref_of(c, kPing[q]);
    // Both ping-pong buffers start identical where no launch ever writes (cells beyond walls).  The copy comes BEFORE the
    // exchange: once a neighbour has received this rank's message it may start its first launch, whose halo images land in this
    // rank's second buffer -- they must not be overwritten by a copy that is still on its way.  (Halos beyond connected sides
    // need no copy: the neighbours' images rewrite all H layers at every launch.)
    if ((rc = ensure_alt(c))) return rc;
    const bool fold = c->g.yhi == SIDE_FOLD;
    if ((has_walls(c) || fold) && (rc = copy_ping(c, true))) return rc;
    const int W = std::min(std::min(c->Hx, c->Hy), 4);
    if ((rc = exchange_refs(c, orig, 5, W))) return rc;
    // the fold tile of a y partition: its three-kernel band works on the tile as it is (FoldBand); the pair launches see the
    // tile cut below the band, like every other tile with its connected sides turned into periodic ones (PeerView)
    const EvpDev Pfull = evp_dev(c, dt);
    FoldBand bd = fold ? fold_band(c, Pfull, false, 2) : FoldBand{};
    PeerView view(c);
    bd.g_cut = c->g;
    EvpDev P = Pfull;           // (arrays and per-row pointers of the tile as it is; only the grid descriptor differs)
    P.g = c->g;
    rc = run_fused(c, P, fc, substeps, first, true, fold ? &bd : nullptr);
    c->last.exchanges = 1;
    return rc;
}


int32_t do_subcycle(csi_context* c, double dt, int substeps, int first) {
    int32_t rc;
    if ((rc = peer_check_entry(c))) return rc;
    if ((rc = ensure_row_constant(c))) return rc;
    launch_fill_halo_batch(halo_batch(c, {CSI_F_U, CSI_F_V}), c->g, c->stream);      // :170-171, both fields in one batch of two launches
    const bool tiled = is_tiled(c);
    // halo exchange of u, v every k sub-steps with width 2k (k = 1: every sub-step; the reference is the
    // k = substeps extreme with its 2*substeps+3 halo, split_explicit_momentum_equations.jl:51-64)
    const int k = exchange_interval(c);
    const int W = 2 * k;
    // sigma is history dependent (sigma += (sigma' - sigma) / gamma): with k = 1 the ring-1 values are
    // recomputed every sub-step and stay identical to the neighbour's; with k > 1 the outer rings skip
    // updates inside a batch, so sigma travels with u, v.  alpha is recomputed before every use.
    const int uvs[5] = {CSI_F_U, CSI_F_V, CSI_F_S11, CSI_F_S22, CSI_F_S12};
    const int nxf = k > 1 ? 5 : 2;
    if ((rc = free_drift_fields(c, dt))) return rc;
    EvpDev P = evp_dev(c, dt);
    const ImageSpec imu = image_spec(c, CSI_F_U), imv = image_spec(c, CSI_F_V);
    const bool fast = c->mode == CSI_MODE_FAST;
    const FastCoef fc = fast_coef(c, P, dt);
    if (fast && !fast_supported(P)) return fail(c, CSI_ERR_UNSUPPORTED, "CSI_MODE_FAST does not support this configuration yet; use CSI_MODE_STRICT");
    // immersed masks: only the two-sub-steps-per-launch kernel takes them (a trailing odd sub-step falls back to the
    // three kernels inside run_fused)
    const int pfk = pair_forcing_kind(P);
    const bool pair_only = P.g.has_mask || pfk == 1 || c->metric_kind == CSI_METRIC_FULL;      // configurations only the two-sub-steps kernel takes
    // the peer halo transport (tiles) needs none of the RCCL batching constraints (an even exchange interval): decide it first
    bool peer = false;
    if (fast && c->fusion && substeps > 0 && (rc = peer_decide(c, P, substeps, &peer))) return rc;
    if (!peer && fast && fold_band_supported(c, P, substeps)) {
        c->peer.last = 0;
        if ((rc = run_fused_fold(c, P, fc, substeps, first))) return rc;
        c->last = csi_context::LastPath{true, 2, 1, c->last.launches, c->last.substeps, c->last.exchanges, c->last.k};      // (the last four: run_fused's)
        return CSI_OK;
    }
    const bool fuse = peer || (fast && c->fusion && substeps > 0 &&
                               (pair_only ? (pfk >= 0 && pair_supported(c) && (!tiled || k % 2 == 0) && substeps >= 2)
                                          : fused_supported(P)));
    if (fuse) {
        c->peer.last = peer ? 1 : 0;
        if ((rc = peer ? run_fused_peer(c, dt, fc, substeps, first) : run_fused(c, P, fc, substeps, first))) return rc;
        c->last = csi_context::LastPath{true, c->last_used_pairs ? 2 : 1, 1 + ((tiled && k == 1) ? 3 : 0), c->last.launches, c->last.substeps, c->last.exchanges, c->last.k};
        return CSI_OK;
    }
    c->last.fused = 0;      // (before the exchange: a sub-cycle that fails there has left the fused paths already)
    c->peer.last = 0;
    if (tiled && (rc = exchange(c, uvs, nxf, W))) return rc;
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    if ((rc = stats_mark(c))) return rc;
    int m = 0, nex = 0;   // position inside the exchange batch
    for (int s = first; s < first + substeps; ++s) {
        if (fast) P.write_diag = (s == first + substeps - 1);
        launch_substep(P, fast ? &fc : nullptr, substep_ranges(c, W - 2 * m), imu, imv, (s % 2) == 0, c->stream);
        ++m;
        if (tiled && (m == k || s == first + substeps - 1)) {   // RCCL send/recv of the u, v halos
            if ((rc = exchange(c, uvs, nxf, W))) return rc;
            m = 0;
            ++nex;
        }
    }
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    if ((rc = stats_mark(c))) return rc;
    stats_launches(c, substeps * (fast ? 3 : 4));
    HIP_TRY(c, hipGetLastError());
    // (launches / sub-steps: not counted on this path -- they stay those of the last path that did)
    c->last = csi_context::LastPath{true, 0, (fast ? 3 : 4) + ((tiled && k == 1) ? 3 : 0), c->last.launches, c->last.substeps, nex, k};
    return CSI_OK;
}

int32_t do_finalize(csi_context* c) {
    const HaloBatch B = halo_batch(c, {CSI_F_S11, CSI_F_S12, CSI_F_S22});
    launch_fill_halo_batch(B, c->g, c->stream);
    HIP_TRY(c, hipGetLastError());
    // fill_halo_regions!(sigma) across tiles.  After a sub-cycle on the peer transport there is nothing to move: the neighbours' last
    // launch stored the images of their sigma into all H halo layers beyond the connected sides (and k_wait_peers has seen them
    // land) -- exactly the values an exchange would bring; what it would ALSO bring are the neighbours' own y fills in the corners
    // (beyond a wall next to a connected x side: nobody stores mirror images of sigma): the same fill on this tile's halo columns
    if (c->peer.last && is_tiled(c)) {
        launch_fill_halo_xcolumns(B, c->g, c->stream);
        HIP_TRY(c, hipGetLastError());
        return CSI_OK;
    }
    const int sg[3] = {CSI_F_S11, CSI_F_S12, CSI_F_S22};
    return exchange(c, sg, 3, c->Hx < c->Hy ? c->Hx : c->Hy);
}

int32_t need_evp(csi_context* c) {
    int32_t rc = need(c, {CSI_F_U, CSI_F_V, CSI_F_H, CSI_F_A, CSI_F_S11, CSI_F_S22, CSI_F_S12, CSI_F_UN, CSI_F_VN,
                          CSI_F_P, CSI_F_ALPHA, CSI_F_DELTA, CSI_F_ZETA_F, CSI_F_ZETA_C});
    if (rc) return rc;
    return need_dynamics_common(c);
}

// the checks of a momentum step after its field slots, every rheology and solver (csi_momentum.hip need_dynamics, need_evp)
int32_t need_dynamics_common(csi_context* c) {
    int32_t rc;
    if (!c->evp_set) return fail(c, CSI_ERR_NOT_BOUND, "csi_evp_params_set has not been called");
    if ((rc = check_stress_fields(c, CSI_STRESS_TOP))) return rc;
    if ((rc = check_stress_fields(c, CSI_STRESS_BOTTOM))) return rc;
    if (c->Hx < 2 || c->Hy < 2) return fail(c, CSI_ERR_INVALID_ARGUMENT, "the momentum step needs halo >= 2");
    if (c->free_drift == CSI_FREE_DRIFT_FIELDS && (!c->f[CSI_F_FREE_DRIFT_U].p || !c->f[CSI_F_FREE_DRIFT_V].p))      // free_drift = (u, v)
        return fail(c, CSI_ERR_NOT_BOUND, std::string("prescribed free-drift velocity field not bound: ") +
                                              slot_name(c->f[CSI_F_FREE_DRIFT_U].p ? CSI_F_FREE_DRIFT_V : CSI_F_FREE_DRIFT_U));
    if (c->free_drift == CSI_FREE_DRIFT_STRESS_BALANCE) {   // stress_balance_free_drift.jl:21-35: exactly one of the two stresses is a SemiImplicitStress
        const bool ts = c->stress[CSI_STRESS_TOP].kind == CSI_STRESS_SEMI_IMPLICIT, bs = c->stress[CSI_STRESS_BOTTOM].kind == CSI_STRESS_SEMI_IMPLICIT;
        if (ts == bs) return fail(c, CSI_ERR_INVALID_ARGUMENT, "StressBalanceFreeDrift needs exactly one SemiImplicitStress (top or bottom)");
    }
    if (c->Nx < c->Hx || c->Ny < c->Hy) return fail(c, CSI_ERR_UNSUPPORTED, "tile smaller than its halo");
    if (is_tiled(c) && !c->tile.set) return fail(c, CSI_ERR_NOT_BOUND, "connected topology but csi_tile_set has not been called");
    return sync_coriolis(c);
}

int32_t do_time_step_momentum(csi_context* c, double dt, int substeps, int rk_reset) {
    int32_t rc;
    if (rk_reset && (rc = reset_velocities(c))) return rc;  // :89-93
    if ((rc = do_initialize(c))) return rc;                 // :130
    // update_external_stress! :133-134: halos of the forcing fields (local boundary conditions, then tiles)
    // ... and of model.forcing.u / .v when they are arrays: inside an exchange batch the velocity kernels run on ranges that
    // extend into the halo and read the forcing there (elasto_visco_plastic_rheology.jl:391-401 is evaluated at every point
    // the step updates), so beyond a connected side the halo must hold the neighbour's values
    if ((c->f[CSI_F_FORCING_U].p != nullptr) != (c->f[CSI_F_FORCING_V].p != nullptr))
        return fail(c, CSI_ERR_NOT_BOUND, "model.forcing arrays: bind both CSI_F_FORCING_U and CSI_F_FORCING_V or neither");
    // (... and of prescribed free-drift velocity fields, which the same kernels read at the same points)
    if ((rc = update_external_stress(c))) return rc;
    if ((rc = do_subcycle(c, dt, substeps, 1))) return rc;  // :170-189
    return do_finalize(c);                                  // :192
}

AdvDev adv_dev(const csi_context* c, int scheme, double dt, int from_cache) {
    AdvDev A{};
    A.g = c->g;
    A.u = ref_of(c, CSI_F_U); A.v = ref_of(c, CSI_F_V); A.h = ref_of(c, CSI_F_H); A.a = ref_of(c, CSI_F_A);
    A.Gh = ref_of(c, CSI_F_GH); A.Ga = ref_of(c, CSI_F_GA); A.hm = ref_of(c, CSI_F_HM); A.am = ref_of(c, CSI_F_AM);
    A.has_snow = c->f[CSI_F_HS].p != nullptr && c->f[CSI_F_GHS].p != nullptr;     // snow thickness: the third tracer
    if (A.has_snow) { A.hs = ref_of(c, CSI_F_HS); A.Ghs = ref_of(c, CSI_F_GHS); A.hsm = ref_of(c, CSI_F_HSM); }
    A.scheme = scheme; A.dt = dt; A.from_cache = from_cache;
    A.w32 = c->weno_w32;
    A.nt = c->tune.adv_nt > 0 ? c->tune.adv_nt : 0;
    A.shape = c->tune.adv_shape > 0 ? c->tune.adv_shape : 0;
    A.fill_images = 0; A.im = image_spec(c, CSI_F_H);
    return A;
}

// in_step: called from csi_time_step_*.  tracers_filled: the tracer update of this stage already wrote the halo images of
// h, aice [, hs] with its stores (no mask, no thermodynamic step after it).  Inside a step the velocities are prognostic
// fields only with dynamics (sea_ice_model.jl:230,373-377): prescribed velocities keep the halos set! gave them.
int32_t do_update_state(csi_context* c, bool in_step, bool tracers_filled) {
    int32_t rc;
    if ((rc = need(c, {CSI_F_H, CSI_F_A}))) return rc;
    // mask_immersed_field_xy! of every prognostic field, then their local halo fills in one batch (two launches)
    const bool snow = c->f[CSI_F_HS].p != nullptr;
    const bool vel = c->f[CSI_F_U].p && c->f[CSI_F_V].p && (!in_step || has_dynamics(c));
    // (a grid narrower than its halo where a side has images: refused before anything is written, mask included)
    if (!tracers_filled) {
        if ((rc = fill_width_check(c, CSI_F_H))) return rc;      // (aice, hs: the same location)
    }
    if (vel && ((rc = fill_width_check(c, CSI_F_U)) || (rc = fill_width_check(c, CSI_F_V)))) return rc;
    launch_mask_center(ref_of(c, CSI_F_H), c->g, c->stream);
    launch_mask_center(ref_of(c, CSI_F_A), c->g, c->stream);
    if (snow) launch_mask_center(ref_of(c, CSI_F_HS), c->g, c->stream);
    for (int id : {CSI_F_MASS_FLUX, CSI_F_MASS_FLUX_SNOW, CSI_F_SNOWFALL_INTERCEPTED})       // sea_ice_model.jl:387-390
        if (c->f[id].p) launch_mask_center(ref_of(c, id), c->g, c->stream);
    if (vel) {
        launch_mask_u(ref_of(c, CSI_F_U), c->g, c->stream);
        launch_mask_v(ref_of(c, CSI_F_V), c->g, c->stream);
    }
    HaloBatch B{};
    auto add = [&](int fid) { halo_add(c, B, fid); };
    if (!tracers_filled) {
        add(CSI_F_H); add(CSI_F_A);
        if (snow) add(CSI_F_HS);
    }
    if (vel) { add(CSI_F_U); add(CSI_F_V); }
    launch_fill_halo_batch(B, c->g, c->stream);
    HIP_TRY(c, hipGetLastError());
    // advected tracers: masked and imaged like hs; inside a step the second half's stores have done both (csi_tracers.hip)
    if (c->trc.set && !in_step && (rc = tracers_update_state(c))) return rc;
    if (is_tiled(c)) {                                      // the MPI part of fill_halo_regions!, sea_ice_model.jl:383
        int ff[5] = {CSI_F_H, CSI_F_A, CSI_F_U, CSI_F_V, CSI_F_HS};
        int n = vel ? 4 : 2;
        if (snow) ff[n++] = CSI_F_HS;
        if ((rc = exchange(c, ff, n, c->Hx < c->Hy ? c->Hx : c->Hy))) return rc;
    }
    return CSI_OK;
}

int32_t do_tendencies(csi_context* c, int scheme) {
    int32_t rc;
    if ((rc = need(c, {CSI_F_U, CSI_F_V, CSI_F_H, CSI_F_A, CSI_F_GH, CSI_F_GA}))) return rc;
    if ((rc = advect_scheme_check(c, scheme))) return rc;
    c->last_adv = launch_tracer_tendencies(adv_dev(c, scheme, 0.0, 0), c->mode, c->stream);
    c->last_adv_stage = 0;
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}
// advection = nothing: zero tendencies (horizontal_div_Uc(..., ::Nothing, ...) = zero(grid), sea_ice_advection.jl:50); the
// tracer update still runs -- dynamic_time_step! launches unconditionally -- and resets h, aice [, hs] to Psi^- at every
// RK stage (what makes the stage-wise thermodynamic steps of an RK3 step non-cumulative)
int32_t do_tendencies_or_zero(csi_context* c, int scheme) {
    if (scheme) return do_tendencies(c, scheme);
    int32_t rc;
    if ((rc = need(c, {CSI_F_GH, CSI_F_GA}))) return rc;
    for (int id : {CSI_F_GH, CSI_F_GA, CSI_F_GHS}) {
        const Bound& b = c->f[id];
        if (b.p) HIP_TRY(c, hipMemsetAsync(b.p, 0, (size_t)b.ld * (size_t)b.nj * sizeof(double), c->stream));
    }
    return CSI_OK;
}
// fill_images: the stores also write the local halo images (periodic wrap / no-flux mirror) of h, aice [, hs]
int32_t do_tracer_step(csi_context* c, double dt, int from_cache, bool fill_images) {
    int32_t rc;
    if ((rc = need(c, {CSI_F_H, CSI_F_A, CSI_F_GH, CSI_F_GA}))) return rc;
    if (from_cache && (rc = need(c, {CSI_F_HM, CSI_F_AM}))) return rc;
    if (from_cache && c->f[CSI_F_HS].p && c->f[CSI_F_GHS].p && (rc = need(c, {CSI_F_HSM}))) return rc;
    AdvDev A = adv_dev(c, 0, dt, from_cache);
    A.fill_images = fill_images ? 1 : 0;
    launch_tracer_step(A, c->stream);
    HIP_TRY(c, hipGetLastError());
    return CSI_OK;
}

}  // namespace csi_host

// csi_profile_substeps (include/csi.h): per-kernel times of the three-kernel sub-step, or the time per launch of the fused paths
extern "C" int32_t csi_profile_substeps(csi_context* c, double dt, int32_t substeps, double* out_ms4) {
    if (!c || !out_ms4) return CSI_ERR_INVALID_ARGUMENT;
    int32_t rc = need_evp(c);
    if (rc) return rc;
    if (substeps < 2 || substeps > 64) return fail(c, CSI_ERR_INVALID_ARGUMENT, "2 <= substeps <= 64");
    EvpDev P = evp_dev(c, dt);
    const FastCoef fc = fast_coef(c, P, dt);
    const bool fast = c->mode == CSI_MODE_FAST, tiled = is_tiled(c);
    const Range rs = stress_range(c), rv = interior_range(c), ru1 = first_u_range(c);
    const ImageSpec imu = image_spec(c, CSI_F_U), imv = image_spec(c, CSI_F_V);
    const int uv[2] = {CSI_F_U, CSI_F_V};
    if (fast && c->fusion && fused_supported(P)) {
        // the fused path: one launch per sub-step or per pair (csi_last_launches); bracket the whole run with two events
        if (substeps & 1) ++substeps;                      // even count: the state ends in the caller's arrays
        bool peer = false;
        if ((rc = peer_decide(c, P, substeps, &peer))) return rc;
        if ((rc = peer ? run_fused_peer(c, dt, fc, substeps, 1) : run_fused(c, P, fc, substeps, 1))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        float t = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&t, c->ev0, c->ev1));
        out_ms4[0] = t / (c->last.launches > 0 ? c->last.launches : substeps); out_ms4[1] = out_ms4[2] = out_ms4[3] = 0.0;
        return CSI_OK;
    }
    std::vector<hipEvent_t> ev((size_t)substeps * 4 + 1);
    for (auto& e : ev) HIP_TRY(c, hipEventCreate(&e));
    if (tiled && (rc = exchange(c, uv, 2, 2))) return rc;    // sizes the buffers outside the timed part
    size_t k = 0;
    HIP_TRY(c, hipEventRecord(ev[k++], c->stream));
    for (int s = 1; s <= substeps; ++s) {
        if (fast) launch_fast_stress(P, rs, fc, c->stream);
        else { launch_strict_visc(P, rs, c->stream); launch_strict_stress(P, rs, c->stream); }
        HIP_TRY(c, hipEventRecord(ev[k++], c->stream));
        // Not launch_substep, on purpose: every kernel is timed on its own, u then v on every sub-step (the order only permutes which
        // kernel has the ring range), v on the interior range
        if (fast) launch_fast_ustep(P, ru1, imu, fc, c->stream); else launch_strict_ustep(P, ru1, imu, c->stream);
        HIP_TRY(c, hipEventRecord(ev[k++], c->stream));
        if (fast) launch_fast_vstep(P, rv, imv, fc, c->stream); else launch_strict_vstep(P, rv, imv, c->stream);
        HIP_TRY(c, hipEventRecord(ev[k++], c->stream));
        if (tiled && (rc = exchange(c, uv, 2, 2))) return rc;
        HIP_TRY(c, hipEventRecord(ev[k++], c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double acc[4] = {0, 0, 0, 0};
    for (int s = 0; s < substeps; ++s)
        for (int q = 0; q < 4; ++q) {
            float t = 0.f;
            HIP_TRY(c, hipEventElapsedTime(&t, ev[(size_t)s * 4 + q], ev[(size_t)s * 4 + q + 1]));
            acc[q] += t;
        }
    for (int q = 0; q < 4; ++q) out_ms4[q] = acc[q] / substeps;
    for (auto& e : ev) hipEventDestroy(e);
    return CSI_OK;
}
