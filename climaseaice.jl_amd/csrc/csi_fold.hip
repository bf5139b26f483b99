// csi_fold.hip -- north fold: the band of rows next to the fold on the three kernels, beside the pair launches  (split out of csi_abi.hip in round 4; see csi_ctx.h)
#include "csi_ctx.h"

namespace csi_host {

// ---- north fold: a band of rows next to the fold on the three kernels, everything below on the two-sub-steps kernel -------
// The two-sub-steps kernel cannot reproduce the reference next to a fold (it would have to recompute halo rows the reference
// READS as stored images).  But only the rows within reach of the fold need that: rows 1 .. M
// (M = Ny - Hy - 4) run through the pair kernel as a tile whose north side is "connected" -- its halo rows M + 1 .. M + 4 are
// interior rows of the same arrays --, rows above M through the three kernels, which store and read fold images exactly like
// the reference's.  Per pair of sub-steps the band, on its own stream and in its own copies of the arrays: copy rows >= M - 7
// of u, v, sigma from the current buffer, advance them by two three-kernel sub-steps on shrinking row ranges (valid from row M
// on after the second), copy rows >= M + 1 into the other buffer -- while the pair launch reads the current buffer and stores
// rows <= M of the other one.  Two events: a pair launch waits for the previous band (its halo rows), a band for the previous
// pair launch (rows M - 7 .. M of its input).
int32_t ensure_band(csi_context* c) {
    // (the band's kernels run on band_stream: a reallocation waits for that stream as well as for the context's -- the two streams
    //  that ever touch these arrays)
    for (ScratchField& b : c->band) HIP_TRY(c, b.ensure(c, c->band_stream));
    if (!c->band_stream) {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->band_stream, hipStreamNonBlocking));
        // the two events order kernels of ONE device against each other (pair launch <-> band step), sixty times per sub-cycle each: no
        // system-scope fence (what they guard reaches the host and other devices behind the kernels that follow on the context's stream).
        // CSI_BAND_EVENT_FLAGS: 0 default events (7.18-7.26 ms per tripolar step), 1 hipEventDisableSystemFence (7.04-7.06: the default),
        // 2 hipEventReleaseToDevice (7.30); profiles/r06_band.md section 6
        const int ef = c->tune.band_event_flags < 0 ? 1 : c->tune.band_event_flags;
        const unsigned evf = hipEventDisableTiming | (ef == 1 ? hipEventDisableSystemFence : (ef == 2 ? hipEventReleaseToDevice : 0u));
        HIP_TRY(c, hipEventCreateWithFlags(&c->band_ev_pair, evf));
        HIP_TRY(c, hipEventCreateWithFlags(&c->band_ev_band, evf));
    }
    return CSI_OK;
}
// one three-kernel sub-step on rows >= jlo, in place: u, v, sigma in b[0..4], diagnostics (last sub-step) in d[0..3] (alpha,
// zeta_c, zeta_f, Delta; nullptr: the caller's arrays); jlo hugely negative: the whole grid
int32_t band_substep(csi_context* c, const FoldBand& bd, const FastCoef& fc, const FRef* b, const FRef* d, bool ufirst, int jlo, bool last, hipStream_t st) {
    EvpDev Q = bd.P;
    Q.u = b[0]; Q.v = b[1]; Q.s11 = b[2]; Q.s22 = b[3]; Q.s12 = b[4];
    if (d) { Q.al = d[0]; Q.zc = d[1]; Q.zf = d[2]; Q.Dl = d[3]; }
    Q.write_diag = last;
    launch_substep(Q, &fc, bd.R.from_row(jlo), bd.imu, bd.imv, ufirst, st);
    return CSI_OK;
}
// rows >= j0 of band array q, as one entry of a copy batch (aligned16 stays 0: these batches take the 8-byte path whatever the pointers)
static void rows_from(const csi_context* c, int q, int j0, const double* src, double* dst, CopyBatch& B) {
    const Bound& b = band_bound(c, q);
    const size_t row = (size_t)(j0 - 1 + c->Hy), off = row * (size_t)b.ld;
    copy_add(B, src + off, dst + off, (long)(((size_t)b.nj - row) * (size_t)b.ld));
}
// The same without the copy kernels (round 6b; evp_fast.hip, k_band_stress / k_band_vel): the band's launches are a chain of dependent,
// latency-bound kernels beside the pair launch -- eight per pair of sub-steps with 3-4 us between two of them; this is six, each with
// every load of a point in flight at once.  The first sub-step reads the current buffer and writes the band's copies; the second
// works on those in place and stores rows >= M + 1 into the other buffer as well.  Same bits as band_substep's three kernels (the same
// value functions; tests/test_gpu_activity.py compares the two paths).
int32_t band_substeps_fused(csi_context* c, const FoldBand& bd, const FastCoef& fc, int cur, int s, int n, bool last) {
    hipStream_t st = c->band_stream;
    HIP_TRY(c, hipStreamWaitEvent(st, c->band_ev_pair, 0));
    FRef src[5], dst[5], b[5], d[4];
    for (int q = 0; q < 5; ++q) {
        const FRef o = ref_of(c, kPing[q]), a = alt_ref(c, q);
        src[q] = cur == 0 ? o : a; dst[q] = cur == 0 ? a : o;
        b[q] = band_ref(c, q);
    }
    for (int q = 0; q < 4; ++q) d[q] = band_ref(c, 5 + q);
    const FRef none{nullptr, 0};
    // one sub-step: u, v, sigma from `in` (each launch reads the component it replaces at the point itself only), results into the
    // band's copies and -- `out` -- rows >= M + 1 into dst
    auto substep = [&](const FRef* in, bool ufirst, int jlo, bool diag, bool out) {
        EvpDev Q = bd.P;
        Q.u = in[0]; Q.v = in[1]; Q.s11 = in[2]; Q.s22 = in[3]; Q.s12 = in[4];
        Q.al = d[0]; Q.zc = d[1]; Q.zf = d[2]; Q.Dl = d[3];
        Q.write_diag = diag;
        const int j0 = bd.M + 1;
        const SubstepRanges R = bd.R.from_row(jlo);
        launch_band_stress(Q, R.rs, fc, BandOut{b[2], b[3], b[4], out ? dst[2] : none, out ? dst[3] : none, out ? dst[4] : none, j0}, st);
        Q.s11 = b[2]; Q.s22 = b[3]; Q.s12 = b[4];
        const BandOut ou{b[0], none, none, out ? dst[0] : none, none, none, j0}, ov{b[1], none, none, out ? dst[1] : none, none, none, j0};
        if (ufirst) {
            launch_band_vel(Q, R.ru1, bd.imu, fc, true, ou, st);
            Q.u = b[0];                                                              // (v reads the new u)
            launch_band_vel(Q, R.r2, bd.imv, fc, false, ov, st);
        } else {
            launch_band_vel(Q, R.rv1, bd.imv, fc, false, ov, st);
            Q.v = b[1];
            launch_band_vel(Q, R.r2, bd.imu, fc, true, ou, st);
        }
    };
    if (n == 2) {
        substep(src, (s % 2) == 0, bd.M - 5, false, false);
        substep(b, ((s + 1) % 2) == 0, bd.M - 2, last, true);
    } else substep(src, (s % 2) == 0, bd.M - 3, last, true);
    if (last) {
        CopyBatch diag{};
        for (int q = 5; q < 9; ++q) rows_from(c, q, bd.M + 1, c->band[q].get(), band_bound(c, q).p, diag);
        launch_copy_batch(diag, st, 64);
    }
    HIP_TRY(c, hipEventRecord(c->band_ev_band, st));
    return CSI_OK;
}
// launches of one band step (the sub-cycle's launch statistics)
int band_launches(const csi_context* c, int n) { return c->tune.band_fused != 0 ? 3 * n : (n == 2 ? 8 : 5); }

// two sub-steps (or the trailing single one) of the band: buffer `cur` (0: the caller's arrays) -> the other one, on the band's stream
int32_t band_substeps(csi_context* c, const FoldBand& bd, const FastCoef& fc, int cur, int s, int n, bool last) {
    if (c->tune.band_fused != 0) return band_substeps_fused(c, bd, fc, cur, s, n, last);
    hipStream_t st = c->band_stream;
    HIP_TRY(c, hipStreamWaitEvent(st, c->band_ev_pair, 0));
    CopyBatch in{}, out{}, diag{};
    for (int q = 0; q < 5; ++q) {
        const Bound& b = band_bound(c, q);
        rows_from(c, q, bd.M - 7, cur == 0 ? b.p : c->alt[q].get(), c->band[q].get(), in);
        rows_from(c, q, bd.M + 1, c->band[q].get(), cur == 0 ? c->alt[q].get() : b.p, out);
    }
    launch_copy_batch(in, st, 64);
    FRef b[5], d[4];
    for (int q = 0; q < 5; ++q) b[q] = band_ref(c, q);
    for (int q = 0; q < 4; ++q) d[q] = band_ref(c, 5 + q);
    // validity after the first sub-step: sigma from row M - 5, velocities from M - 3; after the second: sigma M - 2, velocities M
    int32_t rc;
    if (n == 2) {
        if ((rc = band_substep(c, bd, fc, b, d, (s % 2) == 0, bd.M - 5, false, st))) return rc;
        if ((rc = band_substep(c, bd, fc, b, d, ((s + 1) % 2) == 0, bd.M - 2, last, st))) return rc;
    } else if ((rc = band_substep(c, bd, fc, b, d, (s % 2) == 0, bd.M - 3, last, st))) return rc;
    launch_copy_batch(out, st, 64);
    if (last) {
        for (int q = 5; q < 9; ++q) rows_from(c, q, bd.M + 1, c->band[q].get(), band_bound(c, q).p, diag);
        launch_copy_batch(diag, st, 64);
    }
    HIP_TRY(c, hipEventRecord(c->band_ev_band, st));
    return CSI_OK;
}


// A north fold on an untiled grid (RightFolded y, Periodic x): see FoldBand.
bool fold_band_supported(csi_context* c, const EvpDev& Pfull, int substeps) {
    const GridDev& g = c->g;
    if (g.yhi != SIDE_FOLD || g.xlo != SIDE_PERIODIC || g.xhi != SIDE_PERIODIC) return false;
    if (c->mode != CSI_MODE_FAST || !c->fusion || !c->pairing || substeps < 2 || c->Hy < 4) return false;
    if (g.ylo == SIDE_CONNECTED) {
        // the fold tile of a y partition: the k-batched message exchange with the tile below, pair launches need an even k
        const int k = exchange_interval(c);
        if (k % 2 != 0 || !has_comm(c) || !c->tile.set) return false;
    }
    const int M = c->Ny - c->Hy - 4;
    if (M < 2 * c->Hy + 8) return false;
    FoldCut cut(c, M);
    EvpDev P = Pfull;
    P.g = c->g;
    return pair_supported(c) && pair_forcing_kind(P) >= 0;
}
FoldBand fold_band(const csi_context* c, const EvpDev& Pfull, bool tiled, int k) {
    FoldBand bd{};
    bd.M = c->Ny - c->Hy - 4;
    bd.tiled = tiled; bd.k = k;
    bd.g_full = c->g; bd.Ny_full = c->Ny;
    bd.P = Pfull;
    bd.imu = image_spec(c, CSI_F_U); bd.imv = image_spec(c, CSI_F_V);
    bd.R = substep_ranges(c);
    return bd;
}
int32_t run_fused_fold(csi_context* c, const EvpDev& Pfull, const FastCoef& fc, int substeps, int first) {
    const bool tiled = c->g.ylo == SIDE_CONNECTED;
    FoldBand bd = fold_band(c, Pfull, tiled, tiled ? exchange_interval(c) : 2);
    FoldCut cut(c, bd.M);
    bd.g_cut = c->g;
    EvpDev P = Pfull;
    P.g = c->g;
    return run_fused(c, P, fc, substeps, first, false, &bd);
}


}  // namespace csi_host
