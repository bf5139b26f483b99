// regions.hip -- the diagnostics' tracer group per region of a caller-supplied id map (include/csi.h: csi_regions_compute).
//
//   k_regions_partial     one pass over the interior i = 1 .. Nx, j = 1 .. Ny with the block shape and tile walk of ordered_reduce.h.  A
//                         thread issues every load of its sixteen cells first (h, aice, hs if bound, the mask byte, the id, Az by metric
//                         kind) and keeps them in registers; the block ORs a 64-bit presence word together in LDS (bit r: some cell of
//                         the tile belongs to region r); then ONE accumulate-and-block_fold pass per PRESENT region over the registers,
//                         a cell of another region contributing the identity.  The loop over the presence word is block-uniform.  Regions
//                         absent from the tile get identity records by plain stores.  A tile inside one region costs one pass.
//   red::finish_records   one block per region (and one for the cells of no region) folds that region's records into its result slots
// Record layout: csi_kernels.h RegionsDev.  What a cell contributes to a slot is diagnostics.hip's tracer group, statement for statement:
// region r's record holds the bits k_diag_partial<false, true> leaves under the mask `mask AND (id == r)`.
// An id is only ever COMPARED (and, once known to lie in 0 .. n_regions - 1, used as a shift count): no id value forms an address.
// No global atomics, no flags, no hand-off between workgroups.  Compiled without contraction; STRICT and FAST run the same code.
#include "csi_dev.h"
#include "csi_kernels.h"
#include "ordered_reduce.h"

namespace csi {
namespace regions {

using namespace red;

using Kinds = RegionKinds;      // csi_kernels.h
struct OneCount { __host__ __device__ static constexpr int kind(int) { return K_CNT; } };

// MK: the grid's metric kind (what Az is read from); MASK: a mask is set.  Both are the launch's to choose, so the sixteen unrolled rows
// of loads hold no block-uniform test
template <int MK, bool MASK>
__global__ void __launch_bounds__(256) k_regions_partial(RegionsDev D) {
    const GridDev& g = D.g;
    const int i = tile_col();
    const int ic = min(i, g.Nx);
    const int n = D.n_regions;
    // ---- every load, once: addresses clamped into the interior, the value discarded by a select where the lane is outside the grid
    double h[kRowsPerThread], a[kRowsPerThread], hs[kRowsPerThread], az[kRowsPerThread];
    int id[kRowsPerThread];      // the raw id; after the second loop the region the cell belongs to, or -1: outside the grid, inactive,
                                 // or an id outside 0 .. n - 1
    unsigned char wet[kRowsPerThread];
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int jc = min(tile_row(r), g.Ny);
        h[r] = D.h.ld_(ic, jc);
        a[r] = D.a.ld_(ic, jc);
        const double hs_raw = (D.has_hs ? D.hs : D.h).ld_(ic, jc);      // (no snow layer: h's element, discarded)
        hs[r] = D.has_hs ? hs_raw : 0.0;
        az[r] = MK == 0 ? g.dx * g.dy : MK == 1 ? g.azc[jc] : metric2(g, 2, LOC_C, LOC_C, ic, jc);      // (csi_dev.h azm at (c, c))
        id[r] = D.ids[ic + (long)jc * D.ids_ld];
        wet[r] = MASK ? g.mask[ic + (long)jc * g.mask_ld] : 1;      // (csi_dev.h inactive_cell at an interior cell: its mask byte)
    }
    unsigned long long mine = 0;
    int stray = 0;               // active cells of this thread that belong to no region
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
        const bool act = (i <= g.Nx) & (tile_row(r) <= g.Ny) & (wet[r] != 0);
        const int raw = id[r];
        const bool known = (raw >= 0) & (raw < n);
        id[r] = (act & known) ? raw : -1;
        mine |= (act & known) ? (1ull << (raw & 63)) : 0ull;
        stray += (int)(act & !known);
        // (formed HERE: sunk to their first use, behind the barriers below, they hold sixteen rows' compare masks in scalar registers,
        // more than there are)
        asm volatile("" : "+v"(id[r]), "+v"(mine), "+v"(stray));
    }
    // ---- which regions occur in this tile
    __shared__ unsigned long long present_sm;
    const int tid = (int)(threadIdx.y * kTileCols + threadIdx.x);
    if (tid == 0) present_sm = 0;
    __syncthreads();
    if (mine) atomicOr(&present_sm, mine);      // (an LDS atomic: inside the workgroup)
    __syncthreads();
    const unsigned long long all = present_sm;
    const unsigned long long present = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(all >> 32)) << 32) |
                                       (unsigned)__builtin_amdgcn_readfirstlane((int)(all & 0xffffffffull));
    const long rec = tile_record();
    // ---- identity records of the absent regions, and the identity slots of the record of the cells of no region
    for (int k = tid; k < (n + 1) * RQ_COUNT; k += 256) {
        const int r = k / RQ_COUNT, q = k - r * RQ_COUNT;
        const bool absent = r < n ? !((present >> r) & 1ull) : q != RQ_CELLS;
        if (absent) D.part[(long)k * D.nrec + rec] = identity(Kinds::kind(q));
    }
    {
        double c1[1] = {cnt((long long)stray)};
        block_fold<1, 0, 1, OneCount>(c1, (int)threadIdx.x, (int)threadIdx.y, tid, D.part + ((long)n * RQ_COUNT + RQ_CELLS) * D.nrec + rec, D.nrec);
    }
    // ---- one pass per present region, ascending
    for (unsigned long long left = present; left; left &= left - 1) {
        const int reg = __builtin_ctzll(left);
        double acc[RQ_COUNT];
        set_identity<RQ_COUNT, Kinds>(acc);
        long long cells = 0;
#pragma unroll
        for (int r = 0; r < kRowsPerThread; ++r) {
            const bool act = id[r] == reg;
            // (an empty statement the compiler must take to rewrite the four values: without it every product and every canonicalised
            // operand below, invariant in the region loop, is hoisted out of it and held for all sixteen rows -- some 490 registers)
            asm volatile("" : "+v"(h[r]), "+v"(a[r]), "+v"(hs[r]), "+v"(az[r]));
            acc[RQ_VOLUME] = acc[RQ_VOLUME] + (act ? (h[r] * a[r]) * az[r] : 0.0);
            acc[RQ_AREA] = acc[RQ_AREA] + (act ? a[r] * az[r] : 0.0);
            acc[RQ_EXTENT] = acc[RQ_EXTENT] + ((act & (a[r] >= D.threshold)) ? az[r] : 0.0);
            acc[RQ_SNOW_VOLUME] = acc[RQ_SNOW_VOLUME] + (act ? (hs[r] * a[r]) * az[r] : 0.0);
            acc[RQ_REGION_AREA] = acc[RQ_REGION_AREA] + (act ? az[r] : 0.0);
            acc[RQ_MIN_H] = fmin(acc[RQ_MIN_H], act ? h[r] : INFINITY);
            acc[RQ_MAX_H] = fmax(acc[RQ_MAX_H], act ? h[r] : -INFINITY);
            acc[RQ_MIN_AICE] = fmin(acc[RQ_MIN_AICE], act ? a[r] : INFINITY);
            acc[RQ_MAX_AICE] = fmax(acc[RQ_MAX_AICE], act ? a[r] : -INFINITY);
            acc[RQ_MAX_HS] = fmax(acc[RQ_MAX_HS], act ? hs[r] : -INFINITY);
            cells += (long long)act;        }
        acc[RQ_CELLS] = cnt(cells);
        __syncthreads();      // the previous pass's fold has been read out of block_fold's LDS
        block_fold<RQ_COUNT, 0, RQ_COUNT, Kinds>(acc, (int)threadIdx.x, (int)threadIdx.y, tid, D.part + (long)reg * RQ_COUNT * D.nrec + rec, D.nrec);
    }
}

}  // namespace regions

template <int MK> static void launch_partial(const RegionsDev& D, hipStream_t s) {
    const dim3 b = red::tile_threads(), g = red::tile_blocks(D.g.Nx, D.g.Ny);
    if (D.g.has_mask) hipLaunchKernelGGL((regions::k_regions_partial<MK, true>), g, b, 0, s, D);
    else hipLaunchKernelGGL((regions::k_regions_partial<MK, false>), g, b, 0, s, D);
}

void launch_regions(const RegionsDev& D, double* out, hipStream_t s) {
    if (D.g.metric_kind == 0) launch_partial<0>(D, s);
    else if (D.g.metric_kind == 1) launch_partial<1>(D, s);
    else launch_partial<2>(D, s);
    red::launch_finish<RQ_COUNT, 0, RQ_COUNT, RegionKinds, 2>(D.part, D.nrec, out, s, D.n_regions + 1);
}

}  // namespace csi
