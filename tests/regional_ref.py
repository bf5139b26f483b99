"""NumPy restatement of csi_regions_compute (include/csi.h, "per-region ice integrals and extrema"), built on tests/diagnostics_ref.py:
region r is the diagnostics' tracer group on `active & (ids == r)` -- the same terms, the same documented summation order, a cell of
another region contributing the identity.  Nothing here is taken from the library."""
import numpy as np

import diagnostics_ref as dref

SUMS = ("ice_volume", "ice_area", "ice_extent", "snow_volume", "region_area")
EXTREMA = ("min_h", "max_h", "min_aice", "max_aice", "max_hs")
KEYS = SUMS + EXTREMA + ("cells",)
RENAME = {"active_area": "region_area", "active_cells": "cells"}      # the tracer group's name -> the region record's


def active_of(shape, mask):
    return np.ones(shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)


def region_record(h, a, hs, az, mask, ids, r, threshold=0.15):
    """Region r's record: dref.tracer_group with the mask replaced by mask AND (ids == r)."""
    g = dref.tracer_group(h, a, hs, az, active_of(h.shape, mask) & (np.asarray(ids) == r), threshold)
    out = {RENAME.get(k, k): v for k, v in g.items() if not k.startswith("nonfinite_")}
    return {k: out[k] for k in KEYS}


def regions(h, a, hs, az, mask, ids, n_regions, threshold=0.15):
    """(one dict per region, unassigned_cells): the active cells whose id lies outside 0 .. n_regions - 1 are counted, nothing else."""
    ids = np.asarray(ids)
    act = active_of(h.shape, mask)
    stray = int(np.count_nonzero(act & ((ids < 0) | (ids >= n_regions))))
    return [region_record(h, a, hs, az, mask, ids, r, threshold) for r in range(n_regions)], stray


def region_terms(h, a, hs, az, mask, ids, r, threshold=0.15):
    """(membership, the five (Ny, Nx) term arrays of region r, +0.0 outside it)"""
    return dref.tracer_terms(h, a, hs, az, active_of(h.shape, mask) & (np.asarray(ids) == r), threshold)


def compacted_sum(terms, member):
    """A MISTAKE, for tests: region r's terms summed in the documented order applied to its OWN cells packed into the grid's first
    rows (row-major, the rest +0.0) instead of where they are."""
    packed = np.zeros(terms.size)
    vals = terms[member]
    packed[:vals.size] = vals
    return dref.ordered_sum(packed.reshape(terms.shape))


def vectors(records):
    """A list of region dicts -> one list per quantity, as a RegionalDiagnostics holds them."""
    return {k: [rec[k] for rec in records] for k in KEYS}


def compare(result, records, stray, keys=KEYS):
    """(region, name, got, want) wherever a csi RegionalDiagnostics differs by a bit from the restatement; the count likewise."""
    bad = []
    for r, want in enumerate(records):
        for k in keys:
            vec = getattr(result, k)
            got = None if vec is None else vec[r].item()
            w = want[k]
            if not dref.same_bits(got, w if w is None or isinstance(w, int) else float(w)):
                bad.append((r, k, got, w))
    if result.unassigned_cells != stray:
        bad.append(("unassigned_cells", result.unassigned_cells, stray))
    return bad
