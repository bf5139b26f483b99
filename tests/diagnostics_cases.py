"""Inputs shared by tests/test_diagnostics_ref.py (CPU) and tests/test_gpu_diagnostics.py: grids at the edges of the 64 x 64 block layout
of csrc/diagnostics.hip, the topology / metric / land / snow combinations, and fields whose extrema sit where a wrong index shows."""
import numpy as np

import cases
import climaseaice_jl_amd as csi

# 37 x 29: narrower than a wave, partial everywhere.  64 x 16: a quarter of a block (every thread has one row).  130 x 33: a two-column
# last block column.  1030 x 260: 17 x 5 records.  The block being 64 x 64, its own edges are added: 64 x 64, one exact block; 130 x 65, a
# two-column last block column AND a one-row last block row; 65 x 65, one cell beyond an exact block both ways (with Bounded directions the
# last faces then sit two past it); 1030 x 1030, 17 x 17 = 289 partial records, more than the finishing block's 256 threads.
GRIDS = {"narrow": (37, 29), "block": (64, 16), "edges": (130, 33), "many": (1030, 260), "exact_block": (64, 64), "edges_64": (130, 65),
         "block_plus_one": (65, 65), "more_records_than_threads": (1030, 1030)}
# (topology, metrics, land, snow): every topology pair twice, every metric kind at least twice, land and snow both ways
CONFIGS = {
    "pp_uniform": (("periodic", "periodic"), "uniform", False, False),
    "bb_latlon_land_snow": (("bounded", "bounded"), "latlon", True, True),
    "pb_curvilinear_land": (("periodic", "bounded"), "curvilinear", True, False),
    "bp_uniform_snow": (("bounded", "periodic"), "uniform", False, True),
    "pp_curvilinear_snow": (("periodic", "periodic"), "curvilinear", False, True),
    "bb_uniform_land": (("bounded", "bounded"), "uniform", True, False),
    "bp_latlon": (("bounded", "periodic"), "latlon", False, False),
    "pb_latlon_land_snow": (("periodic", "bounded"), "latlon", True, True),
}
THRESHOLD = 0.15


def make(Nx, Ny, topo=("periodic", "periodic"), metrics="uniform", land=False, snow=False, seed=7, **kw):
    """A cases.make_case case plus `hs` (None without snow): seeded fields, open-water and thin-ice patches, velocity noise."""
    c = cases.make_case(Nx=Nx, Ny=Ny, topo=topo, grid="rectilinear" if metrics == "uniform" else "latlon",
                        curvilinear=0.05 if metrics == "curvilinear" else None, land=0.2 if land else 0.0, random_uv=0.05, substeps=4,
                        seed=seed, **kw)
    rng = np.random.default_rng(seed + 100)
    c["hs"] = 0.1 * rng.random((Ny, Nx)) if snow else None
    if c["mask"] is None and land:
        c["mask"] = np.ones((Ny, Nx), dtype=bool)
    # ties: the maxima of h and aice occur twice, in the first row and in the last one (active cells)
    for j, i in ((0, 1), (Ny - 1, Nx - 2)):
        c["h"][j, i], c["a"][j, i] = 5.0, 1.0
        if c["mask"] is not None:
            c["mask"][j, i] = True
    return c


def spots(Nx, Ny):
    """(row, column) of the first cell, a cell of the last (partial) block column, a cell of the last row -- 0-based"""
    return {"first": (0, 0), "last_column": (min(3, Ny - 1), Nx - 1), "last_row": (Ny - 1, min(5, Nx - 1))}


def place_extrema(c, where, low=False):
    """Put the extremum of every quantity at spot `where` (a copy of the case): the maxima of |u|, |v| (negative u: the absolute value
    matters), h, aice, hs -- or, low = True, the minima of h and aice -- and make the cell active."""
    c = dict(c)
    for k in ("u", "v", "h", "a", "hs", "mask"):
        if c[k] is not None:
            c[k] = c[k].copy()
    j, i = spots(c["Nx"], c["Ny"])[where]
    if c["mask"] is not None:
        c["mask"][j, i] = True
    if low:
        c["h"][j, i], c["a"][j, i] = -0.75, -0.5
    else:
        c["u"][j, i], c["v"][j, i], c["h"][j, i], c["a"][j, i] = -3.0, 2.5, 9.0, 1.5
        if c["hs"] is not None:
            c["hs"][j, i] = 4.0
    return c


def build_model(c, mode="fast", device="cuda:0"):
    """A model without dynamics (prescribed velocities) on the case's grid: u, v, h, aice (and hs) bound, the mask set.  The fields are
    then loaded with load()."""
    kw = {}
    if c["hs"] is not None:
        kw = dict(ice_thermodynamics=csi.SlabThermodynamics(), snow_thermodynamics=csi.snow_slab_thermodynamics())
    m = csi.SeaIceModel(c["g"], dynamics=None, advection=None, timestepper="ForwardEuler", device=device, mode=mode, **kw)
    if c["mask"] is not None:
        m.set_mask(c["mask"])
    return m


def fields_of(m):
    f = {"u": m.velocities.u, "v": m.velocities.v, "h": m.ice_thickness, "a": m.ice_concentration}
    if m.snow_thickness is not None:
        f["hs"] = m.snow_thickness
    return f


def load(m, c, halo=np.nan):
    """Write the case's interiors into the model's parents with every halo element set to `halo` (no update_state!: nothing is masked
    or filled, the diagnostics see exactly these arrays)."""
    g = m.grid
    for k, fld in fields_of(m).items():
        parent = np.full((fld.nj, fld.ni), halo, dtype=np.float64)
        ny, nx = c[k].shape
        parent[g.Hy:g.Hy + ny, g.Hx:g.Hx + nx] = c[k]
        m.copy_to_field(fld, parent)
