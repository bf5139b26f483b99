"""CPU tests of the per-region ice integrals (include/csi.h, "per-region ice integrals and extrema"): the NumPy restatement
tests/regional_ref.py against exact sums, its partition of the active cells, its n_regions = 1 case against tests/diagnostics_ref.py
bit for bit, three mistakes it tells from the rule (with the size of each effect printed); csi_regions_layout against its formula; the
structs as gcc, ctypes and the Julia stub lay them out; the builders, the result, the writer and the loader of the Python front end and
every argument error they raise.  Nothing here needs a GPU."""
import ctypes as C
import json
import math
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import climaseaice_jl_amd as csi
import diagnostics_ref as dref
import regional_ref as ref

L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.15


def fields(Ny, Nx, seed=0, snow=True, land=True):
    rng = np.random.default_rng(seed)
    h = 0.2 + 2.5 * rng.random((Ny, Nx))
    a = rng.random((Ny, Nx))
    hs = 0.3 * rng.random((Ny, Nx)) if snow else None
    az = 1.0e8 * (1.0 + rng.random((Ny, Nx)))
    mask = rng.random((Ny, Nx)) > 0.2 if land else None
    return h, a, hs, az, mask


def checkerboard(Ny, Nx, n, cell=5):
    j, i = np.mgrid[0:Ny, 0:Nx]
    return ((j // cell) * 7 + (i // cell)) % n


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(29, 37), (65, 130)])
def test_sums_lie_within_the_bound_of_the_exact_sum_and_counts_partition_the_active_cells(shape):
    Ny, Nx = shape
    h, a, hs, az, mask = fields(Ny, Nx, seed=1)
    n = 5
    ids = checkerboard(Ny, Nx, n + 2) - 1          # ids -1 .. n: -1 and n name no region
    recs, stray = ref.regions(h, a, hs, az, mask, ids, n, THR)
    for r, rec in enumerate(recs):
        member, terms = ref.region_terms(h, a, hs, az, mask, ids, r, THR)
        for k_ref, k in (("ice_volume", "ice_volume"), ("ice_area", "ice_area"), ("ice_extent", "ice_extent"), ("snow_volume", "snow_volume"),
                         ("active_area", "region_area")):
            x = terms[k_ref][member]
            exact, bound = dref.fsum_bound(x)
            print(f"{Nx} x {Ny} region {r} {k}: |restatement - fsum| = {abs(rec[k] - exact):.3e}, bound (n - 1) 2^-53 sum|x| = {bound:.3e}")
            assert abs(rec[k] - exact) <= bound
        assert rec["cells"] == int(member.sum()) == int((mask & (ids == r)).sum())
        assert rec["min_h"] == h[member].min() and rec["max_aice"] == a[member].max() and rec["max_hs"] == hs[member].max()
    assert stray == int((mask & ((ids < 0) | (ids >= n))).sum()) > 0
    assert sum(rec["cells"] for rec in recs) + stray == int(mask.sum())


@pytest.mark.parametrize("snow,land", [(True, True), (False, False)])
def test_one_region_of_all_cells_is_the_tracer_group_bit_for_bit(snow, land):
    h, a, hs, az, mask = fields(65, 130, seed=2, snow=snow, land=land)
    recs, stray = ref.regions(h, a, hs, az, mask, np.zeros((65, 130), dtype=np.int32), 1, THR)
    want = dref.tracer_group(h, a, hs, az, mask, THR)
    assert stray == 0 and len(recs) == 1
    for k in ref.KEYS:
        k_ref = {v: q for q, v in ref.RENAME.items()}.get(k, k)
        assert dref.same_bits(recs[0][k], want[k_ref]), k
    # a region with no cell: the identities
    empty = ref.region_record(h, a, hs, az, mask, np.zeros((65, 130), dtype=np.int32), 3, THR)
    assert all(dref.same_bits(empty[k], 0.0) for k in ("ice_volume", "ice_area", "ice_extent", "region_area")) and empty["cells"] == 0
    assert (empty["min_h"], empty["max_h"], empty["min_aice"], empty["max_aice"]) == (math.inf, -math.inf, math.inf, -math.inf)


def test_three_mistakes_show():
    Ny, Nx = 65, 130
    h, a, hs, az, mask = fields(Ny, Nx, seed=3)
    ids = (np.arange(Nx)[None, :] >= 70).astype(np.int32) * np.ones((Ny, 1), dtype=np.int32)      # a seam inside the second block column
    recs, _ = ref.regions(h, a, hs, az, mask, ids, 2, THR)
    eps = 2.0 ** -53
    # 1. a cell on the seam assigned to the neighbour
    wrong = ids.copy()
    j = int(np.argwhere(mask[:, 70])[0, 0])
    wrong[j, 70] = 0
    moved, _ = ref.regions(h, a, hs, az, mask, wrong, 2, THR)
    d = moved[0]["ice_volume"] - recs[0]["ice_volume"]
    term = (h[j, 70] * a[j, 70]) * az[j, 70]
    print(f"mistake 1, a seam cell in the neighbour: region 0 volume moves by {d:.6e} (the cell's term {term:.6e}), cells {recs[0]['cells']} -> {moved[0]['cells']}")
    assert moved[0]["cells"] == recs[0]["cells"] + 1 and moved[1]["cells"] == recs[1]["cells"] - 1
    assert abs(d - term) <= 2 * Nx * Ny * eps * recs[0]["ice_volume"] and d > 1e6 * eps * recs[0]["ice_volume"]
    # 2. inactive cells counted
    allcells, _ = ref.regions(h, a, hs, az, None, ids, 2, THR)
    d = allcells[1]["region_area"] - recs[1]["region_area"]
    land_area = math.fsum(az[(~mask) & (ids == 1)])
    print(f"mistake 2, inactive cells counted: region 1 area grows by {d:.6e} (its land {land_area:.6e}), cells {recs[1]['cells']} -> {allcells[1]['cells']}")
    assert allcells[1]["cells"] == int((ids == 1).sum()) > recs[1]["cells"] and abs(d - land_area) <= 2 * Nx * Ny * eps * allcells[1]["region_area"]
    # 3. the region's terms summed in an order compacted over its own cells: data for which the two orders differ, asserted first
    # (numbers of both signs over nine decades in place of a thickness -- to the rule h is data --: the sum cancels, so its low bits
    # depend on the order; with positive terms of one magnitude two orders often round to the same bits)
    rng = np.random.default_rng(4)
    h = rng.standard_normal((Ny, Nx)) * 10.0 ** rng.uniform(-3.0, 6.0, (Ny, Nx))
    recs, _ = ref.regions(h, a, hs, az, mask, ids, 2, THR)
    differ = 0
    for r in (0, 1):
        member, terms = ref.region_terms(h, a, hs, az, mask, ids, r, THR)
        stated, packed = dref.ordered_sum(terms["ice_volume"]), ref.compacted_sum(terms["ice_volume"], member)
        exact, bound = dref.fsum_bound(terms["ice_volume"][member])
        print(f"mistake 3, compacted order, region {r}: stated {stated!r} compacted {packed!r} difference {packed - stated:.3e} "
              f"({abs(packed - stated) / (eps * abs(exact)):.1f} eps of the sum; both within the bound {bound:.3e} of fsum)")
        assert abs(packed - exact) <= bound and abs(stated - exact) <= bound      # a valid sum, only another order
        assert dref.same_bits(stated, recs[r]["ice_volume"])
        differ += not dref.same_bits(stated, packed)
    assert differ == 2, "choose other data: the compacted order gives the stated order's bits"


# ---- the layout function and the structs -----------------------------------------------------------------------------------------------------

def test_layout_function_against_the_formula():
    for Nx in (1, 63, 64, 65, 127, 128, 129, 4096):
        for Ny in (1, 63, 64, 65, 128, 129):
            for n in (1, 2, 63, 64):
                rec = -(-Nx // 64) * -(-Ny // 64)
                assert L.regions_layout(Nx, Ny, n) == (rec, rec * (n + 1) * 11 * 8), (Nx, Ny, n)
    assert L.regions_layout(4096, 4096, 64)[1] == 23429120          # "about 23 MB"
    for bad in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (8, 8, 65), (8, 8, -1)):
        with pytest.raises(csi.CsiError) as e:
            L.regions_layout(*bad)
        assert e.value.code == -1
    lib = L.load()
    assert lib.csi_regions_layout(64, 64, 2, None, None) == 0       # either output pointer may be NULL
    for name, nargs in (("csi_regions_layout", 5), ("csi_regions_compute", 5), ("csi_regions_stats", 2)):
        assert len(getattr(lib, name).argtypes) == nargs and name in L.SYMBOLS


def test_c_layout_matches_ctypes_and_the_julia_stub(tmp_path):
    exe = str(tmp_path / "regions_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "regions_layout.c"), "-o", exe])
    got = json.loads(subprocess.check_output([exe]).decode())
    assert got["sizeof_regions"] == C.sizeof(L.Regions) == 24 and got["sizeof_region_record"] == C.sizeof(L.RegionRecord) == 88
    assert got["CSI_REGIONS_MAX"] == L.REGIONS_MAX == 64 and got["CSI_VERSION"] == 100
    assert got["CSI_F_COUNT_SHORTWAVE"] == 72                       # no new field slot
    for cname, T in (("csi_regions", L.Regions), ("csi_region_record", L.RegionRecord)):
        for name, _ in T._fields_:
            assert got[f"{cname}.{name}"] == getattr(T, name).offset, (cname, name)
    assert [n for n, _ in L.RegionRecord._fields_] == list(ref.KEYS)
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    size = {"Int64": 8, "Int32": 4, "Cdouble": 8}
    for jl, cname, T in (("CsiRegions", "csi_regions", L.Regions), ("CsiRegionRecord", "csi_region_record", L.RegionRecord)):
        body = re.search(r"^struct %s\n(.*?)\nend" % jl, stub, re.S | re.M).group(1)
        off, offsets = 0, {}
        for name, t in re.findall(r"(\w+)::((?:Ptr\{\w+\})|\w+)", body):
            s = 8 if t.startswith("Ptr{") else size[t]
            off = (off + s - 1) // s * s
            offsets[name] = off
            off += s
        assert offsets == {n: got[f"{cname}.{n}"] for n, _ in T._fields_} and off == C.sizeof(T), jl
    assert re.search(r"ccall\(\(:csi_regions_compute, libcsi\), Int32, \(Ptr\{Cvoid\}, Ref\{CsiRegions\}, Cdouble, Ptr\{CsiRegionRecord\}, Ref\{Int64\}\)", stub)
    assert re.search(r"ccall\(\(:csi_regions_layout, libcsi\), Int32, \(Int32, Int32, Int32, Ref\{Int64\}, Ref\{Int64\}\)", stub)
    assert re.search(r"ccall\(\(:csi_regions_stats, libcsi\), Int32, \(Ptr\{Cvoid\}, Ref\{Int64\}\)", stub)
    assert "function regional_diagnostics(model::HIPSeaIceModel, ids, n" in stub and re.search(r"^const REGIONS_MAX = 64$", stub, re.M)


# ---- the builders ----------------------------------------------------------------------------------------------------------------------------

def test_hemispheres_on_a_latitude_longitude_grid_straddling_the_equator():
    g = csi.LatitudeLongitudeGrid((8, 7), longitude=(0, 80), latitude=(-35, 35))      # row 4's centres lie ON the equator
    r = csi.Regions.hemispheres(g)
    assert r.names == ("south", "north") and r.n == 2 and r.ids.dtype == np.int32 and r.ids.shape == (7, 8)
    assert np.array_equal(r.ids[:, 0], [0, 0, 0, 1, 1, 1, 1]) and np.all(r.ids == r.ids[:, :1])
    assert g.ynodes(csi.Center)[3] == 0.0 and not r.ids.flags.writeable
    assert r.index("north") == 1 and r.index(0) == 0
    with pytest.raises(KeyError, match="'east'"):
        r.index("east")


def test_hemispheres_on_a_small_tripolar_grid():
    g = csi.TripolarGrid((32, 24), halo=(4, 4))
    r = csi.Regions.hemispheres(g)
    lat = g.nodes_2d(csi.Center, csi.Center)[1]
    assert np.array_equal(r.ids == 1, lat >= 0) and 0 < int((r.ids == 0).sum()) < r.ids.size
    assert np.all(r.ids[-1] == 1) and np.all(r.ids[0] == 0)
    tile = csi.TileGrid(g, 1, 2, 0, 1)
    assert np.array_equal(csi.Regions.hemispheres(tile).ids, r.ids)                  # a tile's builder maps the global grid
    assert np.array_equal(r.piece(tile), r.ids[12:, :])


def test_grids_without_latitudes_are_refused_by_name():
    rect = csi.RectilinearGrid((16, 12), x=(0, 1), y=(0, 1), halo=(4, 4))
    with pytest.raises(NotImplementedError, match="Regions.hemispheres.*RectilinearGrid has no cell-centre latitudes"):
        csi.Regions.hemispheres(rect)
    with pytest.raises(NotImplementedError, match="Regions.latitude_bands.*OrthogonalCurvilinearGrid"):
        csi.Regions.latitude_bands(csi.OrthogonalCurvilinearGrid.from_grid(rect), [0.0, 1.0])


def test_latitude_bands_at_exact_edges():
    g = csi.LatitudeLongitudeGrid((4, 8), longitude=(0, 40), latitude=(50, 90))      # centres 52.5, 57.5, ..., 87.5
    r = csi.Regions.latitude_bands(g, [57.5, 67.5, 87.5])
    assert np.array_equal(r.ids[:, 0], [-1, 0, 0, 1, 1, 1, 1, -1])                   # an edge belongs to the band above it; the last edge to none
    assert r.names == ("57.5..67.5", "67.5..87.5")
    assert csi.Regions.latitude_bands(g, [0, 60, 90], names=("low", "high")).names == ("low", "high")
    for edges in ([60.0], [60.0, 60.0], [70.0, 60.0], [60.0, math.nan], [60.0, math.inf]):
        with pytest.raises(ValueError, match="strictly increasing finite"):
            csi.Regions.latitude_bands(g, edges)
    with pytest.raises(ValueError, match="2 bands need 2 names"):
        csi.Regions.latitude_bands(g, [50, 60, 70], names=("one",))


def test_from_masks_overlap_and_uncovered_cells():
    g = csi.RectilinearGrid((6, 4), x=(0, 1), y=(0, 1))
    west, east = np.zeros((4, 6), dtype=bool), np.zeros((4, 6), dtype=bool)
    west[:, :2], east[:, 4:] = True, True
    for r in (csi.Regions.from_masks({"west": west, "east": east}), csi.Regions.from_masks({"west": west, "east": east}, grid=g)):
        assert r.names == ("west", "east") and np.array_equal(r.ids[0], [0, 0, -1, -1, 1, 1])
    east[:, 1] = True
    with pytest.raises(ValueError, match="masks 'west' and 'east' overlap in 4 cells"):
        csi.Regions.from_masks({"west": west, "east": east})
    with pytest.raises(ValueError, match="mask 'east' must be a boolean array of shape"):
        csi.Regions.from_masks({"west": west, "east": east.astype(int)})
    with pytest.raises(ValueError, match="mask 'w' must be a boolean array of shape"):
        csi.Regions.from_masks({"w": west}, grid=csi.RectilinearGrid((5, 4), x=(0, 1), y=(0, 1)))
    with pytest.raises(ValueError, match="no masks"):
        csi.Regions.from_masks({})


def test_argument_errors_of_the_front_end():
    g = csi.RectilinearGrid((6, 4), x=(0, 1), y=(0, 1))
    ids = np.zeros((4, 6), dtype=np.int64)
    assert csi.Regions(g, ids).names == ("0",) and csi.Regions(g, ids + 2).names == ("0", "1", "2")
    assert csi.Regions(g, ids - 1).names == ("0",)                                   # nothing assigned: still one (empty) region
    assert csi.Regions(g, ids + 10 ** 6, names=("a", "b")).n == 2                    # ids beyond the names name no region
    with pytest.raises(TypeError, match="integer array"):
        csi.Regions(g, ids.astype(float))
    with pytest.raises(TypeError, match="integer array"):
        csi.Regions(g, ids.astype(bool))
    with pytest.raises(ValueError, match=r"shape \(Ny, Nx\) = \(4, 6\)"):
        csi.Regions(g, ids.T)
    with pytest.raises(ValueError, match="must fit int32"):
        csi.Regions(g, ids + 2 ** 31, names=("a",))
    with pytest.raises(ValueError, match="at most 64 regions per map"):
        csi.Regions(g, ids + 64)
    with pytest.raises(ValueError, match="between 1 and 64 regions per map, got 65"):
        csi.Regions(g, ids, names=[str(k) for k in range(65)])
    with pytest.raises(ValueError, match="between 1 and 64 regions per map, got 0"):
        csi.Regions(g, ids, names=[])
    with pytest.raises(ValueError, match="distinct"):
        csi.Regions(g, ids, names=("a", "a"))
    r = csi.Regions(g, ids)
    with pytest.raises(ValueError, match="made for a 6 x 4 grid, the model's is 8 x 8"):
        r.piece(csi.RectilinearGrid((8, 8), x=(0, 1), y=(0, 1)))
    with pytest.raises(TypeError, match="must be a csi.Regions"):
        csi.regions.regional_diagnostics(SimpleNamespace(), ids)
    with pytest.raises(NotImplementedError, match="time averages of regional series are not built"):
        csi.RegionalSeriesWriter(r, csi.AveragedTimeInterval(1.0), "unused")
    with pytest.raises(TypeError, match="must be a csi.Regions"):
        csi.RegionalSeriesWriter(ids, csi.IterationInterval(1), "unused")
    # the device parent: laid out like a (c,c) parent, halo elements -1, built once
    gh = csi.RectilinearGrid((6, 4), x=(0, 1), y=(0, 1), halo=(2, 3))
    p = r.device_parent(gh, "cpu")
    assert p.shape == (10, 10) and p.dtype.is_floating_point is False and np.array_equal(p.numpy()[3:7, 2:8], r.ids)
    assert (p.numpy() == -1).sum() == 100 - 24 and r.device_parent(gh, "cpu") is p


# ---- the result, the writer and the loader ---------------------------------------------------------------------------------------------------

def _stand_in(g, mask, seed=0, snow=True):
    """A model-like object for the writer (as tests/test_drifters_ref.py makes them) and the recorder that stands in for the device
    call: the restatement on the model's host arrays."""
    h, a, hs, az, _ = fields(g.Ny, g.Nx, seed=seed, snow=snow, land=False)
    m = SimpleNamespace(grid=g, clock=SimpleNamespace(time=0.0, iteration=0), h=h, a=a, hs=hs, az=az, mask=mask, sea_ice_density=900.0)

    def recorder(regions, model, thr):
        recs, stray = ref.regions(model.h, model.a, model.hs, model.az, model.mask, regions.ids, regions.n, thr)
        v = ref.vectors(recs)
        v["ice_mass"] = [model.sea_ice_density * x for x in v["ice_volume"]]
        if model.hs is None:
            v["snow_volume"] = v["max_hs"] = None
        return csi.RegionalDiagnostics(regions.names, model.hs is not None, thr, stray, v)
    return m, recorder


def test_result_is_immutable_and_indexable_by_name():
    g = csi.LatitudeLongitudeGrid((8, 6), longitude=(0, 80), latitude=(-30, 30))
    r = csi.Regions.hemispheres(g)
    m, recorder = _stand_in(g, None, snow=False)
    d = recorder(r, m, THR)
    assert d.names == ("south", "north") and len(d) == 2 and d.unassigned_cells == 0 and d.has_snow is False and d.extent_threshold == THR
    assert d.snow_volume is None and d.max_hs is None and d.cells.dtype == np.int64 and list(d.cells) == [24, 24]
    assert d["north"]["ice_volume"] == d.ice_volume[1] == d[1]["ice_volume"] and d["north"]["snow_volume"] is None
    assert d["south"]["ice_mass"] == 900.0 * d.ice_volume[0] and isinstance(d["south"]["cells"], int)
    with pytest.raises(ValueError):
        d.ice_volume[0] = 1.0
    with pytest.raises(AttributeError, match="immutable"):
        d.ice_volume = None
    with pytest.raises(TypeError):
        d["north"]["ice_volume"] = 0.0
    with pytest.raises(KeyError, match="'east'"):
        d["east"]
    with pytest.raises(KeyError):
        d[2]


def test_writer_and_loader_on_a_stand_in_model(tmp_path):
    g = csi.LatitudeLongitudeGrid((12, 10), longitude=(0, 120), latitude=(-50, 50))
    mask = np.ones((10, 12), dtype=bool)
    mask[4:6, 3:5] = False
    m, recorder = _stand_in(g, mask, seed=5)
    r = csi.Regions.latitude_bands(g, [-50, -20, 20, 40], names=("s", "tropics", "n"))      # the northernmost row belongs to no band
    w = csi.RegionalSeriesWriter(r, csi.IterationInterval(2), str(tmp_path / "series"), extent_threshold=0.3, recorder=recorder)
    writers = {"regions": w}
    want = []
    for step in range(5):
        for x in writers.values():
            x.begin(m)
        if step == 0:
            want.append(recorder(r, m, 0.3))
        m.h = m.h * 0.97 + 0.01 * step
        m.clock.time += 600.0
        m.clock.iteration += 1
        for x in writers.values():
            x.after_step(m, 600.0)
        if m.clock.iteration % 2 == 0:
            want.append(recorder(r, m, 0.3))
        assert np.load(str(tmp_path / "series" / "ice_volume.npy")).shape == (len(want), 3)      # valid after every record
    w.close()
    assert w.records == 3
    out = csi.load_regional_series(str(tmp_path / "series"))
    assert out["names"] == ("s", "tropics", "n") and list(out["iteration"]) == [0, 2, 4] and list(out["time"]) == [0.0, 1200.0, 2400.0]
    assert list(out["unassigned_cells"]) == [12, 12, 12] and out["cells"].dtype == np.int64 and out["cells"].shape == (3, 3)
    for k in csi.regions.QUANTITIES:
        assert out[k].tobytes() == np.array([getattr(d, k) for d in want]).tobytes(), k
    assert not np.array_equal(out["ice_volume"][0], out["ice_volume"][2])
    meta = json.load(open(str(tmp_path / "series" / "meta.json")))
    assert meta["names"] == ["s", "tropics", "n"] and meta["extent_threshold"] == 0.3 and meta["grid"] == {"Nx": 12, "Ny": 10}
    with pytest.raises(FileExistsError):
        csi.RegionalSeriesWriter(r, csi.IterationInterval(2), str(tmp_path / "series"))
    # without snow the snow files are not made; TimeInterval schedules work the same way
    m2, rec2 = _stand_in(g, None, snow=False)
    with csi.RegionalSeriesWriter(r, csi.TimeInterval(1000.0), str(tmp_path / "nosnow"), recorder=rec2) as w2:
        w2.write(m2)
    out = csi.load_regional_series(str(tmp_path / "nosnow"))
    assert "snow_volume" not in out and "max_hs" not in out and out["ice_area"].shape == (1, 3)
