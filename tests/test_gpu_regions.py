"""csi_regions_compute (csrc/regions.hip) on the GPU, bit for bit -- against the NumPy restatement of the documented order
(tests/regional_ref.py), against csi_diagnostics_compute(CSI_DIAG_TRACERS) of the same build under the mask `mask AND (ids == r)`, and
against the plain tracer group for the one-region map: grids at the edges of the 64 x 64 block layout, the topologies, metric kinds,
land and snow of tests/diagnostics_cases.py, STRICT and FAST; maps that split blocks by column and by row, a single-cell region in the
last partial column, an empty region, 64 regions inside every tile, bands on block edges, ids that name no region; halo isolation, -0.0,
the threshold, NaN inside one region, repetition, state after steps, errors by name, the launch count, the series writer; tiles over the
three things that join ranks.  Tiled sums: |tiled - untiled| <= (n - 1) 2^-53 sum |terms| with n the grid's cell count."""
import ctypes as C
import json
import math
import multiprocessing as mp
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import diagnostics_cases as dc
import diagnostics_ref as dref
import regional_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NGPU = torch.cuda.device_count()
_L = csi._lib
I32 = np.iinfo(np.int32)
GRIDS = {"narrow": (37, 29), "exact_block": (64, 64), "block_plus_one": (65, 65), "edges_64": (130, 65)}


def maps(Nx, Ny):
    """name -> (ids, n_regions)"""
    j, i = np.mgrid[0:Ny, 0:Nx]
    out = {}
    out["halves_by_column"] = ((i >= 20).astype(np.int32), 2)                       # the seam inside the first block
    out["halves_by_row"] = ((j >= 11).astype(np.int32), 2)
    one = np.zeros((Ny, Nx), dtype=np.int32)
    one[min(3, Ny - 1), Nx - 1] = 1                                                 # a single cell in the last (partial) column;
    out["single_cell_and_empty"] = (one, 4)                                         # regions 2 and 3 have no cell
    out["one_region"] = (np.zeros((Ny, Nx), dtype=np.int32), 1)
    out["sixty_four_in_every_tile"] = (((j % 8) * 8 + i % 8).astype(np.int32), 64)  # the longest region loop
    out["bands_on_block_edges"] = ((i // 64 + 3 * (j // 64)).astype(np.int32), 6)
    stray = ((j // 3 + i // 5) % 3).astype(np.int32)
    bad = (-1, 64, I32.min, I32.max, 3)
    rng = np.random.default_rng(Nx * 1000 + Ny)
    spots = rng.choice(Nx * Ny, size=min(60, Nx * Ny // 4), replace=False)
    stray.reshape(-1)[spots] = np.array(bad, dtype=np.int64)[np.arange(spots.size) % len(bad)].astype(np.int32)
    stray[0, 0], stray[Ny - 1, Nx - 1] = I32.min, I32.max
    out["ids_that_name_no_region"] = (stray, 3)
    return out


def restate(c, ids, n, threshold=dc.THRESHOLD):
    _, _, az = dref.metrics_of(c["g"])
    return ref.regions(c["h"], c["a"], c["hs"], az, c["mask"], ids, n, threshold)


def regions_of(c, ids, n):
    return csi.Regions(c["g"], ids, names=[f"r{k}" for k in range(n)])


def bits(d):
    """A RegionalDiagnostics as a dict of bytes / None / int: equal dicts are equal bit for bit."""
    out = {k: (None if getattr(d, k) is None else getattr(d, k).tobytes()) for k in csi.regions.QUANTITIES}
    out["unassigned_cells"] = d.unassigned_cells
    return out


# ---- the layout: every grid x every combination x every map, both modes, twice -----------------------------------------------------------
@pytest.mark.parametrize("config", sorted(dc.CONFIGS))
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_bitwise_against_the_restatement(grid, config):
    topo, metrics, land, snow = dc.CONFIGS[config]
    c = dc.make(*GRIDS[grid], topo=topo, metrics=metrics, land=land, snow=snow)
    m = dc.build_model(c, mode="strict")
    dc.load(m, c, halo=np.nan)
    assert m.ctx.regions_stats() == 0
    calls = 0
    for name, (ids, n) in maps(c["Nx"], c["Ny"]).items():
        want, stray = restate(c, ids, n)
        r = regions_of(c, ids, n)
        m.set_mode("strict")
        first = m.regional_diagnostics(r, extent_threshold=dc.THRESHOLD)
        bad = ref.compare(first, want, stray)
        print(grid, config, name, "volume", list(first.ice_volume[:4]), "cells", list(first.cells[:4]), "unassigned", first.unassigned_cells)
        assert not bad, (name, bad[:6])
        assert first.has_snow == snow and first.names == r.names and (first.snow_volume is None) == (not snow)
        assert list(first.ice_mass) == [m.sea_ice_density * v for v in first.ice_volume]
        active = c["Nx"] * c["Ny"] if c["mask"] is None else int(c["mask"].sum())
        assert int(first.cells.sum()) + first.unassigned_cells == active, name
        assert bits(m.regional_diagnostics(r, extent_threshold=dc.THRESHOLD)) == bits(first), (name, "two calls in a row differ")
        m.set_mode("fast")
        assert bits(m.regional_diagnostics(r, extent_threshold=dc.THRESHOLD)) == bits(first), (name, "FAST differs from STRICT")
        calls += 3
        if name == "one_region":                # ... is the plain tracer group of the same build
            d = m.diagnostics("tracers", extent_threshold=dc.THRESHOLD)
            for k, kd in (("ice_volume", "ice_volume"), ("ice_area", "ice_area"), ("ice_extent", "ice_extent"), ("snow_volume", "snow_volume"),
                          ("region_area", "active_area"), ("min_h", "min_h"), ("max_h", "max_h"), ("min_aice", "min_aice"),
                          ("max_aice", "max_aice"), ("max_hs", "max_hs"), ("cells", "active_cells")):
                got = getattr(first, k)
                assert dref.same_bits(None if got is None else got[0].item(), getattr(d, kd)), k
        if name == "single_cell_and_empty":
            jj, ii = min(3, c["Ny"] - 1), c["Nx"] - 1
            on = c["mask"] is None or bool(c["mask"][jj, ii])
            assert list(first.cells[1:]) == [int(on), 0, 0]
            assert first.max_h[1] == (c["h"][jj, ii] if on else -math.inf)
            for k in ("ice_volume", "ice_area", "ice_extent", "region_area"):
                assert all(dref.same_bits(getattr(first, k)[q].item(), 0.0) for q in (2, 3)), k
            assert list(first.min_h[2:]) == [math.inf] * 2 and list(first.max_aice[2:]) == [-math.inf] * 2
    assert m.ctx.regions_stats() == 2 * calls


# ---- against the diagnostics of the same build under the mask AND (ids == r) ---------------------------------------------------------------
@pytest.mark.parametrize("config", ["bb_latlon_land_snow", "pp_uniform", "pb_curvilinear_land"])
@pytest.mark.parametrize("grid", ["block_plus_one", "edges_64"])
def test_region_r_is_the_tracer_group_under_the_mask_and_id_equals_r(grid, config):
    topo, metrics, land, snow = dc.CONFIGS[config]
    c = dc.make(*GRIDS[grid], topo=topo, metrics=metrics, land=land, snow=snow)
    m = dc.build_model(c)
    dc.load(m, c)
    other = dc.build_model(c)
    dc.load(other, c)
    act = np.ones((c["Ny"], c["Nx"]), dtype=bool) if c["mask"] is None else c["mask"]
    all_maps = maps(c["Nx"], c["Ny"])
    for name in ("halves_by_column", "single_cell_and_empty", "ids_that_name_no_region"):
        ids, n = all_maps[name]
        got = m.regional_diagnostics(regions_of(c, ids, n), extent_threshold=dc.THRESHOLD)
        for r in range(n):
            other.set_mask(act & (ids == r))
            d = other.diagnostics("tracers", extent_threshold=dc.THRESHOLD)
            for k, kd in (("ice_volume", "ice_volume"), ("ice_area", "ice_area"), ("ice_extent", "ice_extent"), ("snow_volume", "snow_volume"),
                          ("region_area", "active_area"), ("min_h", "min_h"), ("max_h", "max_h"), ("min_aice", "min_aice"),
                          ("max_aice", "max_aice"), ("max_hs", "max_hs"), ("cells", "active_cells")):
                vec = getattr(got, k)
                assert dref.same_bits(None if vec is None else vec[r].item(), getattr(d, kd)), (name, r, k)


# ---- further cases ---------------------------------------------------------------------------------------------------------------------
def test_halo_elements_of_the_fields_and_of_the_map_change_nothing():
    c = dc.make(*GRIDS["edges_64"], topo=("bounded", "periodic"), metrics="curvilinear", land=True, snow=True)
    m = dc.build_model(c)
    ids, n = maps(c["Nx"], c["Ny"])["ids_that_name_no_region"]
    want, stray = restate(c, ids, n)
    g = m.grid
    results = []
    for field_halo, map_halo in ((np.nan, 0), (1e300, I32.min), (np.nan, 1), (0.0, I32.max)):
        dc.load(m, c, halo=field_halo)
        parent = np.full((g.Ny + 2 * g.Hy, g.Nx + 2 * g.Hx + 3), map_halo, dtype=np.int32)      # (ld wider than the parent needs)
        parent[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx] = ids
        t = torch.from_numpy(parent).to(m.device)
        torch.cuda.synchronize()
        rec, got_stray = m.ctx.regions_compute(t.data_ptr(), parent.shape[1], n, dc.THRESHOLD)
        results.append(([bytes(rec[r]) for r in range(n)], got_stray))
        for r in range(n):
            for k in ref.KEYS:
                assert dref.same_bits(getattr(rec[r], k), want[r][k]), (field_halo, map_halo, r, k)
        assert got_stray == stray
    assert all(x == results[0] for x in results)


def test_negative_zero_fields():
    c = dc.make(*GRIDS["block_plus_one"], topo=("bounded", "periodic"), metrics="uniform", snow=True)
    for k in ("h", "a", "hs"):
        c[k] = np.full_like(c[k], -0.0)
    ids, n = maps(65, 65)["halves_by_row"]
    m = dc.build_model(c)
    dc.load(m, c)
    got = m.regional_diagnostics(regions_of(c, ids, n))
    want, stray = restate(c, ids, n, 0.15)
    assert not ref.compare(got, want, stray), ref.compare(got, want, stray)
    for k in ("ice_volume", "ice_area", "ice_extent", "snow_volume"):
        assert all(dref.same_bits(v.item(), 0.0) for v in getattr(got, k)), k          # +0.0: the sums start from +0.0


def test_concentration_exactly_at_the_threshold_counts():
    c = dc.make(*GRIDS["narrow"], metrics="latlon")
    thr = 0.3
    c["a"][:] = np.nextafter(thr, 0.0)
    c["a"][5, 7] = c["a"][28, 36] = thr                                              # one cell AT the threshold in each half
    ids, n = maps(37, 29)["halves_by_column"]
    _, _, az = dref.metrics_of(c["g"])
    m = dc.build_model(c)
    dc.load(m, c)
    got = m.regional_diagnostics(regions_of(c, ids, n), extent_threshold=thr)
    want, stray = restate(c, ids, n, thr)
    assert not ref.compare(got, want, stray)
    assert list(got.ice_extent) == [az[5, 7], az[28, 36]] and got.extent_threshold == thr
    assert m.regional_diagnostics(regions_of(c, ids, n), extent_threshold=0.0).ice_extent.tobytes() == got.region_area.tobytes()


def test_nan_inside_one_region_stays_there():
    c = dc.make(*GRIDS["edges_64"], topo=("periodic", "periodic"), metrics="latlon", snow=True)
    ids, n = maps(130, 65)["bands_on_block_edges"]
    m = dc.build_model(c)
    dc.load(m, c)
    r = regions_of(c, ids, n)
    clean = m.regional_diagnostics(r)
    c["h"][10, 70] = math.nan                                                        # region 1: columns 65 .. 128, rows 1 .. 64
    assert ids[10, 70] == 1
    dc.load(m, c)
    got = m.regional_diagnostics(r)
    want, stray = restate(c, ids, n, 0.15)
    assert not ref.compare(got, want, stray)
    assert math.isnan(got.ice_volume[1]) and not math.isnan(got.ice_area[1])
    assert got.min_h[1] == np.nanmin(c["h"][ids == 1]) and got.max_h[1] == np.nanmax(c["h"][ids == 1])      # the extrema skip it
    for k in csi.regions.QUANTITIES:
        a, b = getattr(got, k), getattr(clean, k)
        keep = [q for q in range(n) if q != 1]
        assert a[keep].tobytes() == b[keep].tobytes(), k                              # the other regions: the same bits


def test_after_three_rk3_steps_equals_the_restatement_on_the_copied_fields():
    c = cases.make_case(Nx=130, Ny=33, topo=("bounded", "periodic"), land=0.2, random_uv=0.02, substeps=10)
    m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    assert m.ctx.regions_stats() == 0
    for _ in range(3):
        csi.time_step(m, c["dt"])
    assert m.ctx.regions_stats() == 0                                                # a model that never asks makes none of the calls
    ids, n = maps(130, 33)["ids_that_name_no_region"]
    got = m.regional_diagnostics(csi.Regions(m.grid, ids, names=("a", "b", "c")))
    assert m.ctx.regions_stats() == 2
    m.synchronize()
    _, _, az = dref.metrics_of(m.grid)
    want, stray = ref.regions(m.ice_thickness.interior_numpy(), m.ice_concentration.interior_numpy(), None, az, c["mask"], ids, n, 0.15)
    assert not ref.compare(got, want, stray), ref.compare(got, want, stray)
    assert got.ice_volume.min() > 0 and got.has_snow is False and got.unassigned_cells == stray > 0
    assert bits(m.regional_diagnostics(csi.Regions(m.grid, ids, names=("a", "b", "c")))) == bits(got)


def test_argument_errors_by_name():
    c = dc.make(*GRIDS["narrow"])
    m = dc.build_model(c)
    dc.load(m, c)
    g = m.grid
    r = regions_of(c, *maps(37, 29)["halves_by_row"])
    t = r.device_parent(g, m.device)
    ld = t.shape[1]
    for kw, text in ((dict(ids_ptr=0), "ids == NULL"), (dict(n_regions=0), "n_regions must be between 1 and CSI_REGIONS_MAX"),
                     (dict(n_regions=65), "n_regions must be between 1 and CSI_REGIONS_MAX"), (dict(n_regions=-3), "n_regions must be between"),
                     (dict(ld=g.Nx + 2 * g.Hx - 1), "ld < Nx \\+ 2 Hx"), (dict(extent_threshold=-0.1), "extent_threshold must be finite and >= 0"),
                     (dict(extent_threshold=math.nan), "extent_threshold must be finite"), (dict(extent_threshold=math.inf), "extent_threshold must be finite"),
                     (dict(reserved=1), "reserved must be 0")):
        args = dict(ids_ptr=t.data_ptr(), ld=ld, n_regions=2, extent_threshold=0.15, reserved=0)
        args.update(kw)
        with pytest.raises(csi.CsiError, match="regions: " + text) as e:
            m.ctx.regions_compute(**args)
        assert e.value.code == -1, kw
    lib = _L.load()
    reg = _L.Regions(C.c_void_p(t.data_ptr()), ld, 2, 0)
    assert lib.csi_regions_compute(m.ctx.h, C.byref(reg), 0.15, None, None) == -1 and b"out == NULL" in lib.csi_last_error(m.ctx.h)
    out = (_L.RegionRecord * 2)()
    assert lib.csi_regions_compute(m.ctx.h, None, 0.15, out, None) == -1 and b"csi_regions pointer is NULL" in lib.csi_last_error(m.ctx.h)
    assert lib.csi_regions_compute(m.ctx.h, C.byref(reg), 0.15, out, None) == 0      # unassigned_cells may be NULL
    assert m.ctx.regions_stats() == 2
    # a context without fields: what is missing, by name
    ctx = csi.Context(0)
    met = _L.Metrics()
    met.dx = met.dy = 1.0
    ids = torch.zeros((10, 10), dtype=torch.int32, device="cuda:0")
    with pytest.raises(csi.CsiError, match="csi_grid_set has not been called") as e:
        ctx.regions_compute(ids.data_ptr(), 10, 1, 0.15)
    assert e.value.code == -2
    ctx.call("csi_grid_set", 8, 8, 1, 1, _L.PERIODIC, _L.PERIODIC, _L.METRIC_UNIFORM, C.byref(met))
    with pytest.raises(csi.CsiError, match="regions: every call needs field h") as e:
        ctx.regions_compute(ids.data_ptr(), 10, 1, 0.15)
    assert e.value.code == -2
    h = torch.ones((10, 10), dtype=torch.float64, device="cuda:0")
    ctx.call("csi_field_bind", _L.F["H"], C.c_void_p(h.data_ptr()), 10, 10, 10)
    with pytest.raises(csi.CsiError, match="regions: every call needs field aice"):
        ctx.regions_compute(ids.data_ptr(), 10, 1, 0.15)
    a = torch.full((10, 10), 0.5, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.call("csi_field_bind", _L.F["A"], C.c_void_p(a.data_ptr()), 10, 10, 10)
    rec, stray = ctx.regions_compute(ids.data_ptr(), 10, 2, 0.15)
    assert (rec[0].ice_area, rec[0].region_area, rec[0].ice_volume, rec[0].cells, stray) == (32.0, 64.0, 32.0, 64, 0)
    assert math.isnan(rec[0].snow_volume) and math.isnan(rec[0].max_hs) and rec[1].cells == 0 and rec[1].min_h == math.inf
    assert ctx.regions_stats() == 2
    ctx.close()
    # the front end: a map made for another grid
    with pytest.raises(ValueError, match="made for a 64 x 64 grid"):
        m.regional_diagnostics(csi.Regions(csi.RectilinearGrid((64, 64), x=(0, 1), y=(0, 1)), np.zeros((64, 64), dtype=int)))


def test_series_writer_over_five_steps(tmp_path):
    c = cases.make_case(Nx=65, Ny=40, grid="latlon", topo=("periodic", "bounded"), land=0.2, random_uv=0.02, substeps=6)
    m = cases.csi_model(c, mode="fast", timestepper="ForwardEuler", advection=csi.WENO(order=5))
    r = csi.Regions.latitude_bands(m.grid, np.linspace(m.grid.latitude[0], m.grid.latitude[1], 4), names=("low", "mid", "high"))
    m.output_writers["regions"] = csi.RegionalSeriesWriter(r, csi.IterationInterval(2), str(tmp_path / "series"))
    want = [m.regional_diagnostics(r)]
    for _ in range(5):
        csi.time_step(m, c["dt"])
        if m.clock.iteration % 2 == 0:
            want.append(m.regional_diagnostics(r))
    m.output_writers["regions"].close()
    out = csi.load_regional_series(str(tmp_path / "series"))
    assert out["names"] == ("low", "mid", "high") and list(out["iteration"]) == [0, 2, 4] and out["ice_volume"].shape == (3, 3)
    for k in out:
        if k in csi.regions.QUANTITIES:
            assert out[k].tobytes() == np.array([getattr(d, k) for d in want]).tobytes(), k
    assert "snow_volume" not in out and not np.array_equal(out["ice_volume"][0], out["ice_volume"][2])


# ---- tiles ---------------------------------------------------------------------------------------------------------------------------
def tile_ids(Nx, Ny):
    """Four regions whose seams cross every tile seam, and ids that name none"""
    j, i = np.mgrid[0:Ny, 0:Nx]
    ids = ((i * 3 // Nx + j * 5 // Ny) % 4).astype(np.int32)
    ids[::7, ::11] = -1
    ids[3::9, 5::13] = I32.max
    return ids, 4


def _untiled(kw):
    """(the case with the fields of the untiled model after one momentum step, the map, the untiled record, the bound per sum and region)"""
    c = cases.make_case(**kw)
    m = cases.csi_model(c, mode="fast")
    csi.time_step_momentum(m, c["dt"])
    ids, n = tile_ids(c["Nx"], c["Ny"])
    r = csi.Regions(m.grid, ids, names=("a", "b", "c", "d"))
    rec = m.regional_diagnostics(r, extent_threshold=dc.THRESHOLD)
    h, a = m.ice_thickness.interior_numpy(), m.ice_concentration.interior_numpy()
    hs = m.snow_thickness.interior_numpy() if m.snow_thickness is not None else None
    _, _, az = dref.metrics_of(m.grid)
    want, stray = ref.regions(h, a, hs, az, c["mask"], ids, n, dc.THRESHOLD)
    assert not ref.compare(rec, want, stray), ref.compare(rec, want, stray)
    bounds = {}
    for q in range(n):
        _, terms = ref.region_terms(h, a, hs, az, c["mask"], ids, q, dc.THRESHOLD)
        for k, kt in (("ice_volume", "ice_volume"), ("ice_area", "ice_area"), ("ice_extent", "ice_extent"), ("region_area", "active_area")):
            bounds[k, q] = dref.fsum_bound(terms[kt])[1]                             # (n - 1) 2^-53 sum |terms|, n = Nx * Ny
    return r, rec, bounds


def as_plain(d):
    """A RegionalDiagnostics as JSON-able values: doubles as hex"""
    out = {k: (None if getattr(d, k) is None else [float(v).hex() if k != "cells" else int(v) for v in getattr(d, k)]) for k in csi.regions.QUANTITIES}
    out["unassigned_cells"] = d.unassigned_cells
    return out


def _check_tiles(records, untiled, bounds, what):
    for rk, d in enumerate(records):
        assert d == records[0], (what, "rank", rk, "returned other bits than rank 0")
    d, u = records[0], as_plain(untiled)
    assert d["unassigned_cells"] == u["unassigned_cells"] and d["cells"] == u["cells"]
    for k in csi.regions.EXTREMA:
        assert d[k] == u[k], (what, k)
    for (k, q), bound in bounds.items():
        got, want = float.fromhex(d[k][q]), float.fromhex(u[k][q])
        print(what, k, "region", q, "tiled", got, "untiled", want, "difference", got - want, "bound", bound)
        assert abs(got - want) <= bound, (what, k, q, got, want, bound)


def _tile_case(name):
    from test_gpu_local_tiles import DECOMPOSITIONS
    Rx, Ry, kw, _ = DECOMPOSITIONS[name]
    return Rx, Ry, dict(H=8, substeps=14, patches=True, random_uv=0.05, **kw)


@pytest.mark.parametrize("name", ["2x1_bounded_x", "1x2_fold", "2x2_channel_land_arrays"])
def test_tiles_of_one_process_agree_with_each_other_and_with_the_untiled_model(name):
    from test_gpu_local_tiles import run_tile_threads
    Rx, Ry, kw = _tile_case(name)
    regions, untiled, bounds = _untiled(kw)

    def tile(rank, group):
        c = cases.make_case(**kw)
        m = cases.csi_model(c, mode="fast", tile=(Rx, Ry, rank), local_group=group)
        csi.time_step_momentum(m, c["dt"])
        out = as_plain(m.regional_diagnostics(regions, extent_threshold=dc.THRESHOLD))
        assert as_plain(m.regional_diagnostics(regions, extent_threshold=dc.THRESHOLD)) == out
        del m
        return out

    _check_tiles(run_tile_threads(Rx * Ry, tile), untiled, bounds, name)


def _host_rank(conn, shm, kw, Rx, Ry, rank):
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    try:
        import cases as cs
        import climaseaice_jl_amd as csi_
        c = cs.make_case(**kw)
        m = cs.csi_model(c, mode="fast", tile=(Rx, Ry, rank), host_group=shm)
        csi_.time_step_momentum(m, c["dt"])
        ids, _ = tile_ids(c["Nx"], c["Ny"])
        r = csi_.Regions(m.grid, ids, names=("a", "b", "c", "d"))
        conn.send(as_plain(m.regional_diagnostics(r, extent_threshold=dc.THRESHOLD)))
    except Exception as e:      # noqa: BLE001  (reported to the parent, which fails the test)
        conn.send({"error": repr(e)})


def test_two_processes_on_one_gpu_over_the_host_channel_group():
    kw = dict(Nx=150, Ny=128, topo=("bounded", "bounded"), land=0.2, substeps=12, patches=True, random_uv=0.05, H=4)
    Rx, Ry = 1, 2
    _, untiled, bounds = _untiled(kw)
    shm = f"/csi-test-{uuid.uuid4().hex[:12]}"
    ctx = mp.get_context("spawn")
    procs, pipes = [], []
    for r in range(Rx * Ry):
        a, b = ctx.Pipe()
        p = ctx.Process(target=_host_rank, args=(b, shm, kw, Rx, Ry, r))
        p.start()
        procs.append(p); pipes.append(a)
    got = []
    for r in range(Rx * Ry):
        assert pipes[r].poll(300), f"rank {r} did not answer"
        got.append(pipes[r].recv())
    for p in procs:
        p.join(timeout=60)
    for r, d in enumerate(got):
        assert "error" not in d, (r, d.get("error"))
    _check_tiles(got, untiled, bounds, "host-channel group 1x2")


def test_rccl_communicator_of_one_rank():
    """A tile connected to itself over an RCCL communicator of one rank: the all-gather runs, the interior is the whole grid, so every
    member -- the sums included -- equals the untiled model's bit for bit."""
    kw = dict(Nx=130, Ny=64, topo=("periodic", "periodic"), substeps=10, patches=True, random_uv=0.05, H=4)
    regions, untiled, _ = _untiled(kw)
    c = cases.make_case(**kw)
    m = cases.csi_model(c, mode="fast", tile=(1, 1, 0, (True, True)))
    assert m.ctx.comm_count() == 1
    csi.time_step_momentum(m, c["dt"])
    assert as_plain(m.regional_diagnostics(regions, extent_threshold=dc.THRESHOLD)) == as_plain(untiled)


@pytest.mark.skipif(NGPU < 2, reason="needs at least 2 GPUs (one rank per GPU)")
def test_two_devices_over_rccl(tmp_path):
    kw = dict(Nx=256, Ny=192, H=8, substeps=14, topo=("bounded", "periodic"), patches=True, random_uv=0.05, land=0.2)
    _, untiled, bounds = _untiled(kw)
    port = str(29600 + os.getpid() % 90)
    out = str(tmp_path / "regions")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "regions_rank_worker.py"), str(r), "2", port, "2", "1", out,
                               json.dumps(kw), str(dc.THRESHOLD)], env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    got = [json.load(open(f"{out}.rank{r}.json")) for r in range(2)]
    _check_tiles(got, untiled, bounds, "RCCL 2x1 on two devices")
