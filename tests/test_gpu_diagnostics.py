"""csi_diagnostics_compute (csrc/diagnostics.hip) on the GPU, bit for bit against the NumPy restatement of the documented order
(tests/diagnostics_ref.py): every grid at an edge of the 64 x 64 block layout, both topologies each way (the Face fields' wider rows),
the three metric kinds, land, snow, STRICT and FAST; inputs that locate an indexing error; halo isolation; non-finite values; state and
repetition; tiles over the three things that join ranks; the time-step wizard.  The sums' tolerance on tiles is the issue's:
2 (n - 1) 2^-53 sum |x_i| (both trees lie within the one-sided bound of the exact sum over the same terms)."""
import ctypes as C
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
import diagnostics_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NGPU = torch.cuda.device_count()
ALL = ref.SUMS + ref.EXACT
_L = csi._lib


def restate(c, threshold=dc.THRESHOLD):
    dxfc, dycf, az = ref.metrics_of(c["g"])
    want = ref.velocity_group(c["u"], c["v"], dxfc, dycf)
    want.update(ref.tracer_group(c["h"], c["a"], c["hs"], az, c["mask"], threshold))
    return want


def as_dict(rec):
    d = {k: getattr(rec, k) for k in ref.SUMS + ("inv_timescale_max", "advection_timescale", "max_abs_u", "max_abs_v", "min_h", "max_h",
                                               "min_aice", "max_aice", "max_hs", "active_cells")}
    d.update({"nonfinite_" + k: v for k, v in rec.nonfinite.items()})
    d.update({"nan_" + k: v for k, v in rec.nan.items()})
    return d


def same(a, b):
    return sorted(a) == sorted(b) and all(ref.same_bits(a[k], b[k]) for k in a)


# ---- the layout: every grid x every combination, both modes, both halo fills, twice ------------------------------------------------------
@pytest.mark.parametrize("config", sorted(dc.CONFIGS))
@pytest.mark.parametrize("grid", sorted(dc.GRIDS))
def test_bitwise_against_the_restatement(grid, config):
    topo, metrics, land, snow = dc.CONFIGS[config]
    c = dc.make(*dc.GRIDS[grid], topo=topo, metrics=metrics, land=land, snow=snow)
    want = restate(c)
    m = dc.build_model(c, mode="strict")
    dc.load(m, c, halo=np.nan)
    first = m.diagnostics(extent_threshold=dc.THRESHOLD)
    print(grid, config, {k: (getattr(first, k), want[k]) for k in ref.SUMS})
    assert not ref.compare(first, want, ALL), ref.compare(first, want, ALL)
    assert first.has_snow == snow and first.what == ("velocity", "tracers") and first.finite
    assert first.ice_mass == m.sea_ice_density * first.ice_volume
    again = as_dict(m.diagnostics(extent_threshold=dc.THRESHOLD))
    assert same(again, as_dict(first)), "two calls in a row differ"
    m.set_mode("fast")
    assert same(as_dict(m.diagnostics(extent_threshold=dc.THRESHOLD)), again), "FAST differs from STRICT"
    dc.load(m, c, halo=1e300)
    assert same(as_dict(m.diagnostics(extent_threshold=dc.THRESHOLD)), again), "the halos' contents changed a result"


@pytest.mark.parametrize("low", [False, True])
@pytest.mark.parametrize("where", ["first", "last_column", "last_row"])
@pytest.mark.parametrize("config", ["bb_latlon_land_snow", "pp_curvilinear_snow"])
def test_extremum_in_the_first_cell_the_last_partial_column_and_the_last_row(config, where, low):
    topo, metrics, land, snow = dc.CONFIGS[config]
    c = dc.place_extrema(dc.make(*dc.GRIDS["edges_64"], topo=topo, metrics=metrics, land=land, snow=snow), where, low)
    want = restate(c)
    m = dc.build_model(c)
    dc.load(m, c)
    rec = m.diagnostics()
    assert not ref.compare(rec, want, ALL), ref.compare(rec, want, ALL)
    if low:
        assert (rec.min_h, rec.min_aice) == (-0.75, -0.5)
    else:
        assert (rec.max_abs_u, rec.max_abs_v, rec.max_h, rec.max_aice, rec.max_hs) == (3.0, 2.5, 9.0, 1.5, 4.0)
        j, i = dc.spots(c["Nx"], c["Ny"])[where]
        dxfc, dycf, _ = ref.metrics_of(c["g"])
        assert rec.inv_timescale_max == (3.0 / dxfc[j, i]) + (2.5 / dycf[j, i])      # the velocity extremum's cell is the timescale's


def test_last_faces_of_bounded_directions_enter_the_maxima():
    """u[Nx + 1, j] and v[i, Ny + 1] exist on Bounded directions only: they enter max |u|, max |v| and the counts, no cell's timescale."""
    for grid in ("exact_block", "edges_64"):
        c = dc.make(*dc.GRIDS[grid], topo=("bounded", "bounded"), metrics="latlon")
        c["u"][-1, -1], c["v"][-1, 0] = -7.0, 6.0
        want = restate(c)
        m = dc.build_model(c)
        dc.load(m, c)
        rec = m.diagnostics()
        assert not ref.compare(rec, want, ALL), ref.compare(rec, want, ALL)
        assert (rec.max_abs_u, rec.max_abs_v) == (7.0, 6.0) and rec.inv_timescale_max < 1e-3


def test_negative_zero_fields_and_ice_at_rest():
    c = dc.make(*dc.GRIDS["block_plus_one"], topo=("bounded", "periodic"), metrics="uniform", snow=True)
    for k in ("u", "v", "h", "a", "hs"):
        c[k] = np.full_like(c[k], -0.0)
    want = restate(c)
    m = dc.build_model(c)
    dc.load(m, c)
    rec = m.diagnostics()
    assert not ref.compare(rec, want, ALL), ref.compare(rec, want, ALL)
    assert rec.advection_timescale == math.inf and rec.inv_timescale_max == 0.0
    for k in ("ice_volume", "ice_area", "ice_extent", "snow_volume"):
        assert ref.same_bits(getattr(rec, k), 0.0), k                       # +0.0: the sums start from +0.0
    assert csi.cell_advection_timescale(m) == math.inf


def test_concentration_exactly_at_the_threshold_counts():
    c = dc.make(*dc.GRIDS["narrow"], metrics="latlon")
    thr = 0.3
    c["a"][:] = np.nextafter(thr, 0.0)
    c["a"][5, 7] = c["a"][28, 36] = thr                                     # two cells AT the threshold, every other one a bit below
    _, _, az = ref.metrics_of(c["g"])
    m = dc.build_model(c)
    dc.load(m, c)
    rec = m.diagnostics("tracers", extent_threshold=thr)
    assert not ref.compare(rec, restate(c, thr), ref.SUMS), ref.compare(rec, restate(c, thr), ref.SUMS)
    assert rec.ice_extent == az[5, 7] + az[28, 36] and rec.extent_threshold == thr
    assert m.diagnostics("tracers", extent_threshold=0.0).ice_extent == rec.active_area


# ---- non-finite values ---------------------------------------------------------------------------------------------------------------
def test_nonfinite_values_are_counted_and_turn_the_timescale():
    base = dc.make(*dc.GRIDS["edges_64"], topo=("bounded", "bounded"), metrics="uniform", land=True, snow=True)
    Ny, Nx = base["h"].shape
    land_j, land_i = np.argwhere(~base["mask"])[0]
    m = dc.build_model(base)

    def run(edit):
        c = dict(base, **{k: base[k].copy() for k in ("u", "v", "h", "a", "hs")})
        edit(c)
        dc.load(m, c)
        rec = m.diagnostics()
        want = restate(c)
        assert not ref.compare(rec, want, ALL), ref.compare(rec, want, ALL)
        return rec

    clean = run(lambda c: None)
    assert clean.finite and 0.0 < clean.advection_timescale < math.inf
    csi.assert_finite(m)

    def nan_everywhere(c):
        c["h"][Ny - 1, Nx - 1] = math.nan        # an interior corner
        c["a"][land_j, land_i] = math.inf        # under land: not summed, but counted
        c["hs"][0, 0] = -math.inf
        c["u"][3, Nx] = math.nan                 # the last face of the Bounded x direction
    rec = run(nan_everywhere)
    assert dict(rec.nonfinite) == dict(u=1, v=0, h=1, aice=1, hs=1) and dict(rec.nan) == dict(u=1, v=0)
    assert math.isnan(rec.advection_timescale) and not rec.finite
    assert rec.inv_timescale_max == clean.inv_timescale_max                 # the device maximum skips the NaN
    with pytest.raises(FloatingPointError, match=r"u \(1 element\), h \(1 element\), aice \(1 element\), hs \(1 element\)"):
        csi.assert_finite(m)
    assert math.isnan(csi.TimeStepWizard()(m, 100.0))

    rec = run(lambda c: c["v"].__setitem__((Ny - 1, Nx - 1), -math.inf))     # an infinite velocity at an interior corner
    assert rec.advection_timescale == 0.0 and rec.max_abs_v == math.inf and dict(rec.nonfinite)["v"] == 1 and dict(rec.nan)["v"] == 0
    rec = run(lambda c: c["u"].__setitem__((2, Nx), math.inf))               # ... in the last Bounded face: counted, in no cell's timescale
    assert rec.max_abs_u == math.inf and rec.nonfinite["u"] == 1 and rec.advection_timescale == clean.advection_timescale
    rec = run(lambda c: c["v"].__setitem__((Ny, 4), math.nan))               # NaN in the last Bounded face of v: the timescale is NaN
    assert rec.nan["v"] == 1 and math.isnan(rec.advection_timescale)


# ---- state and repetition ------------------------------------------------------------------------------------------------------------
def test_after_three_rk3_steps_equals_the_restatement_on_the_copied_fields():
    c = cases.make_case(Nx=130, Ny=33, topo=("bounded", "periodic"), land=0.2, random_uv=0.02, substeps=10)
    m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    for _ in range(3):
        csi.time_step(m, c["dt"])
    rec = m.diagnostics()
    want = ref.of_model(m, mask=c["mask"])
    assert not ref.compare(rec, want, ALL), ref.compare(rec, want, ALL)
    assert rec.finite and rec.max_abs_u > 0 and rec.ice_volume > 0 and rec.has_snow is False
    assert same(as_dict(m.diagnostics()), as_dict(rec))


def test_one_group_leaves_the_other_not_computed():
    c = dc.make(*dc.GRIDS["narrow"], snow=False)
    m = dc.build_model(c)
    dc.load(m, c)
    full = m.diagnostics()
    vel, trc = m.diagnostics("velocity"), m.diagnostics("tracers")
    assert vel.what == ("velocity",) and trc.what == ("tracers",)
    for k in ref.SUMS + ("ice_mass", "min_h", "max_h", "min_aice", "max_aice", "max_hs", "active_cells"):
        assert getattr(vel, k) is None, k
    for k in ("advection_timescale", "inv_timescale_max", "max_abs_u", "max_abs_v"):
        assert getattr(trc, k) is None and ref.same_bits(getattr(vel, k), getattr(full, k)), k
    assert dict(vel.nonfinite) == dict(u=0, v=0) and dict(trc.nonfinite) == dict(h=0, aice=0) and dict(trc.nan) == {}
    assert (trc.snow_volume, trc.max_hs) == (None, None) and all(ref.same_bits(getattr(trc, k), getattr(full, k)) for k in ref.SUMS[:3])
    # the C struct's documented "not computed" values
    raw = m.ctx.diagnostics_compute(_L.DIAG_VELOCITY, 0.15)
    assert raw.what == 1 and raw.has_snow == 0 and all(math.isnan(getattr(raw, k)) for k in ("ice_volume", "active_area", "min_h", "max_hs"))
    assert (raw.nonfinite_h, raw.nonfinite_aice, raw.nonfinite_hs, raw.active_cells) == (-1, -1, -1, -1)
    raw = m.ctx.diagnostics_compute(_L.DIAG_TRACERS, 0.15)
    assert math.isnan(raw.advection_timescale) and math.isnan(raw.max_abs_u) and (raw.nonfinite_u, raw.nan_v) == (-1, -1)
    assert math.isnan(raw.snow_volume) and raw.nonfinite_hs == -1 and raw.active_cells == c["Nx"] * c["Ny"]


def test_argument_errors_by_name():
    c = dc.make(*dc.GRIDS["narrow"])
    m = dc.build_model(c)
    for what in (0, 4, 7, -1):
        with pytest.raises(csi.CsiError, match="unknown bit") as e:
            m.ctx.diagnostics_compute(what, 0.15)
        assert e.value.code == -1
    for thr in (-0.1, math.nan, math.inf):
        with pytest.raises(csi.CsiError, match="extent_threshold must be finite and >= 0"):
            m.ctx.diagnostics_compute(3, thr)
    with pytest.raises(ValueError):
        m.diagnostics("momentum")
    # a context without fields: each group names what it needs (a model without velocities supports the tracer group only)
    ctx = csi.Context(0)
    met = _L.Metrics()
    met.dx = met.dy = 1.0
    ctx.call("csi_grid_set", 8, 8, 1, 1, _L.PERIODIC, _L.PERIODIC, _L.METRIC_UNIFORM, C.byref(met))
    with pytest.raises(csi.CsiError, match="velocity group needs field u .*CSI_DIAG_TRACERS only") as e:
        ctx.diagnostics_compute(_L.DIAG_ALL, 0.15)
    assert e.value.code == -2
    with pytest.raises(csi.CsiError, match="tracer group needs field h"):
        ctx.diagnostics_compute(_L.DIAG_TRACERS, 0.15)
    h = torch.zeros((10, 10), dtype=torch.float64, device="cuda:0")
    ctx.call("csi_field_bind", _L.F["H"], C.c_void_p(h.data_ptr()), 10, 10, 10)
    with pytest.raises(csi.CsiError, match="tracer group needs field aice"):
        ctx.diagnostics_compute(_L.DIAG_TRACERS, 0.15)
    a = torch.full((10, 10), 0.5, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.call("csi_field_bind", _L.F["A"], C.c_void_p(a.data_ptr()), 10, 10, 10)
    d = ctx.diagnostics_compute(_L.DIAG_TRACERS, 0.15)
    assert (d.ice_area, d.active_area, d.ice_volume, d.active_cells) == (32.0, 64.0, 0.0, 64)
    ctx.close()


# ---- the wizard ----------------------------------------------------------------------------------------------------------------------
def test_wizard_equals_new_time_step_on_the_restated_timescale():
    c = cases.make_case(Nx=130, Ny=33, grid="latlon", topo=("periodic", "bounded"), random_uv=0.05, substeps=10)
    m = cases.csi_model(c, mode="fast")
    csi.time_step_momentum(m, c["dt"])
    want = ref.of_model(m, what="velocity")["advection_timescale"]
    assert 0.0 < want < math.inf
    assert ref.same_bits(csi.cell_advection_timescale(m), want)
    for wiz, dt in ((csi.TimeStepWizard(), 0.2 * want), (csi.TimeStepWizard(cfl=0.7, max_change=10.0, min_change=0.01), 0.5 * want),
                    (csi.TimeStepWizard(max_dt=1.0), 100.0), (csi.TimeStepWizard(), 1e-3 * want), (csi.TimeStepWizard(), 1e3 * want)):
        assert ref.same_bits(wiz(m, dt), csi.new_time_step(dt, want, wiz)), (wiz, dt)


# ---- tiles ---------------------------------------------------------------------------------------------------------------------------
def _sum_bounds(c):
    """per sum: 2 (n - 1) 2^-53 sum |x_i| over the untiled grid's terms"""
    _, _, az = ref.metrics_of(c["g"])
    _, terms = ref.tracer_terms(c["h"], c["a"], None, az, c["mask"], dc.THRESHOLD)
    return {k: 2.0 * ref.fsum_bound(t)[1] for k, t in terms.items()}


def _check_tiles(records, untiled, bounds, what):
    for r, d in enumerate(records):
        assert same(d, records[0]), (what, "rank", r, "returned other bits than rank 0")
    d = records[0]
    for k in d:
        if k in ref.SUMS:
            if untiled[k] is not None:
                print(what, k, "tiled", d[k], "untiled", untiled[k], "difference", d[k] - untiled[k], "bound", bounds[k])
                assert abs(d[k] - untiled[k]) <= bounds[k], (what, k, d[k], untiled[k], bounds[k])
        else:
            assert ref.same_bits(d[k], untiled[k]), (what, k, d[k], untiled[k])


def _tile_case(name):
    from test_gpu_local_tiles import DECOMPOSITIONS
    Rx, Ry, kw, _ = DECOMPOSITIONS[name]
    return Rx, Ry, dict(H=8, substeps=14, patches=True, random_uv=0.05, **kw)


def _untiled(kw):
    """(case with its fields after one momentum step, the untiled model's record)"""
    c = cases.make_case(**kw)
    m = cases.csi_model(c, mode="fast")
    csi.time_step_momentum(m, c["dt"])
    rec = as_dict(m.diagnostics(extent_threshold=dc.THRESHOLD))
    assert not ref.compare(m.diagnostics(extent_threshold=dc.THRESHOLD), ref.of_model(m, mask=c["mask"], threshold=dc.THRESHOLD), ALL)
    c = dict(c, h=m.ice_thickness.interior_numpy(), a=m.ice_concentration.interior_numpy())
    return c, rec


@pytest.mark.parametrize("name", ["2x1_bounded_x", "1x2_fold", "2x2_channel_land_arrays"])
def test_tiles_of_one_process_agree_with_each_other_and_with_the_untiled_model(name):
    from test_gpu_local_tiles import run_tile_threads
    Rx, Ry, kw = _tile_case(name)
    c, untiled = _untiled(kw)

    def tile(rank, group):
        m = cases.csi_model(cases.make_case(**kw), mode="fast", tile=(Rx, Ry, rank), local_group=group)
        csi.time_step_momentum(m, c["dt"])
        out = as_dict(m.diagnostics(extent_threshold=dc.THRESHOLD))
        vel = m.diagnostics("velocity")
        assert ref.same_bits(vel.advection_timescale, out["advection_timescale"])
        del m
        return out

    _check_tiles(run_tile_threads(Rx * Ry, tile), untiled, _sum_bounds(c), name)


def _host_rank(conn, shm, kw, Rx, Ry, rank):
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    try:
        import cases as cs
        import climaseaice_jl_amd as csi_
        c = cs.make_case(**kw)
        m = cs.csi_model(c, mode="fast", tile=(Rx, Ry, rank), host_group=shm)
        csi_.time_step_momentum(m, c["dt"])
        conn.send(as_dict(m.diagnostics(extent_threshold=dc.THRESHOLD)))
    except Exception as e:      # noqa: BLE001  (reported to the parent, which fails the test)
        conn.send({"error": repr(e)})


def test_two_processes_on_one_gpu_over_the_host_channel_group():
    kw = dict(Nx=150, Ny=128, topo=("bounded", "bounded"), land=0.2, substeps=12, patches=True, random_uv=0.05, H=4)
    Rx, Ry = 1, 2
    c, untiled = _untiled(kw)
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
    _check_tiles(got, untiled, _sum_bounds(c), "host-channel group 1x2")


def test_rccl_communicator_of_one_rank():
    """A tile connected to itself over an RCCL communicator of one rank: the all-gather runs (ncclAllGather), the interior is the whole
    grid, so every member -- the sums included -- equals the untiled model's bit for bit."""
    kw = dict(Nx=130, Ny=64, topo=("periodic", "periodic"), substeps=10, patches=True, random_uv=0.05, H=4)
    c, untiled = _untiled(kw)
    m = cases.csi_model(cases.make_case(**kw), mode="fast", tile=(1, 1, 0, (True, True)))
    assert m.ctx.comm_count() == 1
    csi.time_step_momentum(m, c["dt"])
    assert same(as_dict(m.diagnostics(extent_threshold=dc.THRESHOLD)), untiled)


@pytest.mark.skipif(NGPU < 2, reason="needs at least 2 GPUs (one rank per GPU)")
def test_two_devices_over_rccl(tmp_path):
    import json
    kw = dict(Nx=256, Ny=192, H=8, substeps=14, topo=("bounded", "periodic"), patches=True, random_uv=0.05, land=0.2)
    c, untiled = _untiled(kw)
    port = str(29500 + os.getpid() % 90)
    out = str(tmp_path / "diag")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "diagnostics_rank_worker.py"), str(r), "2", port, "2", "1", out,
                               json.dumps(kw), str(dc.THRESHOLD)], env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    got = []
    for r in range(2):
        raw = json.load(open(f"{out}.rank{r}.json"))
        got.append({k: (None if v is None else int(v) if isinstance(untiled[k], int) else float.fromhex(v)) for k, v in raw.items()})
    _check_tiles(got, untiled, _sum_bounds(c), "RCCL 2x1 on two devices")
