"""Every layout of the advection kernel k_tendencies (csrc/advect.hip) against the oracle: the three block shapes of the
two-tracers-per-thread layout forced on small grids whose sizes sit on the tile edges (CSI_ADV_NT, CSI_ADV_SHAPE), in the tendency
launch and in the whole-RK-stage launch, with f32 weights, the three-tracer snow layout, and the unforced rule at its own
thresholds.  Every test asserts the layout the library reports (csi_last_advection) against tests/advect_layouts.py before it
compares a number; the comparison is the one of tests/test_gpu_steps.py (STRICT bit for bit, FAST within G_TOL / ADV_TOL with
identical zero sets).  How far the oracle's answer moves under the slips these cases are meant to catch:
scripts/advect_layout_sensitivity.py, profiles/r14_advection_layouts.md."""
import numpy as np
import pytest

import advect_layouts as al
import cases
import climaseaice_jl_amd as csi
from test_gpu_steps import ADV_TOL, G_TOL, same_tendency          # noqa: F401  (G_TOL: used by same_tendency on names starting with G)

pytestmark = pytest.mark.gpu

ADVECTION = {7: csi.WENO(order=7), 5: csi.WENO(order=5), 3: csi.WENO(order=3), -5: csi.UpwindBiased(order=5),
             -3: csi.UpwindBiased(order=3), 1: csi.UpwindBiased(order=1)}
DT = 120.0


def force(monkeypatch, nt=0, shape=0):
    for k, v in al.forced_env(nt, shape).items():
        if v:
            monkeypatch.setenv(k, v)
        else:
            monkeypatch.delenv(k, raising=False)


def layout_of(m):
    p = m.ctx.last_advection()
    return (p["tracers_per_thread"], p["tile_x"], p["tile_y"]), p["stage_fused"]


# ---- inputs and oracle answers: made once per key, shared by every test that needs them, never written to -------------------------
_CASES, _WANT = {}, {}


def forced_case(Nx, Ny, topo, land=None, **kw):
    """topo: a key of advect_layouts.TOPOS or the pair itself.  Halo 4, seeded velocity noise of three times the mean flow (the upwind
    side changes from face to face), land in the bounded box unless `land` says otherwise."""
    land = (0.2 if topo == "bb" else 0.0) if land is None else land
    key = (Nx, Ny, topo, land, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = cases.make_case(Nx=Nx, Ny=Ny, H=4, topo=al.TOPOS.get(topo, topo), substeps=2, random_uv=0.3, patches=True, land=land, **kw)
    return key, _CASES[key]


def frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def oracle_tendencies(key, c, scheme, w32=False):
    k = ("G", key, scheme, w32)
    if k not in _WANT:
        p = cases.oracle_problem(c)
        p.s.weno_weights_f32 = int(w32)
        p.compute_tracer_tendencies(scheme)
        _WANT[k] = frozen({"Gh": p.interior("Gh").copy(), "Ga": p.interior("Ga").copy()})
        assert all(np.abs(v).max() > 0 for v in _WANT[k].values())
    return _WANT[k]


def oracle_rk3(key, c, scheme, n_steps, w32=False):
    """the oracle's stage loop of an advection-only RK3 step (test_advection_only_time_step_bitwise): whole parents, halos included"""
    k = ("rk3", key, scheme, n_steps, w32)
    if k not in _WANT:
        p = cases.oracle_problem(c)
        p.s.weno_weights_f32 = int(w32)
        for _ in range(n_steps):
            p.f["hm"][...] = p.f["h"]; p.f["am"][...] = p.f["aice"]
            for beta in (3, 2, 1):
                p.compute_tracer_tendencies(scheme)
                p.dynamic_step_tracers(DT / beta, True)
                p.update_state()
        _WANT[k] = frozen({n: p.f[n].copy() for n in ("h", "aice", "hm", "am")})
        assert np.abs(p.interior("h") - c["h"]).max() > 1e-6           # the advection did something
    return _WANT[k]


def compare_tendencies(m, mode, want, what):
    for k, f in (("Gh", m.timestepper.Gn.h), ("Ga", m.timestepper.Gn.aice)):
        same_tendency(mode, f.interior_numpy(), want[k], (k,) + what)


def advection_only_model(c, scheme, mode, weight_dtype="f64", fusion=None):
    adv = csi.WENO(order=scheme, weight_dtype=weight_dtype) if weight_dtype == "f32" else ADVECTION[scheme]
    m = csi.SeaIceModel(c["g"], dynamics=None, advection=adv, timestepper="SplitRungeKutta3", mode=mode)
    if fusion is not None:
        m.set_fusion(fusion)
    csi.set_(m, h=c["h"], aice=c["a"], u=c["u"], v=c["v"])
    return m


def state_of(m):
    ts = m.timestepper
    return {"h": m.ice_thickness.numpy().copy(), "aice": m.ice_concentration.numpy().copy(),
            "hm": ts.Psi_minus.h.numpy().copy(), "am": ts.Psi_minus.aice.numpy().copy()}


def compare_state(mode, got, want, n_steps, what):
    """h, aice and Psi^-, whole parents with halos: STRICT bit for bit, FAST n_steps x ADV_TOL (relative on h, absolute on aice <= 1)"""
    for k in ("h", "aice", "hm", "am"):
        assert np.all(np.isfinite(got[k])), (k,) + what
        if mode == "strict":
            assert np.array_equal(got[k], want[k]), (k,) + what + (np.abs(got[k] - want[k]).max(), np.argwhere(got[k] != want[k])[:4])
        else:
            scale = np.abs(want[k]).max() if k in ("h", "hm") else 1.0
            assert np.abs(got[k] - want[k]).max() <= n_steps * ADV_TOL * scale, (k,) + what + (np.abs(got[k] - want[k]).max() / scale,)
            assert np.array_equal(got[k] == 0.0, want[k] == 0.0), (k,) + what + ("zero set",)


# ---- (a) forced shapes on small grids, tendencies ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", al.MODES)
@pytest.mark.parametrize("shape", al.FORCED_SHAPES)
@pytest.mark.parametrize("topo", list(al.TOPOS))
@pytest.mark.parametrize("grid", al.FORCED_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_forced_shapes_tendencies_vs_oracle(grid, topo, shape, mode, oracle_lib, monkeypatch):
    """Two tracers per thread in each block shape on grids that end in a one-column block, in exact multiples of the tile, or below
    one tile's rows: Gh, Ga of all six schemes against the oracle; with land (the bounded box), land poisoned with 1e300 never reaches
    a wet cell."""
    key, c = forced_case(*grid, topo)
    force(monkeypatch, nt=2, shape=shape)
    m = cases.csi_model(c, mode=mode)
    for scheme in al.SCHEMES:
        m.ctx.call("csi_compute_tracer_tendencies", scheme)
        m.synchronize()
        assert layout_of(m) == (al.expected_layout(*grid, nt=2, shape=shape), 0)
        compare_tendencies(m, mode, oracle_tendencies(key, c, scheme), (scheme, grid, topo, shape))
    if c["mask"] is None:
        return
    wet = c["mask"].astype(bool)
    scheme = al.SCHEMES[shape - 1]                      # one scheme per shape: WENO7, WENO5, Upwind5
    m.ctx.call("csi_compute_tracer_tendencies", scheme)
    m.synchronize()
    first = {k: f.interior_numpy().copy() for k, f in (("Gh", m.timestepper.Gn.h), ("Ga", m.timestepper.Gn.aice))}
    for k in first:
        assert np.all(first[k][~wet] == 0.0)
    for fld, fid in ((m.ice_thickness, "H"), (m.ice_concentration, "A")):
        a = fld.interior_numpy().copy()
        a[~wet] = 1e300
        fld.set(a)
        m.ctx.call("csi_fill_halo_local", csi._lib.F[fid])
    m.ctx.call("csi_compute_tracer_tendencies", scheme)
    m.synchronize()
    for k, f in (("Gh", m.timestepper.Gn.h), ("Ga", m.timestepper.Gn.aice)):
        assert np.array_equal(f.interior_numpy()[wet], first[k][wet]), (k, scheme, grid, shape)


@pytest.mark.parametrize("mode", al.MODES)
@pytest.mark.parametrize("shape", al.GEOMETRY_SHAPES)
@pytest.mark.parametrize("name", list(al.GEOMETRY_CASES))
def test_forced_shapes_on_other_geometries_vs_oracle(name, shape, mode, oracle_lib, monkeypatch):
    """The 63-column shapes with per-row metrics (lat-lon channel), per-point metrics (curvilinear) and across a north fold with an
    immersed mask: below 200 000 cells these geometries only ever ran the one-tracer layout."""
    kw = dict(al.GEOMETRY_CASES[name])
    Nx, Ny = kw.pop("Nx"), kw.pop("Ny")
    key, c = forced_case(Nx, Ny, kw.pop("topo"), land=kw.pop("land", 0.0), **kw)
    force(monkeypatch, nt=2, shape=shape)
    m = cases.csi_model(c, mode=mode)
    for scheme in al.SCHEMES:
        m.ctx.call("csi_compute_tracer_tendencies", scheme)
        m.synchronize()
        assert layout_of(m) == (al.expected_layout(Nx, Ny, nt=2, shape=shape), 0)
        compare_tendencies(m, mode, oracle_tendencies(key, c, scheme), (scheme, name, shape))


# ---- (b) f32 weights -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", al.MODES)
@pytest.mark.parametrize("shape", al.FORCED_SHAPES)
@pytest.mark.parametrize("scheme", al.WENO)
def test_forced_shapes_f32_weights_vs_oracle(scheme, shape, mode, oracle_lib, monkeypatch):
    """WENO weights in single precision in every block shape: the tendencies, then one RK3 step of the stage launch, against the
    oracle's f32-weight mode."""
    key, c = forced_case(*al.F32_GRID, al.F32_TOPO, land=0.0)
    force(monkeypatch, nt=2, shape=shape)
    want_layout = al.expected_layout(*al.F32_GRID, nt=2, shape=shape)
    m = cases.csi_model(c, mode=mode, advection=csi.WENO(order=scheme, weight_dtype="f32"))
    m.ctx.call("csi_compute_tracer_tendencies", scheme)
    m.synchronize()
    assert layout_of(m) == (want_layout, 0)
    want = oracle_tendencies(key, c, scheme, w32=True)
    compare_tendencies(m, mode, want, (scheme, "f32 weights", shape))
    assert not np.array_equal(want["Gh"], oracle_tendencies(key, c, scheme)["Gh"])       # the f32 mode is another answer
    m = advection_only_model(c, scheme, mode, weight_dtype="f32")
    csi.time_step(m, DT)
    m.synchronize()
    assert layout_of(m) == (want_layout, 1)
    compare_state(mode, state_of(m), oracle_rk3(key, c, scheme, 1, w32=True), 1, (scheme, "f32 weights", shape))


# ---- (c) stage launches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", al.MODES)
@pytest.mark.parametrize("layout", list(al.STAGE_LAYOUTS))
@pytest.mark.parametrize("topo", al.STAGE_TOPOS)
@pytest.mark.parametrize("grid", al.STAGE_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_stage_launch_vs_oracle(grid, topo, layout, mode, oracle_lib, monkeypatch):
    """A whole RK stage in one launch (k_tendencies<..., STEP>) in every layout: three steps of an advection-only RK3 model against
    the oracle's stage loop -- h, aice and Psi^-, whole parents with halos -- and against the separate kernels (csi_set_fusion(0)),
    bit for bit in both modes."""
    nt, shape = al.STAGE_LAYOUTS[layout]
    key, c = forced_case(*grid, topo, land=0.0)
    force(monkeypatch, nt=nt, shape=shape)
    want_layout = al.expected_layout(*grid, nt=nt, shape=shape)
    n_steps = 3
    for scheme in al.SCHEMES:
        out = {}
        for fusion in (2, 0):
            m = advection_only_model(c, scheme, mode, fusion=fusion)
            for _ in range(n_steps):
                csi.time_step(m, DT)
            m.synchronize()
            assert layout_of(m) == (want_layout, 1 if fusion else 0), (scheme, fusion)
            out[fusion] = state_of(m)
        compare_state(mode, out[2], oracle_rk3(key, c, scheme, n_steps), n_steps, (scheme, grid, topo, layout))
        for k in out[2]:
            assert np.array_equal(out[2][k], out[0][k]), (k, scheme, "one launch per stage against the separate kernels",
                                                          np.abs(out[2][k] - out[0][k]).max())


# ---- (d) the snow layout -------------------------------------------------------------------------------------------------------------
def snow_case(topo):
    key, c = forced_case(*al.SNOW_GRID, topo)
    k = ("hs", key)
    if k not in _CASES:
        rng = np.random.default_rng(41)
        _CASES[k] = np.where(c["a"] > 0, 0.05 + 0.3 * rng.random(c["a"].shape), 0.0)
        _CASES[k].setflags(write=False)
    return key, c, _CASES[k]


def oracle_snow(key, c, hs0, scheme, w32):
    k = ("snow", key, scheme, w32)
    if k not in _WANT:
        p = cases.oracle_problem(c)
        p.s.has_snow = 1
        p.s.weno_weights_f32 = int(w32)
        p.interior("hs")[...] = hs0
        p.update_state()
        p.compute_tracer_tendencies(scheme)
        out = {n: p.interior(n).copy() for n in ("Gh", "Ga", "Ghs")}
        p.dynamic_step_tracers(DT, False)                               # FE form, in place
        out.update({n + " (FE)": p.interior(n).copy() for n in ("h", "aice", "hs")})
        for n, cache in (("h", "hm"), ("aice", "am"), ("hs", "hsm")):
            p.f[cache][...] = p.f[n]
        p.dynamic_step_tracers(DT / 3, True)                            # RK form, from Psi^-
        out.update({n + " (RK)": p.interior(n).copy() for n in ("h", "aice", "hs")})
        _WANT[k] = frozen(out)
    return _WANT[k]


@pytest.mark.parametrize("mode", al.MODES)
@pytest.mark.parametrize("topo", list(al.TOPOS))
def test_snow_layout_vs_oracle(topo, mode, oracle_lib, monkeypatch):
    """Three tracers (h, aice, snow thickness), one per thread, 64 x 4 tiles: Gh, Ga AND Ghs of every scheme (f32 weights for the
    WENO orders too) against the oracle with has_snow, then the tracer update in both forms with hs.  CSI_ADV_NT=2 does not apply."""
    key, c, hs0 = snow_case(topo)
    force(monkeypatch, nt=2, shape=3)
    ice = csi.SlabThermodynamics(top_heat_flux=-80.0, bottom_heat_flux=6.0, bottom_salinity=30.0,
                                 top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    m = cases.csi_model(c, mode=mode, timestepper="SplitRungeKutta3", ice_thermodynamics=ice,
                        snow_thermodynamics=csi.snow_slab_thermodynamics(), snowfall=3e-5)
    fields = dict(h=m.ice_thickness, aice=m.ice_concentration, hs=m.snow_thickness)
    for scheme, w32 in [(s, False) for s in al.SCHEMES] + [(s, True) for s in al.WENO]:
        want = oracle_snow(key, c, hs0, scheme, w32)
        csi.set_(m, h=c["h"], aice=c["a"], hs=hs0.copy())
        m.ctx.call("csi_set_weno_weight_dtype", int(w32))
        m.ctx.call("csi_compute_tracer_tendencies", scheme)
        m.synchronize()
        assert layout_of(m) == (al.expected_layout(*al.SNOW_GRID, has_snow=True, nt=2, shape=3), 0) == ((1, 64, 4), 0)
        for k, f in (("Gh", m.timestepper.Gn.h), ("Ga", m.timestepper.Gn.aice), ("Ghs", m.timestepper.Gn.hs)):
            assert np.abs(want[k]).max() > 0
            same_tendency(mode, f.interior_numpy(), want[k], (k, scheme, w32, topo))
        assert not np.array_equal(want["Ghs"], want["Gh"]) and not np.array_equal(want["Ghs"], want["Ga"])
        m.ctx.call("csi_dynamic_step_tracers", DT, 0)
        m.synchronize()
        for k, f in fields.items():
            same_tendency(mode, f.interior_numpy(), want[k + " (FE)"], (k + " (FE)", scheme, w32, topo))
        if mode == "fast":      # continue from the oracle's state: the update itself is the same code in both modes
            csi.set_(m, **{k: want[k + " (FE)"].copy() for k in fields})
        m.ctx.call("csi_cache_current_fields")
        m.ctx.call("csi_dynamic_step_tracers", DT / 3, 1)
        m.synchronize()
        for k, f in fields.items():
            same_tendency(mode, f.interior_numpy(), want[k + " (RK)"], (k + " (RK)", scheme, w32, topo))


# ---- (e) the rule at its own thresholds, nothing forced ------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(al.THRESHOLD_GRIDS), ids=lambda g: f"{g[0]}x{g[1]}")
def test_unforced_rule_at_its_thresholds(grid, oracle_lib, monkeypatch):
    """One cell row below and exactly at 200 000, 600 000 and 2 500 000 cells, without any knob: the layout the library reports is the
    rule's, and one WENO7 STRICT tendency call equals the oracle bit for bit; at 1000 x 600 and 2500 x 1000 also one advection-only
    RK3 step, one launch per stage (the launch bench.py times at 2048^2)."""
    force(monkeypatch)
    key, c = forced_case(*grid, "pb")
    want_layout = al.expected_layout(*grid)
    m = cases.csi_model(c, mode="strict")
    m.ctx.call("csi_compute_tracer_tendencies", 7)
    m.synchronize()
    assert layout_of(m) == (want_layout, 0)
    compare_tendencies(m, "strict", oracle_tendencies(key, c, 7), (7, grid))
    if al.THRESHOLD_GRIDS[grid]:
        del m
        m = advection_only_model(c, 7, "strict")
        csi.time_step(m, DT)
        m.synchronize()
        assert layout_of(m) == (want_layout, 1)
        compare_state("strict", state_of(m), oracle_rk3(key, c, 7, 1), 1, (7, grid))


def test_shape_knob_is_checked_when_the_context_is_created(monkeypatch):
    for bad in ("4", "-1", "63x7", "2 "):
        monkeypatch.setenv("CSI_ADV_SHAPE", bad)
        with pytest.raises(csi.CsiError) as e:
            csi._lib.Context(0)
        assert "CSI_ADV_SHAPE" in str(e.value)
    monkeypatch.setenv("CSI_ADV_SHAPE", "0")
    ctx = csi._lib.Context(0)
    assert ctx.last_advection() == dict(tracers_per_thread=0, tile_x=0, tile_y=0, stage_fused=0)      # nothing launched yet
    ctx.close()
