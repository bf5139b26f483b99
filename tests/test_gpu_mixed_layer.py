"""The slab-ocean mixed layer on the GPU (csrc/mixed_layer.hip, csi_mixed_layer_set) against the NumPy restatement
tests/mixed_layer_ref.py, bit for bit, in STRICT and FAST mode (the arithmetic is the same in both).  Shapes for the 128 x 8 points of
a block, two points per thread: 37 x 29, 64 x 4, 65 x 5, 130 x 9."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import mixed_layer_ref as M
import thermo_linear_ref as T
import time_series_ref as tsref
from test_gpu_local_tiles import run_tile_threads

pytestmark = pytest.mark.gpu

L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 600.0
DEPTH = 10.0
H = 3
SHAPES = [(37, 29), (64, 4), (65, 5), (130, 9)]
CONFIGS = ["numbers", "surface", "bulk", "deep", "salinity", "all"]


def grid(Nx, Ny):
    return csi.RectilinearGrid((Nx, Ny), x=(0, 1), y=(0, 1), halo=(H, H))


def state(Nx, Ny, seed):
    """Random cells around freezing with thick ice over part of them (mixed_layer_ref.random_state, shaped)."""
    s = M.random_state(Nx * Ny, seed)
    out = {k: (v.reshape(Ny, Nx) if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    rng = np.random.default_rng(seed + 1000)
    out["S"] = 25.0 + 10.0 * rng.random((Ny, Nx))
    out["h"] = np.where(out["a"] > 0, 1.0 + rng.random((Ny, Nx)), 0.0)
    return out


def inputs_of(st, config):
    """(keyword arguments of SlabOceanMixedLayer, keyword arguments of mixed_layer_ref.step, bottom salinity) of a configuration:
    numbers only, one array alone, or every array with a per-cell salinity."""
    Fo = st["Fo"] if config in ("surface", "all") else -35.0
    Qd = st["Qd"] if config in ("deep", "all") else 3.5
    K, Ta = (st["K"], st["Ta"]) if config in ("bulk", "all") else (17.5, -6.25)
    S = st["S"] if config in ("salinity", "all") else 30.0
    return (dict(surface_heat_flux=Fo, coefficient=K, atmosphere_temperature=Ta, deep_heat_flux=Qd),
            dict(Fo=Fo, K=K, Ta=Ta, Qd=Qd, Sb=S), S)


def ocean_model(g, mode, okw, S, To, stepper="ForwardEuler", snow=False, top=-40.0, depth=DEPTH, gamma=M.GAMMA, **kw):
    ocean = csi.SlabOceanMixedLayer(depth, temperature=To, ice_ocean_exchange_velocity=gamma, **okw)
    ice = csi.SlabThermodynamics(bottom_salinity=S, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    if snow:
        kw.update(snow_thermodynamics=csi.snow_slab_thermodynamics(), snowfall=3e-5)
    return csi.SeaIceModel(g, ice_thermodynamics=ice, timestepper=stepper, mode=mode, top_heat_flux=top, ocean=ocean, **kw)


def ocean_fields(m):
    return dict(To=m.ocean.temperature, Qb=m.ocean.bottom_heat_flux, Qow=m.ocean.surface_flux_used)


def same(m, r, what):
    m.synchronize()
    for k, f in ocean_fields(m).items():
        got = f.interior_numpy()
        assert np.all(np.isfinite(got)), (what, k)
        assert np.array_equal(got, r[k]), (what, k, np.abs(got - r[k]).max(), int((got != r[k]).sum()))


# ---- the stand-alone step ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_standalone_step_matches_restatement(mode):
    """csi_mixed_layer_step alone: numbers only, each array alone and every array with a per-cell salinity, the shapes taken in turn
    (every array on every shape); To', Qb and Qow equal the restatement, and a second step from the first one's To' does too."""
    runs = [(c, SHAPES[k % 4]) for k, c in enumerate(CONFIGS)] + [("all", s) for s in SHAPES[:3]]
    for k, (config, (Nx, Ny)) in enumerate(runs):
        st = state(Nx, Ny, 10 + k)
        okw, rkw, S = inputs_of(st, config)
        m = ocean_model(grid(Nx, Ny), mode, okw, S, st["To"])
        m.ocean.surface_flux_used
        csi.set_(m, h=st["h"], aice=st["a"])
        before = m.ctx.mixed_layer_stats()
        To = st["To"]
        for n in range(2):
            m.ctx.mixed_layer_step(DT, False)
            r = M.step(To, st["a"], DT, DEPTH, **rkw)
            same(m, r, (config, (Nx, Ny), n))
            To = r["To"]
        assert m.ctx.mixed_layer_stats() == before + 2
        assert (r["Qfr"] < 0).any() and (r["Qio"] > 0).any()
        flags = m.ocean.params().flags
        assert bool(flags & L.ML_SURFACE_ARRAY) == (config in ("surface", "all")) and bool(flags & L.ML_BULK_ARRAYS) == (config in ("bulk", "all"))
        assert bool(flags & L.ML_DEEP_ARRAY) == (config in ("deep", "all")) and (m.bottom_salinity is not None) == (config in ("salinity", "all"))


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_absent_terms(mode):
    """Fo alone, the bulk term alone, neither: Qs is the term that exists, or 0."""
    Nx, Ny = 65, 5
    st = state(Nx, Ny, 31)
    for okw, rkw in ((dict(surface_heat_flux=st["Fo"]), dict(Fo=st["Fo"])), (dict(coefficient=9.0, atmosphere_temperature=st["Ta"]), dict(K=9.0, Ta=st["Ta"])),
                     (dict(surface_heat_flux=12.0), dict(Fo=12.0)), ({}, {})):
        m = ocean_model(grid(Nx, Ny), mode, okw, 30.0, st["To"])
        m.ocean.surface_flux_used
        csi.set_(m, h=st["h"], aice=st["a"])
        m.ctx.mixed_layer_step(DT, False)
        same(m, M.step(st["To"], st["a"], DT, DEPTH, Sb=30.0, **rkw), sorted(okw))


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_every_branch(mode):
    """The branch-covering state (gamma dt >= depth): the counts first, then the bits."""
    for Nx, Ny in SHAPES:
        inp, kw = M.branch_state((Ny, Nx))
        r = M.step(inp["To"], inp["a"], Fo=inp["Fo"], **kw)
        n = M.branch_counts(inp["To"], inp["a"], r, kw["dt"], kw["gamma"])
        assert all(n[b] >= 6 for b in M.BRANCHES), n
        m = ocean_model(grid(Nx, Ny), mode, dict(surface_heat_flux=inp["Fo"]), kw["Sb"], inp["To"], depth=kw["depth"], gamma=kw["gamma"])
        m.ocean.surface_flux_used
        csi.set_(m, h=np.where(inp["a"] > 0, 1.0, 0.0), aice=inp["a"])
        m.ctx.mixed_layer_step(kw["dt"], False)
        same(m, r, ("branches", Nx, Ny))


def test_from_cache_reads_the_cached_temperature():
    """from_cache = 1: To' is computed from the Psi^- copy whatever To holds; without the copy bound it is refused by name."""
    Nx, Ny = 130, 9
    st = state(Nx, Ny, 41)
    okw, rkw, S = inputs_of(st, "all")
    m = ocean_model(grid(Nx, Ny), "fast", okw, S, st["To"] + 5.0, stepper="SplitRungeKutta3")
    m.ocean.surface_flux_used
    csi.set_(m, h=st["h"], aice=st["a"])
    m.ocean.temperature_minus.set(st["To"])
    for dt in (DT / 3, DT / 2, DT):
        m.ctx.mixed_layer_step(dt, True)
        same(m, M.step(st["To"], st["a"], dt, DEPTH, **rkw), ("from_cache", dt))
    assert np.array_equal(m.ocean.temperature_minus.interior_numpy(), st["To"])
    fe = ocean_model(grid(Nx, Ny), "fast", okw, S, st["To"])
    with pytest.raises(csi.CsiError, match="ocean_temperature-"):
        fe.ctx.mixed_layer_step(DT, True)


def test_halos_are_neither_read_nor_written():
    """NaN and 1e300 in every halo -- To, aice, the four inputs, the salinity, and the two outputs --: interior results unchanged, halos
    untouched."""
    Nx, Ny = 37, 29
    st = state(Nx, Ny, 51)
    out = []
    for poison in (None, np.nan, 1e300):
        g = grid(Nx, Ny)
        flds = {k: csi.CenterField(g, "cuda:0", k) for k in ("Fo", "K", "Ta", "Qd", "S")}
        for k, f in flds.items():
            if poison is not None:
                f.fill_parent(poison)
            f.set(st[k])
        m = ocean_model(g, "fast", dict(surface_heat_flux=flds["Fo"], coefficient=flds["K"], atmosphere_temperature=flds["Ta"],
                                        deep_heat_flux=flds["Qd"]), flds["S"], st["To"])
        outs = (m.ocean.temperature, m.ocean.bottom_heat_flux, m.ocean.surface_flux_used)
        csi.set_(m, h=st["h"], aice=st["a"])
        if poison is not None:
            for f in outs + (m.ice_concentration,):
                keep = f.interior_numpy().copy()
                f.fill_parent(poison)
                f.set(keep)
        m.synchronize()
        m.ctx.mixed_layer_step(DT, False)
        m.synchronize()
        out.append({k: f.interior_numpy().copy() for k, f in ocean_fields(m).items()})
        if poison is not None:
            for f in outs:
                full = f.numpy().copy()
                full[H:H + Ny, H:H + Nx] = poison
                assert np.all(np.isnan(full)) if np.isnan(poison) else np.all(full == poison)
    r = M.step(st["To"], st["a"], DT, DEPTH, Fo=st["Fo"], K=st["K"], Ta=st["Ta"], Qd=st["Qd"], Sb=st["S"])
    for got in out:
        for k in got:
            assert np.array_equal(got[k], r[k]), k


# ---- coupled to the ice step ------------------------------------------------------------------------------------------------------------

def coupled_reference(st, snow, rkw, S, nsteps, top):
    """The restatement's chain: mixed layer, then the ice step with [Qb] as its bottom flux.  Returns the last dicts and the budget's
    largest share of its bound."""
    h, a, hs, Tu, To = st["h"], st["a"], st.get("hs", np.zeros_like(st["h"])), np.zeros_like(st["h"]), st["To"]
    share = 0.0
    for n in range(nsteps):
        o = M.step(To, a, DT, DEPTH, **rkw)
        share = max(share, (M.budget_residual(To, o, DT, rkw.get("Qd", 0.0)) / M.budget_bound(To, o, DT, rkw.get("Qd", 0.0))).max())
        if snow:
            r = T.layered_step(h, a, hs, Tu, DT, [top], [o["Qb"]], 3e-5, S=S)
            h, a, hs, Tu = r["h"], r["aice"], r["hs"], r["tu_snow"]
        else:
            r = T.slab_step(h, a, Tu, DT, [top], [o["Qb"]], S=S)
            h, a, Tu = r["h"], r["aice"], r["Tu"]
        To = o["To"]
    return o, r, share


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_coupled_to_the_ice_step(snow, mode):
    """Three thermodynamic steps of a column model (time_step's column path): h, aice, hs, To, surface_flux_used and
    heat_fluxes_used.bottom (= Qb) equal the restatement's chain; the per-cell budget formed from the DEVICE's own fields holds within
    the CPU test's bound."""
    Nx, Ny = 65, 5
    st = state(Nx, Ny, 61)
    st["hs"] = np.where(st["a"] > 0, 0.1, 0.0)
    okw, rkw, S = inputs_of(st, "all")
    m = ocean_model(grid(Nx, Ny), mode, okw, S, st["To"], snow=snow)
    used, qow = m.heat_fluxes_used, m.ocean.surface_flux_used
    csi.set_(m, h=st["h"], aice=st["a"], **(dict(hs=st["hs"]) if snow else {}))
    for n in range(3):
        m.synchronize()
        To0 = m.ocean.temperature.interior_numpy().copy()
        csi.time_step(m, DT)
    o, r, share = coupled_reference(st, snow, rkw, S, 3, -40.0)
    same(m, o, ("coupled", snow))
    assert np.array_equal(used.bottom.interior_numpy(), o["Qb"]) and np.array_equal(m.ice_thickness.interior_numpy(), r["h"])
    assert np.array_equal(m.ice_concentration.interior_numpy(), r["aice"])
    if snow:
        assert np.array_equal(m.snow_thickness.interior_numpy(), r["hs"])
    assert np.abs(r["h"] - st["h"]).max() > 1e-5 and (o["Qb"] != 0).any()
    # the budget from the device's own fields: C (To' - To) / dt = Qd - Qow - Qb
    dev = dict(o, To=m.ocean.temperature.interior_numpy(), Qb=used.bottom.interior_numpy(), Qow=qow.interior_numpy())
    res, bound = M.budget_residual(To0, dev, DT, st["Qd"]), M.budget_bound(To0, dev, DT, st["Qd"])
    print(f"device budget snow={snow} mode={mode}: largest share of the bound {(res / bound).max():.3f} (restatement {share:.3f})")
    assert np.all(res <= bound)
    assert {"ocean.temperature", "ocean.surface_flux_used", "ocean.surface_heat_flux", "bottom_heat_flux"} <= set(csi.bound_fields(m))


@pytest.mark.parametrize("snow", [False, True], ids=["bare", "snowy"])
def test_freezing_of_a_lake_columns(snow):
    """examples/freezing_of_a_lake.py's four columns after 50 steps of 10 minutes against the restatement (the 2 880 steps stay in the
    example)."""
    spec = importlib.util.spec_from_file_location("freezing_of_a_lake", os.path.join(ROOT, "examples", "freezing_of_a_lake.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    m = ex.build(snow=snow)
    for n in range(50):
        csi.time_step(m, 600.0)
    got = ex.columns(m)
    K = ((1e-3 * 1.225) * 1004) * 5
    Ta = ex.ATMOSPHERE_TEMPERATURE.astype(np.float64)
    h = a = hs = Tu = np.zeros((1, 4))
    To = np.ones((1, 4))
    for n in range(50):
        o = M.step(To, a, 600.0, 10.0, K=K, Ta=Ta, rho=1000.0, c=4000.0, gamma=0.0)
        top = [T.Linear(np.full((1, 4), K), Ta, "ice_present")]
        if snow:
            r = T.layered_step(h, a, hs, Tu, 600.0, top, [o["Qb"]], ex.SNOWFALL)
            h, a, hs, Tu = r["h"], r["aice"], r["hs"], r["tu_snow"]
        else:
            r = T.slab_step(h, a, Tu, 600.0, top, [o["Qb"]])
            h, a, Tu = r["h"], r["aice"], r["Tu"]
        To = o["To"]
    want = [h[0], a[0], Tu[0], To[0]] + ([hs[0]] if snow else [])
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y), (snow, k, x, y)
    assert np.all(got[3] < 1.0) and np.unique(got[3]).size >= 3          # the lake cools, each column at its own rate


# ---- whole steps --------------------------------------------------------------------------------------------------------------------

def _whole_case():
    return cases.make_case(Nx=37, Ny=29, substeps=8, topo=("periodic", "bounded"), patches=True, random_uv=0.02)


@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
def test_whole_steps_against_the_entry_points_driven_by_hand(stepper):
    """FE and RK3 steps with EVP dynamics and WENO7 at 37 x 29: the model with `ocean` against a model WITHOUT one whose stages are
    driven through the existing entry points, the restatement writing its bottom heat-flux array between the tracer update and the
    thermodynamic step of every stage.  After an RK3 step To equals ONE restated step of the whole dt from Psi^-."""
    c = _whole_case()
    Ny, Nx = c["a"].shape
    st = state(Nx, Ny, 71)
    okw, rkw, S = inputs_of(st, "all")
    rk = stepper == "SplitRungeKutta3"

    def build(ocean):
        ice = csi.SlabThermodynamics(bottom_salinity=S, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        kw = dict(ocean=csi.SlabOceanMixedLayer(DEPTH, temperature=st["To"], **okw)) if ocean else dict(bottom_heat_flux=np.zeros((Ny, Nx)))
        return cases.csi_model(c, mode="fast", timestepper=stepper, advection=csi.WENO(order=7), ice_thermodynamics=ice, top_heat_flux=-40.0, **kw)

    A, B = build(True), build(False)
    assert B.ctx.mixed_layer_stats() == 0
    To = st["To"]
    dt, sub, scheme = c["dt"], c["substeps"], 7
    for n in range(2):
        csi.time_step(A, dt)
        # B: the same step through the stage's entry points
        if rk:
            B.ctx.call("csi_cache_current_fields")
        elif n == 0:
            B.ctx.call("csi_update_state")
        for beta in ((3, 2, 1) if rk else (1,)):
            dtau = dt / beta
            B.ctx.call("csi_compute_tracer_tendencies", scheme)
            B.ctx.call("csi_time_step_momentum", dtau, sub, int(rk))
            B.ctx.call("csi_dynamic_step_tracers", dtau, int(rk))
            B.synchronize()
            o = M.step(To, B.ice_concentration.interior_numpy(), dtau, DEPTH, **rkw)      # (RK3: every stage from Psi^- = To)
            B.external_heat_fluxes.bottom.set(o["Qb"])
            B.synchronize()
            B.ctx.call("csi_slab_thermo_step", C.byref(B._slab_params), dtau)
            B.ctx.call("csi_update_state")
        B.clock.time += dt
        B.clock.iteration += 1
        To = o["To"]                      # (the last stage: one step of the whole dt)
        A.synchronize(); B.synchronize()
        assert np.array_equal(A.ocean.temperature.interior_numpy(), To), (stepper, n)
        for name, fa, fb in (("h", A.ice_thickness, B.ice_thickness), ("aice", A.ice_concentration, B.ice_concentration),
                             ("u", A.velocities.u, B.velocities.u), ("v", A.velocities.v, B.velocities.v),
                             ("Qb", A.ocean.bottom_heat_flux, B.external_heat_fluxes.bottom)):
            x, y = fa.interior_numpy(), fb.interior_numpy()
            assert np.all(np.isfinite(x)) and np.array_equal(x, y), (stepper, n, name, np.abs(x - y).max())
    assert A.ctx.mixed_layer_stats() == (6 if rk else 2) and B.ctx.mixed_layer_stats() == 0
    assert np.abs(A.ice_thickness.interior_numpy() - c["h"]).max() > 1e-6 and (o["Qb"] != 0).any()


def test_a_model_without_ocean_is_the_model_of_before():
    """No csi_mixed_layer_set: no launch of the kernel, and the results of a context that never heard of it -- a model with the same
    bottom heat-flux ARRAY, once untouched and once after a mixed layer was set and removed again."""
    c = _whole_case()
    Ny, Nx = c["a"].shape
    st = state(Nx, Ny, 81)
    out = []
    for toggled in (False, True):
        ice = csi.SlabThermodynamics(bottom_salinity=30.0, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), ice_thermodynamics=ice,
                            top_heat_flux=-40.0, bottom_heat_flux=0.1 * st["Qd"])
        if toggled:
            p = csi.SlabOceanMixedLayer(DEPTH).params()
            m.ctx.call("csi_mixed_layer_set", C.byref(p))
            m.ctx.call("csi_mixed_layer_set", None)
        for n in range(2):
            csi.time_step(m, c["dt"])
        m.synchronize()
        assert m.ctx.mixed_layer_stats() == 0 and m.ocean is None
        out.append([f.numpy().copy() for f in (m.ice_thickness, m.ice_concentration, m.velocities.u, m.velocities.v)])
    for x, y in zip(*out):
        assert np.array_equal(x, y)


# ---- series, state, output, tiles ---------------------------------------------------------------------------------------------------

def test_series_drive_the_surface_flux_and_the_air_temperature():
    """Fo by a DEVICE series (Clamp) and Ta by a HOST series with a window of two (Linear): equal to a run whose two fields are set by
    hand from tests/time_series_ref.py before every step; the model's series-driven slots are exactly these two."""
    Nx, Ny = 65, 5
    st = state(Nx, Ny, 91)
    g = grid(Nx, Ny)
    rng = np.random.default_rng(92)
    times = np.array([0.0, 700.0, 1500.0, 2600.0])
    data = dict(Fo=st["Fo"] + 30.0 * rng.standard_normal((4, Ny, Nx)), Ta=st["Ta"] + 6.0 * rng.standard_normal((4, Ny, Nx)))
    index = dict(Fo=(csi.Clamp(), L.TIME_CLAMP, 0.0, None), Ta=(csi.Linear(), L.TIME_LINEAR, 0.0, 2))
    models = []
    for series in (True, False):
        v = {k: csi.FieldTimeSeries(g, (csi.Center, csi.Center), times, data[k], time_indexing=index[k][0], backend=csi.InMemory(index[k][3]))
             if series else data[k][0].copy() for k in data}
        m = ocean_model(g, "strict", dict(surface_heat_flux=v["Fo"], coefficient=11.0, atmosphere_temperature=v["Ta"], deep_heat_flux=2.0),
                        30.0, st["To"])
        csi.set_(m, h=st["h"], aice=st["a"])
        models.append(m)
    A, B = models
    assert sorted(A._series) == ["ML_REFERENCE_TEMPERATURE", "ML_SURFACE_HEAT_FLUX"] and not B._series
    targets = dict(Fo="surface_heat_flux", Ta="atmosphere_temperature")
    for n in range(5):
        t = B.clock.time
        B.synchronize()
        for k in data:
            B.ocean.fields[targets[k]].set(tsref.at(times, data[k], index[k][1], index[k][2], t))
        csi.time_step(A, DT); csi.time_step(B, DT)
        A.synchronize(); B.synchronize()
        for k in data:
            assert np.array_equal(A.ocean.fields[targets[k]].interior_numpy(), B.ocean.fields[targets[k]].interior_numpy()), (n, k)
        for name, fa, fb in (("To", A.ocean.temperature, B.ocean.temperature), ("Qb", A.ocean.bottom_heat_flux, B.ocean.bottom_heat_flux),
                             ("h", A.ice_thickness, B.ice_thickness)):
            assert np.array_equal(fa.interior_numpy(), fb.interior_numpy()), (n, name)
    assert np.abs(A.ocean.temperature.interior_numpy() - st["To"]).max() > 1e-4


def test_checkpoint_round_trip_carries_the_ocean_temperature():
    Nx, Ny = 64, 4
    st = state(Nx, Ny, 101)
    okw, rkw, S = inputs_of(st, "all")
    c = cases.make_case(Nx=Nx, Ny=Ny, substeps=4, topo=("periodic", "periodic"), patches=True, random_uv=0.02)

    def build():
        ice = csi.SlabThermodynamics(bottom_salinity=S, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        return cases.csi_model(c, mode="strict", timestepper="SplitRungeKutta3", advection=csi.WENO(order=5), ice_thermodynamics=ice,
                               top_heat_flux=-40.0, ocean=csi.SlabOceanMixedLayer(DEPTH, temperature=st["To"], **okw))

    m = build()
    for n in range(2):
        csi.time_step(m, c["dt"])
    saved = csi.prognostic_state(m)
    assert {"ocean.temperature", "ocean.temperature_minus"} <= set(saved)
    for n in range(2):
        csi.time_step(m, c["dt"])
    first = csi.prognostic_state(m)
    m2 = build()
    csi.restore_prognostic_state(m2, saved)
    for n in range(2):
        csi.time_step(m2, c["dt"])
    second = csi.prognostic_state(m2)
    for k in first:
        if k != "clock":
            assert np.array_equal(first[k], second[k]), k
    assert not np.array_equal(first["ocean.temperature"], saved["ocean.temperature"])


def test_output_writer_takes_the_ocean_fields_by_name(tmp_path):
    Nx, Ny = 37, 29
    st = state(Nx, Ny, 111)
    okw, rkw, S = inputs_of(st, "all")
    m = ocean_model(grid(Nx, Ny), "fast", okw, S, st["To"])
    assert "ocean.surface_flux_used" not in csi.bound_fields(m)
    csi.set_(m, h=st["h"], aice=st["a"])
    m.output_writers["o"] = csi.OutputWriter(m, ["ocean.temperature", "ocean.surface_flux_used", "bottom_heat_flux"], csi.IterationInterval(1),
                                             str(tmp_path / "o"), dtype="f64")
    for n in range(2):
        csi.time_step(m, DT)
    m.output_writers["o"].close()
    got = csi.load_output(str(tmp_path / "o"))
    o, r, _ = coupled_reference(st, False, rkw, S, 2, -40.0)
    assert list(got["iteration"]) == [0, 1, 2] and np.array_equal(got["ocean.temperature"][0], st["To"])
    assert np.array_equal(got["ocean.temperature"][2], o["To"]) and np.array_equal(got["ocean.surface_flux_used"][2], o["Qow"])
    assert np.array_equal(got["bottom_heat_flux"][2], o["Qb"])


def test_tiled_step_equals_untiled():
    """An RK3 step with EVP, WENO7 and the mixed layer with every array on a 1 x 2 in-process tile group equals the untiled step: the
    layer is rank-local."""
    c = cases.make_case(Nx=64, Ny=48, H=8, substeps=8, topo=("periodic", "periodic"), patches=True, random_uv=0.03)
    st = state(64, 48, 121)
    okw, rkw, S = inputs_of(st, "all")

    def build(tile=None, group=None):
        ice = csi.SlabThermodynamics(bottom_salinity=S, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), tile=tile, local_group=group,
                            ice_thermodynamics=ice, top_heat_flux=-40.0, ocean=csi.SlabOceanMixedLayer(DEPTH, temperature=st["To"], **okw))
        m.ocean.surface_flux_used
        return m

    def fields(m):
        m.synchronize()
        return [f.interior_numpy().copy() for f in (m.ice_thickness, m.ice_concentration, m.velocities.u, m.ocean.temperature,
                                                    m.ocean.bottom_heat_flux, m.ocean.surface_flux_used)]

    m = build()
    for n in range(2):
        csi.time_step(m, c["dt"])
    whole = fields(m)
    assert (whole[4] != 0).any()

    def tile(rank, group):
        mt = build((1, 2, rank), group)
        for n in range(2):
            csi.time_step(mt, c["dt"])
        return fields(mt), mt.grid

    for (parts, g) in run_tile_threads(2, tile):
        for k, (x, y) in enumerate(zip(parts, whole)):
            ny, nx = x.shape
            assert np.array_equal(x, y[g.j_off:g.j_off + ny, g.i_off:g.i_off + nx]), k


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_refusals_by_name():
    Nx, Ny = 64, 4
    g = grid(Nx, Ny)
    st = state(Nx, Ny, 131)
    good = csi.SlabOceanMixedLayer(DEPTH).params()

    def bad(**kw):
        p = csi.SlabOceanMixedLayer(DEPTH).params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    m = ocean_model(g, "fast", {}, 30.0, st["To"])
    for p, words in ((bad(density=float("nan")), "density is not finite"), (bad(deep_heat_flux=float("inf")), "deep_heat_flux is not finite"),
                     (bad(density=0.0), "density must be > 0"), (bad(heat_capacity=-1.0), "heat_capacity must be > 0"),
                     (bad(depth=0.0), "depth must be > 0"), (bad(exchange_velocity=-1e-9), "exchange_velocity must be >= 0"),
                     (bad(flags=32), "unknown flag bits"), (bad(reserved=1), "unknown flag bits")):
        with pytest.raises(csi.CsiError, match=words):
            m.ctx.call("csi_mixed_layer_set", C.byref(p))
    # a flag that names an unbound slot
    for flag, words in ((L.ML_SURFACE_ARRAY, "ocean_surface_heat_flux"), (L.ML_BULK_ARRAYS, "ocean_coefficient"), (L.ML_DEEP_ARRAY, "ocean_deep_heat_flux")):
        m.ctx.call("csi_mixed_layer_set", C.byref(bad(flags=flag)))
        with pytest.raises(csi.CsiError, match=words):
            m.ctx.mixed_layer_step(DT, False)
    m.ctx.call("csi_mixed_layer_set", C.byref(good))
    with pytest.raises(csi.CsiError, match="ocean_temperature-"):
        m.ctx.mixed_layer_step(DT, True)
    with pytest.raises(csi.CsiError, match="finite dt > 0"):
        m.ctx.mixed_layer_step(0.0, False)
    # bottom heat-flux terms other than exactly one ARRAY term
    two = (L.HeatFluxTerm * 2)()
    two[0].kind, two[1].kind, two[1].value = L.FLUX_ARRAY, L.FLUX_CONSTANT, 1.0
    for terms, n in ((two, 2), (None, 0)):
        m.ctx.call("csi_heat_fluxes_set", L.HEAT_BOTTOM, terms, n)
        with pytest.raises(csi.CsiError, match="exactly one ARRAY bottom heat-flux term"):
            m.ctx.mixed_layer_step(DT, False)
    # no slab parameters; no mixed layer
    m.ctx.call("csi_heat_fluxes_set", L.HEAT_BOTTOM, two, 1)
    m.ctx.mixed_layer_step(DT, False)
    m.ctx.call("csi_slab_params_set", None)
    with pytest.raises(csi.CsiError, match="needs csi_slab_params_set"):
        m.ctx.mixed_layer_step(DT, False)
    m.ctx.call("csi_mixed_layer_set", None)
    with pytest.raises(csi.CsiError, match="csi_mixed_layer_set has not been called"):
        m.ctx.mixed_layer_step(DT, False)
    # a series on the array the layer writes, either way round
    times = np.array([0.0, 100.0])
    fts = csi.FieldTimeSeries(g, (csi.Center, csi.Center), times, np.zeros((2, Ny, Nx)))
    ice = csi.SlabThermodynamics(bottom_salinity=30.0, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    s = csi.SeaIceModel(g, ice_thermodynamics=ice, timestepper="ForwardEuler", top_heat_flux=-40.0, bottom_heat_flux=fts)
    with pytest.raises(csi.CsiError, match="time series on bottom_heat_flux"):
        s.ctx.call("csi_mixed_layer_set", C.byref(good))
    m2 = ocean_model(g, "fast", {}, 30.0, st["To"])
    m2._series["BOTTOM_HEAT_FLUX"] = s._series["BOTTOM_HEAT_FLUX"]
    with pytest.raises(csi.CsiError, match="time series on bottom_heat_flux"):
        m2._set_series("BOTTOM_HEAT_FLUX")
    del m2._series["BOTTOM_HEAT_FLUX"]
    # an RK3 step needs the Psi^- copy
    c = _whole_case()
    ice = csi.SlabThermodynamics(bottom_salinity=30.0, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    r = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), ice_thermodynamics=ice, top_heat_flux=-40.0,
                        ocean=csi.SlabOceanMixedLayer(DEPTH))
    r.ctx.call("csi_field_bind", L.slot_id("ML_TEMPERATURE_M"), None, 0, 0, 0)
    with pytest.raises(csi.CsiError, match="ocean_temperature-"):
        csi.time_step(r, c["dt"])
