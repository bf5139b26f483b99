"""The SHORTWAVE top-flux term -- absorbed shortwave radiation with a stepped, temperature-dependent albedo -- on the GPU
(csrc/thermo_flux.hip, the SW_NUMBER / SW_CELL instantiations) against the NumPy restatement tests/thermo_shortwave_ref.py, bit for bit,
in STRICT and FAST mode (the thermodynamics is the same in both).  Shapes for the 64 x 4 block: 37 x 29, 64 x 4, 65 x 5, 130 x 9."""
import importlib.util
import os

import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import thermo_flux_ref as R
import thermo_linear_ref as T
import thermo_shortwave_ref as S
import time_series_ref as tsref
from test_gpu_local_tiles import run_tile_threads
from test_gpu_thermo_linear import DT, H, SHAPES, WEIGHTINGS, grid, mixed_state, thermo_model

pytestmark = pytest.mark.gpu

L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNOW_PAIR = (0.85, 0.70, -0.05)
MAXITERS = 1000
INVALID, UNSUPPORTED = -1, -4      # CSI_ERR_INVALID_ARGUMENT, CSI_ERR_UNSUPPORTED (include/csi.h)


def state(Nx, Ny, seed):
    """mixed_state of the LINEAR term's tests -- open water, h < hc, aice == 0, warm and cold air, snow of every depth and none, ice gone
    within the step -- plus the shortwave flux per cell, and a prescribed temperature that sits on both sides of the thresholds."""
    st = mixed_state(Nx, Ny, seed)
    rng = np.random.default_rng(seed + 1000)
    st["F"] = -320.0 * rng.random((Ny, Nx))
    st["F"][rng.random((Ny, Nx)) < 0.05] = 0.0
    near = rng.random((Ny, Nx)) < 0.5
    st["tp"] = np.where(near, -0.2 * rng.random((Ny, Nx)), st["tp"])
    st["tp"].flat[:4] = [-0.1, np.nextafter(-0.1, -np.inf), -0.05, np.nextafter(-0.05, -np.inf)]
    return st


def pair(st, weighting, per_cell, snow_pair):
    """(csi term, restatement term) of the shortwave term."""
    F = st["F"] if per_cell else -187.5
    c = csi.ShortwaveRadiation(F, csi.SteppedAlbedo(), csi.SteppedAlbedo(*SNOW_PAIR) if snow_pair else None, weighting)
    return c, S.Shortwave(F, S.SEMTNER, S.Albedo(*SNOW_PAIR) if snow_pair else None, weighting)


def tops(st, weighting, per_cell, snow_pair, beside):
    """beside: "alone"; "linear" (a LinearHeatFlux of numbers ahead of the term, no emission); "emission" (emission ahead of the term);
    "all": (emission, LinearHeatFlux per cell, the term, an array)."""
    c, r = pair(st, weighting, per_cell, snow_pair)
    if beside == "linear":
        return (csi.LinearHeatFlux(11.5, -3.25, "ice_present"), c), [T.Linear(11.5, -3.25, "ice_present"), r]
    if beside == "emission":
        return (csi.RadiativeEmission(), c, -210.0), [R.EMISSION, r, -210.0]
    if beside == "all":
        return ((csi.RadiativeEmission(), csi.LinearHeatFlux(st["K"], st["Ta"], "concentration"), c, st["qt"] - 250.0),
                [R.EMISSION, T.Linear(st["K"], st["Ta"], "concentration"), r, st["qt"] - 250.0])
    return c, [r]


def ref_steps(st, snow, rtop, rbottom, Sb, nsteps, prescribed=None, snowfall=0.0, dt=DT, Tu0=None):
    """The restatement stepped nsteps times: its last dict.  No consolidated cell may reach maxiters: asserted before any comparison."""
    h, a, hs = st["h"], st["a"], st["hs"]
    Tu = prescribed.copy() if prescribed is not None else (np.zeros_like(h) if Tu0 is None else Tu0)
    for n in range(nsteps):
        its = []
        if snow:
            r = S.layered_step(h, a, hs, Tu, dt, rtop, rbottom, snowfall, flux_balance=prescribed is None, S=Sb, iterations=its)
            h, a, hs, Tu = r["h"], r["aice"], r["hs"], r["tu_snow"]
        else:
            r = S.slab_step(h, a, Tu, dt, rtop, rbottom, flux_balance=prescribed is None, S=Sb, iterations=its)
            h, a, Tu = r["h"], r["aice"], r["Tu"]
        assert all(i.max() < MAXITERS for i in its if i.size), "the restatement's secant reached maxiters"
    return r


def device_fields(m, snow):
    used = m.heat_fluxes_used
    out = dict(h=m.ice_thickness, aice=m.ice_concentration, q_top=used.top, q_bottom=used.bottom, albedo=m.albedo_used)
    if snow:
        out.update(hs=m.snow_thickness, mf_ice=m.mass_fluxes.thermodynamics.ice, mf_snow=m.mass_fluxes.thermodynamics.snow,
                   mf_int=m.mass_fluxes.intercepted_snowfall, tu_ice=m.ice_top_temperature, tu_snow=m.snow_top_temperature)
    else:
        out.update(Tu=m.ice_thermodynamics.top_surface_temperature)
    return out


def run_and_compare(st, mode, snow, top, rtop, Sb, nsteps=3, prescribed=None, what=""):
    Ny, Nx = st["h"].shape
    r = ref_steps(st, snow, rtop, [st["qb"]], Sb, nsteps, prescribed=prescribed, snowfall=st["ps"] if snow else 0.0)
    m = thermo_model(grid(Nx, Ny), mode, snow, top, st["qb"], Sb, prescribed=prescribed, snowfall=st["ps"] if snow else 0.0)
    m.heat_fluxes_used
    m.albedo_used
    csi.set_(m, h=st["h"], aice=st["a"], **(dict(hs=st["hs"]) if snow else {}))
    for n in range(nsteps):
        csi.time_step(m, DT)
    m.synchronize()
    for k, f in device_fields(m, snow).items():
        got = f.interior_numpy()
        assert np.all(np.isfinite(got)), (what, k)
        assert np.array_equal(got, r[k]), (what, (Nx, Ny), k, np.abs(got - r[k]).max(), int((got != r[k]).sum()))
    return m, r


def test_the_state_holds_every_regime():
    """What the matrix below relies on, shown on the restatement once: in a 37 x 29 state the surface ends on the cold branch, on the
    warm branch below Tm, capped at Tm and unconsolidated; both snow albedos and both ice albedos are used; the term moves the result."""
    st = state(37, 29, 1)
    _, rtop = tops(st, None, True, True, "emission")
    r = ref_steps(st, True, rtop, [st["qb"]], st["S"], 1, snowfall=st["ps"])
    cons = st["h"] >= 0.05
    tu = r["tu_snow"]
    snowy = st["hs"] > 0
    assert (cons & ~snowy & (tu < -0.1)).any() and (cons & ~snowy & (tu >= -0.1) & (tu < 0)).any() and (cons & (tu == 0)).any()
    assert (~cons).any() and (cons & (st["a"] == 0)).any()
    # (under emission alone the snow stays cold; beside warm air -- the "all" tuple -- it reaches its warm albedo)
    _, rtop_all = tops(st, None, True, True, "all")
    r_all = ref_steps(st, True, rtop_all, [st["qb"]], st["S"], 1, snowfall=st["ps"])
    assert set(np.unique(r["albedo"])) | set(np.unique(r_all["albedo"])) == {0.85, 0.75, 0.70, 0.64}
    r0 = ref_steps(st, True, [R.EMISSION, -210.0], [st["qb"]], st["S"], 1, snowfall=st["ps"])
    assert np.abs(r["h"] - r0["h"]).max() > 1e-4


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_matrix_matches_restatement(weighting, snow, mode):
    """Each weighting x (F a number / per cell) x (alone / beside a LinearHeatFlux / beside emission / beside emission, a LinearHeatFlux
    and an array), the shapes taken in turn, the snow pair on every other case of the layered step: h, aice, hs, both surface
    temperatures, the three mass fluxes, both used fluxes and the albedo used equal the restatement.  With emission: three steps, Tu
    carried.  Without it the balance is two parallel lines with a jump between them, on which the secant can cycle until maxiters once
    its two starting points lie on different sides (include/csi.h): those cases take the one step from Tu- = 0 on which no cell of the
    state does -- ref_steps asserts it."""
    k = 0
    for per_cell in (False, True):
        for beside in ("alone", "linear", "emission", "all"):
            Nx, Ny = SHAPES[k % 4]
            k += 1
            st = state(Nx, Ny, 100 + k)
            top, rtop = tops(st, weighting, per_cell, snow and k % 2 == 0, beside)
            m, r = run_and_compare(st, mode, snow, top, rtop, st["S"] if beside == "all" else 30.0,
                                   nsteps=3 if beside in ("emission", "all") else 1, what=(weighting, per_cell, beside))
            assert (m.shortwave_flux is not None) == per_cell
            assert np.array_equal(m.heat_fluxes_used.top.interior_numpy(), r["q_top"])      # Qx(Tu): the absorbed shortwave is in it
    assert np.abs(r["h"] - st["h"]).max() > 1e-5 and np.unique(r["albedo"]).size >= 2


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_every_shape_with_everything_per_cell(snow, mode):
    for Nx, Ny in SHAPES:
        st = state(Nx, Ny, 7 + Nx)
        top, rtop = tops(st, "concentration", True, snow, "all")
        run_and_compare(st, mode, snow, top, rtop, st["S"], nsteps=2, what="shapes")


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_the_snow_pair_holds_where_hs_is_positive(mode):
    """A field with hs > 0 and hs == 0 cells under a prescribed temperature between the two thresholds and below both: the albedo used
    is the snow pair's exactly where the step started with snow."""
    Nx, Ny = 65, 5
    st = state(Nx, Ny, 21)
    snowy = st["hs"] > 0
    assert snowy.sum() > 20 and (~snowy).sum() > 20
    st["tp"] = np.where(np.arange(Nx * Ny).reshape(Ny, Nx) % 2 == 0, -0.07, -3.0)
    top, rtop = tops(st, None, True, True, "alone")
    m, r = run_and_compare(st, mode, True, top, rtop, 30.0, nsteps=1, prescribed=st["tp"], what="snow pair")
    got = m.albedo_used.interior_numpy()
    want = np.where(snowy, np.where(st["tp"] < -0.05, 0.85, 0.70), np.where(st["tp"] < -0.1, 0.75, 0.64))
    assert np.array_equal(got, want) and set(np.unique(got)) == {0.85, 0.75, 0.64}


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_prescribed_temperature_evaluates_the_term_there(snow, mode):
    """... per cell (the threshold itself and the next double below it among the cells) and as a number."""
    for k, per_cell in enumerate((False, True)):
        Nx, Ny = SHAPES[k]
        st = state(Nx, Ny, 31 + k)
        top, rtop = tops(st, WEIGHTINGS[k + 1], per_cell, snow, "all")
        m, r = run_and_compare(st, mode, snow, top, rtop, st["S"], prescribed=st["tp"], what=("prescribed", per_cell))
        if not snow:
            assert list(m.albedo_used.interior_numpy().flat[:2]) == [0.64, 0.75]
    # a number: no per-cell temperature is read (LTU off)
    st = state(64, 4, 35)
    c, r = pair(st, None, True, False)
    ice = csi.SlabThermodynamics(bottom_salinity=30.0, top_heat_boundary_condition=csi.PrescribedTemperature(-0.1))
    m = csi.SeaIceModel(grid(64, 4), ice_thermodynamics=ice, timestepper="ForwardEuler", mode=mode, top_heat_flux=(c, -20.0), bottom_heat_flux=2.0)
    m.albedo_used
    csi.set_(m, h=st["h"], aice=st["a"])
    csi.time_step(m, DT)
    m.synchronize()
    want = S.slab_step(st["h"], st["a"], np.full_like(st["h"], -0.1), DT, [r, -20.0], [2.0], flux_balance=False, S=30.0)
    assert np.array_equal(m.ice_thickness.interior_numpy(), want["h"]) and np.all(m.albedo_used.interior_numpy() == 0.64)


@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_halos_of_the_new_arrays_are_not_read(snow):
    """NaN and 1e300 in the halos of F and of albedo_used (and of K, Ta, S, the used-flux outputs) leave the results unchanged and the
    halos of the outputs untouched."""
    Nx, Ny = 37, 29
    st = state(Nx, Ny, 61)
    out = []
    for poison in (None, np.nan, 1e300):
        g = grid(Nx, Ny)
        flds = {k: csi.CenterField(g, "cuda:0", k) for k in ("F", "K", "Ta", "S")}
        for k, f in flds.items():
            if poison is not None:
                f.fill_parent(poison)
            f.set(st[k])
        top = (csi.RadiativeEmission(), csi.LinearHeatFlux(flds["K"], flds["Ta"]), csi.ShortwaveRadiation(flds["F"]), st["qt"] - 250.0)
        m = thermo_model(g, "fast", snow, top, st["qb"], flds["S"], snowfall=st["ps"] if snow else 0.0)
        assert m.shortwave_flux is flds["F"]
        outputs = (m.heat_fluxes_used.top, m.heat_fluxes_used.bottom, m.albedo_used)
        if poison is not None:
            for f in outputs:
                f.fill_parent(poison)
        csi.set_(m, h=st["h"], aice=st["a"], **(dict(hs=st["hs"]) if snow else {}))
        for n in range(2):
            csi.time_step(m, DT)
        m.synchronize()
        out.append({k: f.interior_numpy().copy() for k, f in device_fields(m, snow).items()})
        if poison is not None:
            full = m.albedo_used.numpy().copy()
            full[H:H + Ny, H:H + Nx] = poison
            assert np.all(np.isnan(full)) if np.isnan(poison) else np.all(full == poison)
    for other in out[1:]:
        for k in out[0]:
            assert np.all(np.isfinite(other[k])) and np.array_equal(out[0][k], other[k]), k


@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_a_series_drives_the_shortwave_flux(snow):
    """F by a HOST series with a window of two (Cyclical) beside a DEVICE series on the top array: equal to a run whose fields are set by
    hand from tests/time_series_ref.py before every step.  Both ride in the model's one table of series."""
    Nx, Ny = 65, 5
    st = state(Nx, Ny, 71)
    g = grid(Nx, Ny)
    rng = np.random.default_rng(72)
    times = np.array([0.0, 700.0, 1500.0, 2600.0])
    data = dict(F=st["F"] * (0.5 + rng.random((4, Ny, Nx))), q=st["qt"] - 200.0 + 20.0 * rng.standard_normal((4, Ny, Nx)))
    index = dict(F=(csi.Cyclical(3000.0), L.TIME_CYCLICAL, 3000.0, 2), q=(csi.Clamp(), L.TIME_CLAMP, 0.0, None))
    models = []
    for series in (True, False):
        v = {k: csi.FieldTimeSeries(g, (csi.Center, csi.Center), times, data[k], time_indexing=index[k][0], backend=csi.InMemory(index[k][3]))
             if series else data[k][0].copy() for k in data}
        top = (csi.ShortwaveRadiation(v["F"], area_weighting="concentration"), v["q"], csi.RadiativeEmission())
        m = thermo_model(g, "strict", snow, top, st["qb"], 30.0, snowfall=st["ps"] if snow else 0.0)
        m.albedo_used
        csi.set_(m, h=st["h"], aice=st["a"], **(dict(hs=st["hs"]) if snow else {}))
        models.append(m)
    A, B = models
    assert sorted(A._series) == ["SHORTWAVE", "TOP_HEAT_FLUX"] and not B._series
    targets = dict(F=lambda m: m.shortwave_flux, q=lambda m: m.external_heat_fluxes.top)
    for n in range(6):
        t = B.clock.time
        B.synchronize()
        for k in data:
            targets[k](B).set(tsref.at(times, data[k], index[k][1], index[k][2], t))
        csi.time_step(A, DT); csi.time_step(B, DT)
        A.synchronize(); B.synchronize()
        for k in data:
            assert np.array_equal(targets[k](A).interior_numpy(), targets[k](B).interior_numpy()), (n, k)
        fa, fb = device_fields(A, snow), device_fields(B, snow)
        for k in fa:
            assert np.array_equal(fa[k].interior_numpy(), fb[k].interior_numpy()), (snow, n, k)
    assert A.time_series_status("SHORTWAVE")[1] >= 3            # (the HOST series uploaded slices as the clock moved)
    assert np.abs(A.ice_thickness.interior_numpy() - st["h"]).max() > 1e-5


@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_whole_steps_with_advection(snow, stepper):
    """Whole FE / RK3 steps with EVP dynamics and WENO7 advection against the entry points driven by hand -- the library's stage loop
    against csi.time_step_momentum / the tracer and thermodynamic calls is what cases.csi_model's own tests pin; here: the per-cell
    kernels fed an array that holds one number give the bits of the number kernels, everything stays finite, the surface is solved."""
    c = cases.make_case(Nx=48, Ny=40, substeps=8, topo=("periodic", "bounded"), patches=True, random_uv=0.02)
    rng = np.random.default_rng(5)
    hs0 = np.where(c["a"] > 0, 0.2 * rng.random(c["a"].shape), 0.0)
    out = []
    for F in (-300.0, np.full((40, 48), -300.0)):
        ice = csi.SlabThermodynamics(bottom_salinity=31.0, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        sw = csi.ShortwaveRadiation(F, snow_albedo=csi.SteppedAlbedo(*SNOW_PAIR) if snow else None, area_weighting="concentration")
        kw = dict(ice_thermodynamics=ice, top_heat_flux=(csi.RadiativeEmission(), sw, -260.0), bottom_heat_flux=6.0)
        if snow:
            kw.update(snow_thermodynamics=csi.snow_slab_thermodynamics(), snowfall=3e-5)
        m = cases.csi_model(c, mode="strict", timestepper=stepper, advection=csi.WENO(order=7), **kw)
        used, alpha = m.heat_fluxes_used, m.albedo_used
        if snow:
            csi.set_(m, hs=hs0)
        for n in range(2):
            csi.time_step(m, c["dt"])
        m.synchronize()
        tu = m.snow_top_temperature if snow else m.ice_top_temperature
        out.append([f.numpy().copy() for f in (m.velocities.u, m.velocities.v, m.ice_thickness, m.ice_concentration, tu)] +
                   [used.top.interior_numpy().copy(), used.bottom.interior_numpy().copy(), alpha.interior_numpy().copy()])
    for x, y in zip(*out):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y)
    assert (out[0][4] < 0).any() and (out[0][5] != 0).any() and np.all(out[0][6] == 6.0)
    assert set(np.unique(out[0][7])) <= {0.85, 0.75, 0.70, 0.64}


@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
def test_whole_steps_against_the_entry_points_driven_by_hand(stepper):
    """FE and RK3 steps with EVP dynamics and WENO7: csi.time_step against a second model whose stages are driven through the entry
    points -- tracer tendencies, momentum, tracer update, csi_slab_thermo_step with the stage's step, update_state --, with emission,
    the shortwave term per cell and an array on top."""
    import ctypes as C
    c = cases.make_case(Nx=48, Ny=40, substeps=8, topo=("periodic", "bounded"), patches=True, random_uv=0.02)
    Ny, Nx = c["a"].shape
    st = state(Nx, Ny, 45)
    rk = stepper == "SplitRungeKutta3"

    def build():
        ice = csi.SlabThermodynamics(bottom_salinity=30.0, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        m = cases.csi_model(c, mode="fast", timestepper=stepper, advection=csi.WENO(order=7), ice_thermodynamics=ice, bottom_heat_flux=4.0,
                            top_heat_flux=(csi.RadiativeEmission(), csi.ShortwaveRadiation(st["F"], area_weighting="concentration"), st["qt"] - 250.0))
        m.albedo_used
        m.heat_fluxes_used
        return m

    A, B = build(), build()
    dt, sub, scheme = c["dt"], c["substeps"], 7
    for n in range(2):
        csi.time_step(A, dt)
        if rk:
            B.ctx.call("csi_cache_current_fields")
        elif n == 0:
            B.ctx.call("csi_update_state")
        for beta in ((3, 2, 1) if rk else (1,)):
            dtau = dt / beta
            B.ctx.call("csi_compute_tracer_tendencies", scheme)
            B.ctx.call("csi_time_step_momentum", dtau, sub, int(rk))
            B.ctx.call("csi_dynamic_step_tracers", dtau, int(rk))
            B.ctx.call("csi_slab_thermo_step", C.byref(B._slab_params), dtau)
            B.ctx.call("csi_update_state")
        B.clock.time += dt
        B.clock.iteration += 1
        A.synchronize(); B.synchronize()
        for name, get in (("h", lambda m: m.ice_thickness), ("aice", lambda m: m.ice_concentration), ("u", lambda m: m.velocities.u),
                          ("v", lambda m: m.velocities.v), ("Tu", lambda m: m.ice_top_temperature), ("albedo", lambda m: m.albedo_used),
                          ("q_top", lambda m: m.heat_fluxes_used.top)):
            x, y = get(A).interior_numpy(), get(B).interior_numpy()
            assert np.all(np.isfinite(x)) and np.array_equal(x, y), (stepper, n, name, np.abs(x - y).max())
    assert np.abs(A.ice_thickness.interior_numpy() - c["h"]).max() > 1e-6 and set(np.unique(A.albedo_used.interior_numpy())) <= {0.75, 0.64}


def test_checkpoint_round_trip():
    """The term has no state of its own: a restored model continues bit for bit (the surface temperature, Tu- of the solve, travels)."""
    Nx, Ny = 64, 4
    st = state(Nx, Ny, 81)

    def build():
        return thermo_model(grid(Nx, Ny), "strict", True, (csi.ShortwaveRadiation(st["F"], snow_albedo=csi.SteppedAlbedo(*SNOW_PAIR)), -220.0,
                                                                 csi.RadiativeEmission()),
                            st["qb"], st["S"], snowfall=st["ps"])

    m = build()
    csi.set_(m, h=st["h"], aice=st["a"], hs=st["hs"])
    for n in range(3):
        csi.time_step(m, DT)
    saved = csi.prognostic_state(m)
    for n in range(3):
        csi.time_step(m, DT)
    first = csi.prognostic_state(m)
    m2 = build()
    csi.restore_prognostic_state(m2, saved)
    for n in range(3):
        csi.time_step(m2, DT)
    second = csi.prognostic_state(m2)
    for k in first:
        if k != "clock":
            assert np.array_equal(first[k], second[k]), k
    assert not any("albedo" in k or "shortwave" in k for k in first)


def test_output_writer_lists_albedo_used(tmp_path):
    Nx, Ny = 37, 29
    st = state(Nx, Ny, 91)
    top, rtop = tops(st, "concentration", True, False, "emission")
    m = thermo_model(grid(Nx, Ny), "fast", False, top, st["qb"], 30.0)
    assert "albedo_used" not in csi.bound_fields(m) and "shortwave" in csi.bound_fields(m)
    csi.set_(m, h=st["h"], aice=st["a"])
    m.output_writers["q"] = csi.OutputWriter(m, ["h", "albedo_used", "shortwave"], csi.IterationInterval(1), str(tmp_path / "q"), dtype="f64")
    assert "albedo_used" in csi.bound_fields(m)             # (the writer asked for it)
    m.heat_fluxes_used
    for n in range(2):
        csi.time_step(m, DT)
    m.output_writers["q"].close()
    got = csi.load_output(str(tmp_path / "q"))
    r = ref_steps(st, False, rtop, [st["qb"]], 30.0, 2)
    assert list(got["iteration"]) == [0, 1, 2]
    assert np.array_equal(got["albedo_used"][2], r["albedo"]) and np.array_equal(got["h"][2], r["h"]) and np.array_equal(got["shortwave"][1], st["F"])
    no_term = thermo_model(grid(Nx, Ny), "fast", False, -30.0, 2.0, 30.0)
    with pytest.raises(ValueError, match="albedo_used needs a ShortwaveRadiation term"):
        no_term.albedo_used


def test_tiled_step_equals_untiled():
    """An RK3 step with EVP, WENO7, emission, the shortwave term per cell and an array on a 1 x 2 in-process tile group equals the
    untiled step, the albedo used included."""
    c = cases.make_case(Nx=64, Ny=48, H=8, substeps=8, topo=("periodic", "periodic"), patches=True, random_uv=0.03)
    st = state(64, 48, 37)

    def build(tile=None, group=None):
        ice = csi.SlabThermodynamics(bottom_salinity=st["S"], top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), tile=tile, local_group=group,
                            ice_thermodynamics=ice, bottom_heat_flux=st["qb"],
                            top_heat_flux=(csi.RadiativeEmission(), csi.ShortwaveRadiation(st["F"], area_weighting="concentration"), st["qt"] - 250.0))
        m.heat_fluxes_used
        m.albedo_used
        return m

    def fields(m):
        m.synchronize()
        return [f.interior_numpy().copy() for f in (m.ice_thickness, m.ice_concentration, m.ice_top_temperature, m.velocities.u,
                                                    m.heat_fluxes_used.top, m.albedo_used)]

    m = build()
    for n in range(2):
        csi.time_step(m, c["dt"])
    whole = fields(m)
    assert np.unique(whole[5]).size == 2

    def tile(rank, group):
        mt = build((1, 2, rank), group)
        for n in range(2):
            csi.time_step(mt, c["dt"])
        return fields(mt), mt.grid

    for (parts, g) in run_tile_threads(2, tile):
        for k, (x, y) in enumerate(zip(parts, whole)):
            ny, nx = x.shape
            assert np.array_equal(x, y[g.j_off:g.j_off + ny, g.i_off:g.i_off + nx]), k


def test_the_examples_column_crosses_the_threshold():
    """examples/arctic_basin_seasonal_cycle.py's column from day 130 with 2.8 m of ice, 90 eight-hour ForwardEuler steps: on the
    restatement the albedo drops from 0.75 to 0.64 and the surface reaches the melting point -- asserted first --, and the device gives
    the restatement's h, aice, Tu and albedo at every step."""
    spec = importlib.util.spec_from_file_location("arctic_basin_seasonal_cycle", os.path.join(ROOT, "examples", "arctic_basin_seasonal_cycle.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    for k in ("shortwave", "others"):
        assert np.array_equal(ex.FLUX[k], S.MONTHLY[k])
    assert np.array_equal(ex.TIMES, S.MONTH_TIMES) and ex.SIGMA == S.SIGMA and ex.DT == 8 * 3600.0
    t0, dt = 130 * S.DAY, ex.DT
    h, a, Tu = np.full((1, 4), 2.8), np.ones((1, 4)), np.full((1, 4), -8.0)
    want = []
    for n in range(90):
        its = []
        r = S.slab_step(h, a, Tu, dt, S.column_top(t0 + n * dt), [0.0], iterations=its)
        assert its[0].max() < MAXITERS
        h, a, Tu = r["h"], r["aice"], r["Tu"]
        want.append(r)
    alphas = np.array([r["albedo"][0, 0] for r in want])
    assert alphas[0] == 0.75 and alphas[-1] == 0.64 and want[0]["Tu"][0, 0] < -0.1 and want[-1]["Tu"][0, 0] == 0.0
    m = ex.build(timestepper="ForwardEuler", h0=2.8)
    m.albedo_used
    m.ice_thermodynamics.top_surface_temperature.set(np.full((1, 4), -8.0))
    m.clock.time = t0
    for n in range(90):
        csi.time_step(m, dt)
        got = ex.column(m)
        r = want[n]
        assert got == (r["h"][0, 0], r["aice"][0, 0], r["Tu"][0, 0], r["albedo"][0, 0]), (n, got)
    assert sorted(m._series) == ["SHORTWAVE", "TOP_HEAT_FLUX"]


@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_a_model_without_the_term_is_the_model_of_before(snow):
    """Emission, a LinearHeatFlux per cell, an array, a per-cell salinity and the used fluxes, no shortwave term: the fields equal
    tests/thermo_linear_ref.py, which the library matched bit for bit before the term existed; the shortwave slots stay unbound."""
    Nx, Ny = 130, 9
    st = state(Nx, Ny, 95)
    top = (csi.RadiativeEmission(), csi.LinearHeatFlux(st["K"], st["Ta"]), st["qt"] - 250.0)
    rtop = [R.EMISSION, T.Linear(st["K"], st["Ta"], "concentration"), st["qt"] - 250.0]
    m = thermo_model(grid(Nx, Ny), "strict", snow, top, st["qb"], st["S"], snowfall=st["ps"] if snow else 0.0)
    used = m.heat_fluxes_used
    assert m.shortwave is None and "shortwave" not in csi.bound_fields(m) and "albedo_used" not in csi.bound_fields(m)
    csi.set_(m, h=st["h"], aice=st["a"], **(dict(hs=st["hs"]) if snow else {}))
    h, a, hs, Tu = st["h"], st["a"], st["hs"], np.zeros_like(st["h"])
    for n in range(3):
        csi.time_step(m, DT)
        if snow:
            r = T.layered_step(h, a, hs, Tu, DT, rtop, [st["qb"]], st["ps"], S=st["S"])
            h, a, hs, Tu = r["h"], r["aice"], r["hs"], r["tu_snow"]
        else:
            r = T.slab_step(h, a, Tu, DT, rtop, [st["qb"]], S=st["S"])
            h, a, Tu = r["h"], r["aice"], r["Tu"]
    m.synchronize()
    got = dict(h=m.ice_thickness, aice=m.ice_concentration, q_top=used.top, q_bottom=used.bottom)
    got.update(dict(hs=m.snow_thickness, tu_snow=m.snow_top_temperature, tu_ice=m.ice_top_temperature) if snow
               else dict(Tu=m.ice_thermodynamics.top_surface_temperature))
    for k, f in got.items():
        assert np.array_equal(f.interior_numpy(), r[k]), k


def test_refusals_by_name():
    """The front end's, before a device is touched (the CPU tests run them too), and the library's own through the C ABI."""
    g = grid(8, 6)
    ice = lambda: csi.SlabThermodynamics()
    for kw, err, words in (
            (dict(bottom_heat_flux=csi.ShortwaveRadiation(-100.0)), NotImplementedError, "ShortwaveRadiation is a top heat flux only"),
            (dict(top_heat_flux=(csi.ShortwaveRadiation(-100.0), csi.ShortwaveRadiation(-50.0))), NotImplementedError, "at most one ShortwaveRadiation"),
            (dict(top_heat_flux=csi.ShortwaveRadiation(-100.0, snow_albedo=csi.SteppedAlbedo())), ValueError, "no snow layer"),
            (dict(top_heat_flux=csi.ShortwaveRadiation(np.zeros((3, 3)))), ValueError, "ShortwaveRadiation.flux"),
            (dict(top_heat_flux=lambda i, j, grid, T, clock, fields: 0.0), NotImplementedError, "FluxFunction and other callables")):
        with pytest.raises(err, match=words):
            csi.SeaIceModel(g, ice_thermodynamics=ice(), **kw)
    with pytest.raises(ValueError, match="an albedo lies in"):
        csi.SteppedAlbedo(cold=1.5)
    # the C ABI: a SHORTWAVE term without the set call; the term at the bottom; two terms; a per-cell flag without a bound slot; an
    # albedo outside [0, 1]; an unknown weighting
    m = csi.SeaIceModel(g, ice_thermodynamics=ice(), timestepper="ForwardEuler", top_heat_flux=-10.0)
    import ctypes as C
    term = lambda kind: L.HeatFluxTerm(kind, 0, 0.0, 0.0, 0.0, 0.0)
    one = (L.HeatFluxTerm * 1)(term(L.FLUX_SHORTWAVE))
    two = (L.HeatFluxTerm * 2)(term(L.FLUX_SHORTWAVE), term(L.FLUX_SHORTWAVE))

    def refused(code, words, name, *args):
        with pytest.raises(L.CsiError, match=words) as e:
            m.ctx.call(name, *args)
        assert e.value.code == code, (name, e.value.code)

    refused(INVALID, "needs csi_shortwave_set", "csi_heat_fluxes_set", L.HEAT_TOP, one, 1)
    refused(INVALID, "no array is bound to CSI_F_SHORTWAVE", "csi_shortwave_set",
            C.byref(L.Shortwave(0.0, 0.75, 0.64, -0.1, 0, 0, 0, 0, 1, 0, 0)))
    refused(INVALID, "csi_shortwave.cold: an albedo lies in", "csi_shortwave_set",
            C.byref(L.Shortwave(-100.0, 1.75, 0.64, -0.1, 0, 0, 0, 0, 0, 0, 0)))
    refused(INVALID, "csi_shortwave.snow_warm: an albedo lies in", "csi_shortwave_set",
            C.byref(L.Shortwave(-100.0, 0.75, 0.64, -0.1, 0.8, -0.2, 0.0, 0, 0, 1, 0)))
    refused(INVALID, "unknown weighting", "csi_shortwave_set", C.byref(L.Shortwave(-100.0, 0.75, 0.64, -0.1, 0, 0, 0, 7, 0, 0, 0)))
    for flags in ((2, 0, 0), (0, 2, 0), (-1, 0, 0), (0, 0, 1)):                   # per_cell, has_snow_pair other than 0 / 1; reserved != 0
        refused(INVALID, "per_cell and has_snow_pair are 0 or 1, reserved must be 0", "csi_shortwave_set",
                C.byref(L.Shortwave(-100.0, 0.75, 0.64, -0.1, 0.8, 0.7, 0.0, 0, *flags)))
    refused(INVALID, "flux is not finite", "csi_shortwave_set",
            C.byref(L.Shortwave(float("nan"), 0.75, 0.64, -0.1, 0, 0, 0, 0, 0, 0, 0)))
    m.ctx.call("csi_shortwave_set", C.byref(L.Shortwave(-100.0, 0.75, 0.64, -0.1, 0, 0, 0, 0, 0, 0, 0)))
    refused(UNSUPPORTED, "top heat flux only", "csi_heat_fluxes_set", L.HEAT_BOTTOM, one, 1)
    refused(UNSUPPORTED, "at most one ShortwaveRadiation", "csi_heat_fluxes_set", L.HEAT_TOP, two, 2)
    m.ctx.call("csi_heat_fluxes_set", L.HEAT_TOP, one, 1)                 # accepted now ...
    m.ctx.call("csi_shortwave_set", None)                                 # ... and with the setting removed the step refuses
    refused(INVALID, "needs csi_shortwave_set", "csi_time_step_fe", float(DT), 1, 0, 1)
