"""The LINEAR top-flux term, the per-cell bottom salinity and the used-flux outputs on the GPU (csrc/thermo_flux.hip) against the
NumPy restatement tests/thermo_linear_ref.py, bit for bit, in STRICT and FAST mode (the thermodynamics is the same in both).
Shapes for the 64 x 4 block: 37 x 29, 64 x 4, 65 x 5, 130 x 9."""
import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import thermo_flux_ref as R
import thermo_linear_ref as T
import time_series_ref as tsref
from test_gpu_local_tiles import run_tile_threads

pytestmark = pytest.mark.gpu

L = csi._lib
DT = 600.0
H = 3
SHAPES = [(37, 29), (64, 4), (65, 5), (130, 9)]
WEIGHTINGS = [None, "concentration", "ice_present"]


def grid(Nx, Ny):
    return csi.RectilinearGrid((Nx, Ny), x=(0, 1), y=(0, 1), halo=(H, H))


def mixed_state(Nx, Ny, seed):
    """Cell by cell: open water; h < hc; aice == 0 with h > 0; thick ice under warm air (Tu capped at Tm); cold air (freezing); snow of
    every depth and snow so thin that its melt cap binds; ice so thin that it is gone within the step."""
    rng = np.random.default_rng(seed)
    shape = (Ny, Nx)
    u = rng.random(shape)
    h = 0.06 + 2.0 * rng.random(shape)
    h[u < 0.10] = 0.0                                         # open water
    h[(u >= 0.10) & (u < 0.22)] = 0.03 * rng.random(shape)[(u >= 0.10) & (u < 0.22)]      # below hc = 0.05
    h[(u >= 0.22) & (u < 0.30)] = 2e-4                        # gone within a step of strong heating
    a = np.where(h > 0, 0.2 + 0.8 * rng.random(shape), 0.0)
    a[(u >= 0.30) & (u < 0.38)] = 0.0                         # aice == 0 with h > 0, consolidated
    hs = rng.random(shape) * 0.4 * (rng.random(shape) > 0.4) * (h > 0)
    hs[(u >= 0.38) & (u < 0.46)] = 1e-4                       # the melt cap binds
    K = 5.0 + 55.0 * rng.random(shape)
    K[u > 0.95] = 0.0
    Ta = -30.0 + 42.0 * rng.random(shape)                     # from hard frost to +12
    S = 25.0 + 10.0 * rng.random(shape)
    qt = -150.0 + 200.0 * rng.random(shape)
    qb = -20.0 + 40.0 * rng.random(shape)
    ps = 3e-5 * rng.random(shape)
    tp = -25.0 + 25.0 * rng.random(shape)
    return dict(h=h, a=a, hs=hs, K=K, Ta=Ta, S=S, qt=qt, qb=qb, ps=ps, tp=tp)


def linear_pair(st, weighting, per_cell):
    """(csi term, restatement term) of the LINEAR term: K / Ta as numbers, one per cell, both per cell."""
    K = st["K"] if per_cell in ("k", "both") else 17.5
    Ta = st["Ta"] if per_cell in ("ta", "both") else -6.25
    return csi.LinearHeatFlux(K, Ta, area_weighting=weighting), T.Linear(K, Ta, weighting)


def tops(st, weighting, per_cell, extra):
    c, r = linear_pair(st, weighting, per_cell)
    if extra:                                                 # emission and an array around the linear term
        return (csi.RadiativeEmission(), c, st["qt"] - 250.0), [R.EMISSION, r, st["qt"] - 250.0]
    return c, [r]


def thermo_model(g, mode, snow, top, bottom, S, prescribed=None, snowfall=0.0, **kw):
    bc = csi.PrescribedTemperature(prescribed) if prescribed is not None else csi.MeltingConstrainedFluxBalance()
    if snow:
        ice = csi.SlabThermodynamics(bottom_salinity=S, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        return csi.SeaIceModel(g, ice_thermodynamics=ice, snow_thermodynamics=csi.snow_slab_thermodynamics(top_heat_boundary_condition=bc),
                               snowfall=snowfall, timestepper="ForwardEuler", mode=mode, top_heat_flux=top, bottom_heat_flux=bottom, **kw)
    ice = csi.SlabThermodynamics(bottom_salinity=S, top_heat_boundary_condition=bc)
    return csi.SeaIceModel(g, ice_thermodynamics=ice, timestepper="ForwardEuler", mode=mode, top_heat_flux=top, bottom_heat_flux=bottom, **kw)


def ref_steps(st, snow, rtop, rbottom, S, nsteps, prescribed=None, snowfall=0.0):
    """The restatement stepped nsteps times: its last dict, with the names of device_fields."""
    h, a, hs = st["h"], st["a"], st["hs"]
    Tu = prescribed.copy() if prescribed is not None else np.zeros_like(h)
    for n in range(nsteps):
        if snow:
            r = T.layered_step(h, a, hs, Tu, DT, rtop, rbottom, snowfall, flux_balance=prescribed is None, S=S)
            h, a, hs, Tu = r["h"], r["aice"], r["hs"], r["tu_snow"]
        else:
            r = T.slab_step(h, a, Tu, DT, rtop, rbottom, flux_balance=prescribed is None, S=S)
            h, a, Tu = r["h"], r["aice"], r["Tu"]
    return r


def device_fields(m, snow):
    used = m.heat_fluxes_used
    out = dict(h=m.ice_thickness, aice=m.ice_concentration, q_top=used.top, q_bottom=used.bottom)
    if snow:
        out.update(hs=m.snow_thickness, mf_ice=m.mass_fluxes.thermodynamics.ice, mf_snow=m.mass_fluxes.thermodynamics.snow,
                   mf_int=m.mass_fluxes.intercepted_snowfall, tu_ice=m.ice_top_temperature, tu_snow=m.snow_top_temperature)
    else:
        out.update(Tu=m.ice_thermodynamics.top_surface_temperature)
    return out


def run_and_compare(st, mode, snow, top, rtop, S, nsteps=3, prescribed=None, what=""):
    Ny, Nx = st["h"].shape
    m = thermo_model(grid(Nx, Ny), mode, snow, top, st["qb"], S, prescribed=prescribed, snowfall=st["ps"] if snow else 0.0)
    m.heat_fluxes_used
    csi.set_(m, h=st["h"], aice=st["a"], **(dict(hs=st["hs"]) if snow else {}))
    for n in range(nsteps):
        csi.time_step(m, DT)
    m.synchronize()
    r = ref_steps(st, snow, rtop, [st["qb"]], S, nsteps, prescribed=prescribed, snowfall=st["ps"] if snow else 0.0)
    for k, f in device_fields(m, snow).items():
        if f is None:
            continue
        got = f.interior_numpy()
        assert np.all(np.isfinite(got)), (what, k)
        assert np.array_equal(got, r[k]), (what, (Nx, Ny), k, np.abs(got - r[k]).max(), int((got != r[k]).sum()))
    return m, r


def test_the_state_holds_every_regime():
    """What the matrix below relies on, shown on the restatement once: every regime of the issue occurs in a 37 x 29 state."""
    st = mixed_state(37, 29, 1)
    h, a, hs = st["h"], st["a"], st["hs"]
    _, rtop = tops(st, "concentration", "both", False)
    r = T.layered_step(h, a, hs, np.zeros_like(h), DT, rtop, [st["qb"]], 0.0, S=st["S"])      # (no snowfall: bare ice shows the cap)
    cons = h >= 0.05
    assert (h == 0).any() and ((h > 0) & ~cons).any() and (cons & (a == 0)).any()
    assert (cons & (r["tu_snow"] == 0.0) & (hs > 0)).any() and (cons & (r["tu_snow"] < -1.0)).any()          # melting (capped) and freezing
    assert ((hs > 0) & (r["hs"] == 0) & (r["aice"] > 0)).any()                                                  # snow melted away: the cap bound
    assert ((h > 0) & (a > 0) & (r["h"] == 0)).any()                                                            # all the ice lost within the step
    assert (r["h"] > h).any() and (r["h"] < h).any()


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_matrix_matches_restatement(weighting, snow, mode):
    """Each weighting x (K, Ta numbers / K per cell / Ta per cell / both per cell) x (alone / inside (emission, linear, array)), three
    steps with Tu carried, the shapes taken in turn; h, aice, hs, both surface temperatures, the three mass fluxes and both used
    fluxes equal the restatement."""
    k = 0
    for per_cell in ("numbers", "k", "ta", "both"):
        for extra in (False, True):
            Nx, Ny = SHAPES[k % 4]
            k += 1
            st = mixed_state(Nx, Ny, 100 + k)
            top, rtop = tops(st, weighting, per_cell, extra)
            S = st["S"] if per_cell == "both" else 30.0
            m, r = run_and_compare(st, mode, snow, top, rtop, S, what=(weighting, per_cell, extra))
            assert (m.linear_heat_flux is not None) == (per_cell != "numbers")
    assert np.abs(r["h"] - st["h"]).max() > 1e-5


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_every_shape_with_everything_per_cell(snow, mode):
    for Nx, Ny in SHAPES:
        st = mixed_state(Nx, Ny, 7 + Nx)
        top, rtop = tops(st, "concentration", "both", True)
        run_and_compare(st, mode, snow, top, rtop, st["S"], nsteps=2, what="shapes")


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_prescribed_temperature_evaluates_the_term_there(snow, mode):
    for k, per_cell in enumerate(("numbers", "both")):
        Nx, Ny = SHAPES[k]
        st = mixed_state(Nx, Ny, 31 + k)
        top, rtop = tops(st, WEIGHTINGS[k + 1], per_cell, True)
        run_and_compare(st, mode, snow, top, rtop, st["S"], prescribed=st["tp"], what=("prescribed", per_cell))


@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
@pytest.mark.parametrize("linear", [False, True])
def test_per_cell_bottom_salinity(linear, snow):
    """Per-cell S with and without the linear term against the restatement; an array holding one number gives the number path's bits."""
    Nx, Ny = 65, 5
    st = mixed_state(Nx, Ny, 41)
    top, rtop = tops(st, "ice_present", "numbers", False) if linear else (-35.0, [-35.0])
    run_and_compare(st, "fast", snow, top, rtop, st["S"], what=("salinity", linear))
    out = []
    for S in (31.25, np.full((Ny, Nx), 31.25)):
        m = thermo_model(grid(Nx, Ny), "strict", snow, top, 3.0, S, snowfall=2e-5 if snow else 0.0)
        assert (m.bottom_salinity is not None) == (not np.isscalar(S))
        csi.set_(m, h=st["h"], aice=st["a"], **(dict(hs=st["hs"]) if snow else {}))
        for n in range(3):
            csi.time_step(m, DT)
        m.synchronize()
        out.append([f.interior_numpy().copy() for f in (m.ice_thickness, m.ice_concentration) + ((m.snow_thickness,) if snow else ())])
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    assert np.abs(out[0][0] - st["h"]).max() > 1e-6


@pytest.mark.parametrize("config", ["slab_equilibrium", "slab_balance", "layered"])
def test_used_fluxes_on_a_numeric_configuration(config):
    """Binding the outputs selects the flux kernels for a configuration of numbers: h, aice, hs keep the number path's bits and the
    fields hold the numbers (with the equilibrium default the top one holds the internal flux)."""
    Nx, Ny = 130, 9
    st = mixed_state(Nx, Ny, 51)
    snow = config == "layered"
    out, used = [], None
    for bind in (False, True):
        if config == "slab_equilibrium":
            ice = csi.SlabThermodynamics(top_temperature=-8.0, bottom_salinity=30.0, bottom_heat_flux=4.0)
            m = csi.SeaIceModel(grid(Nx, Ny), ice_thermodynamics=ice, timestepper="ForwardEuler")
        else:
            m = thermo_model(grid(Nx, Ny), "fast", snow, -60.0, 4.0, 30.0, snowfall=2e-5 if snow else 0.0)
        if bind:
            used = m.heat_fluxes_used
            assert {"top_heat_flux_used", "bottom_heat_flux_used"} <= set(csi.bound_fields(m))
        else:
            assert "top_heat_flux_used" not in csi.bound_fields(m)
        csi.set_(m, h=st["h"], aice=st["a"], **(dict(hs=st["hs"]) if snow else {}))
        for n in range(3):
            if n == 2:
                before = m.ice_thickness.interior_numpy().copy()
            csi.time_step(m, DT)
        m.synchronize()
        out.append([f.interior_numpy().copy() for f in (m.ice_thickness, m.ice_concentration) + ((m.snow_thickness,) if snow else ())])
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    qt, qb = used.top.interior_numpy(), used.bottom.interior_numpy()
    assert np.all(qb == 4.0)
    if config == "slab_equilibrium":      # Qu is the internal flux -k (Tu - Tb) / h of the state the last step started from
        Tb = 0.0 - 0.054 * 30.0
        with np.errstate(all="ignore"):
            want = np.where(before <= 0, 0.0, -2.0 * (-8.0 - Tb) / before)
        assert np.array_equal(qt, want) and (qt != 0).any()
    else:
        assert np.all(qt == -60.0)
    full = used.top.numpy()
    assert np.all(full[:H] == 0) and np.all(full[:, :H] == 0)          # halos are never written


@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_halos_of_the_new_arrays_are_not_read(snow):
    """NaN and 1e300 in the halos of K, Ta, S and of the used-flux outputs leave the results unchanged."""
    Nx, Ny = 37, 29
    st = mixed_state(Nx, Ny, 61)
    out = []
    for poison in (None, np.nan, 1e300):
        g = grid(Nx, Ny)
        flds = {k: csi.CenterField(g, "cuda:0", k) for k in ("K", "Ta", "S")}
        for k, f in flds.items():
            if poison is not None:
                f.fill_parent(poison)
            f.set(st[k])
        top = (csi.RadiativeEmission(), csi.LinearHeatFlux(flds["K"], flds["Ta"]), st["qt"] - 250.0)
        m = thermo_model(g, "fast", snow, top, st["qb"], flds["S"], snowfall=st["ps"] if snow else 0.0)
        used = m.heat_fluxes_used
        if poison is not None:
            for f in (used.top, used.bottom):
                f.fill_parent(poison)
        csi.set_(m, h=st["h"], aice=st["a"], **(dict(hs=st["hs"]) if snow else {}))
        for n in range(2):
            csi.time_step(m, DT)
        m.synchronize()
        out.append({k: f.interior_numpy().copy() for k, f in device_fields(m, snow).items()})
        if poison is not None:
            full = used.top.numpy().copy()
            full[H:H + Ny, H:H + Nx] = poison
            assert np.all(np.isnan(full)) if np.isnan(poison) else np.all(full == poison)
    for other in out[1:]:
        for k in out[0]:
            assert np.all(np.isfinite(other[k])) and np.array_equal(out[0][k], other[k]), k


@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_series_drive_coefficient_reference_temperature_and_salinity(snow):
    """Ta by a DEVICE series (Clamp), K and S by HOST series with a window of two (Linear, Cyclical): equal to a run whose three
    fields are set by hand from tests/time_series_ref.py before every step.  All three ride in the one table of one launch: the
    series-driven slots of the model are exactly these three."""
    Nx, Ny = 65, 5
    st = mixed_state(Nx, Ny, 71)
    g = grid(Nx, Ny)
    rng = np.random.default_rng(72)
    times = np.array([0.0, 700.0, 1500.0, 2600.0])
    data = dict(Ta=st["Ta"] + 6.0 * rng.standard_normal((4, Ny, Nx)), K=st["K"] * (0.5 + rng.random((4, Ny, Nx))),
                S=st["S"] + rng.standard_normal((4, Ny, Nx)))
    index = dict(Ta=(csi.Clamp(), L.TIME_CLAMP, 0.0, None), K=(csi.Linear(), L.TIME_LINEAR, 0.0, 2), S=(csi.Cyclical(3000.0), L.TIME_CYCLICAL, 3000.0, 2))
    models = []
    for series in (True, False):
        v = {k: csi.FieldTimeSeries(g, (csi.Center, csi.Center), times, data[k], time_indexing=index[k][0], backend=csi.InMemory(index[k][3]))
             if series else data[k][0].copy() for k in data}
        top = (csi.LinearHeatFlux(v["K"], v["Ta"]), -30.0)
        m = thermo_model(g, "strict", snow, top, st["qb"], v["S"], snowfall=st["ps"] if snow else 0.0)
        csi.set_(m, h=st["h"], aice=st["a"], **(dict(hs=st["hs"]) if snow else {}))
        models.append(m)
    A, B = models
    assert sorted(A._series) == ["BOTTOM_SALINITY", "FLUX_COEFFICIENT", "FLUX_REFERENCE_TEMPERATURE"] and not B._series
    targets = dict(Ta=lambda m: m.linear_heat_flux.reference_temperature, K=lambda m: m.linear_heat_flux.coefficient, S=lambda m: m.bottom_salinity)
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
    assert A.time_series_status("FLUX_COEFFICIENT")[1] >= 3            # (the HOST series uploaded slices as the clock moved)
    assert np.abs(A.ice_thickness.interior_numpy() - st["h"]).max() > 1e-5


@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_whole_steps_with_advection(snow, stepper):
    """Whole FE / RK3 steps with EVP dynamics and WENO7 advection: the per-cell kernels fed arrays that hold one number give the bits
    of the number kernels, everything stays finite and the surface temperature is solved."""
    c = cases.make_case(Nx=48, Ny=40, substeps=8, topo=("periodic", "bounded"), patches=True, random_uv=0.02)
    rng = np.random.default_rng(5)
    hs0 = np.where(c["a"] > 0, 0.2 * rng.random(c["a"].shape), 0.0)
    out = []
    for K, Ta, S in ((12.5, -9.0, 31.0), (np.full((40, 48), 12.5), np.full((40, 48), -9.0), np.full((40, 48), 31.0))):
        ice = csi.SlabThermodynamics(bottom_salinity=S, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        kw = dict(ice_thermodynamics=ice, top_heat_flux=(csi.RadiativeEmission(), csi.LinearHeatFlux(K, Ta), -280.0), bottom_heat_flux=6.0)
        if snow:
            kw.update(snow_thermodynamics=csi.snow_slab_thermodynamics(), snowfall=3e-5)
        m = cases.csi_model(c, mode="strict", timestepper=stepper, advection=csi.WENO(order=7), **kw)
        used = m.heat_fluxes_used
        if snow:
            csi.set_(m, hs=hs0)
        for n in range(2):
            csi.time_step(m, c["dt"])
        m.synchronize()
        tu = m.snow_top_temperature if snow else m.ice_top_temperature
        out.append([f.numpy().copy() for f in (m.velocities.u, m.velocities.v, m.ice_thickness, m.ice_concentration, tu)] +
                   [used.top.interior_numpy().copy(), used.bottom.interior_numpy().copy()])
    for x, y in zip(*out):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y)
    assert (out[0][4] < 0).any() and (out[0][5] != 0).any() and np.all(out[0][6] == 6.0)


def test_checkpoint_round_trip_carries_the_surface_temperature():
    Nx, Ny = 64, 4
    st = mixed_state(Nx, Ny, 81)

    def build():
        m = thermo_model(grid(Nx, Ny), "strict", False, csi.LinearHeatFlux(st["K"], -8.0), st["qb"], st["S"])
        return m

    m = build()
    csi.set_(m, h=st["h"], aice=st["a"])
    for n in range(3):
        csi.time_step(m, DT)
    state = csi.prognostic_state(m)
    assert "ice_thermodynamics.top_surface_temperature" in state
    for n in range(3):
        csi.time_step(m, DT)
    first = csi.prognostic_state(m)
    m2 = build()
    csi.restore_prognostic_state(m2, state)
    for n in range(3):
        csi.time_step(m2, DT)
    second = csi.prognostic_state(m2)
    for k in first:
        if k != "clock":
            assert np.array_equal(first[k], second[k]), k
    assert np.abs(first["ice_thermodynamics.top_surface_temperature"]).max() > 0


def test_output_writer_lists_a_used_flux(tmp_path):
    Nx, Ny = 37, 29
    st = mixed_state(Nx, Ny, 91)
    top, rtop = tops(st, "concentration", "both", False)
    m = thermo_model(grid(Nx, Ny), "fast", False, top, st["qb"], st["S"])
    with pytest.raises(ValueError, match="'top_heat_flux_used'"):
        csi.OutputWriter(m, ["h", "top_heat_flux_used"], csi.IterationInterval(1), str(tmp_path / "a"))
    m.heat_fluxes_used
    csi.set_(m, h=st["h"], aice=st["a"])
    m.output_writers["q"] = csi.OutputWriter(m, ["h", "top_heat_flux_used", "bottom_heat_flux_used", "flux_coefficient", "bottom_salinity"],
                                             csi.IterationInterval(1), str(tmp_path / "q"), dtype="f64")
    for n in range(2):
        csi.time_step(m, DT)
    m.output_writers["q"].close()
    got = csi.load_output(str(tmp_path / "q"))
    r = ref_steps(st, False, rtop, [st["qb"]], st["S"], 2)
    assert list(got["iteration"]) == [0, 1, 2]
    assert np.array_equal(got["top_heat_flux_used"][2], r["q_top"]) and np.array_equal(got["bottom_heat_flux_used"][2], st["qb"])
    assert np.array_equal(got["h"][2], r["h"]) and np.array_equal(got["flux_coefficient"][0], st["K"]) and np.array_equal(got["bottom_salinity"][1], st["S"])


def test_tiled_step_equals_untiled():
    """An RK3 step with EVP, WENO7, the linear term per cell, emission, an array and a per-cell salinity on a 1 x 2 in-process tile
    group equals the untiled step, used fluxes included."""
    c = cases.make_case(Nx=64, Ny=48, H=8, substeps=8, topo=("periodic", "periodic"), patches=True, random_uv=0.03)
    st = mixed_state(64, 48, 37)

    def build(tile=None, group=None):
        ice = csi.SlabThermodynamics(bottom_salinity=st["S"], top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), tile=tile, local_group=group,
                            ice_thermodynamics=ice, bottom_heat_flux=st["qb"],
                            top_heat_flux=(csi.RadiativeEmission(), csi.LinearHeatFlux(st["K"], st["Ta"]), st["qt"] - 250.0))
        m.heat_fluxes_used
        return m

    def state(m):
        m.synchronize()
        return [f.interior_numpy().copy() for f in (m.ice_thickness, m.ice_concentration, m.ice_top_temperature, m.velocities.u,
                                                    m.heat_fluxes_used.top, m.heat_fluxes_used.bottom)]

    m = build()
    for n in range(2):
        csi.time_step(m, c["dt"])
    whole = state(m)
    assert (whole[4] != 0).any()

    def tile(rank, group):
        mt = build((1, 2, rank), group)
        for n in range(2):
            csi.time_step(mt, c["dt"])
        return state(mt), mt.grid

    for (parts, g) in run_tile_threads(2, tile):
        for k, (x, y) in enumerate(zip(parts, whole)):
            ny, nx = x.shape
            assert np.array_equal(x, y[g.j_off:g.j_off + ny, g.i_off:g.i_off + nx]), k


@pytest.mark.parametrize("snow, precipitation, melting, partial", [(False, False, False, False), (False, False, True, True),
                                                                   (True, True, False, False), (True, True, True, True)])
def test_energy_closure_on_the_device(snow, precipitation, melting, partial):
    """Twenty steps of the CPU test's state, 37 x 29 cells: the residual of test/test_energy_conservation.jl formed from the fields
    the device wrote (h, aice, hs, both used fluxes, the intercepted snowfall), within the reference's bounds -- 1e-15 at aice = 1,
    1e-13 at aice < 1."""
    Nx, Ny = 37, 29
    st = T.closure_state(n=Nx * Ny, partial=partial, snow=snow, melting=melting)
    shaped = {k: v.reshape(Ny, Nx) for k, v in st.items()}
    K = 1e-3 * 1.225 * 1004 * 5
    top = csi.bulk_sensible_heat_flux(1e-3, 1.225, 1004, 5, shaped["Ta"])
    assert top.coefficient == K
    m = thermo_model(grid(Nx, Ny), "fast", snow, top, shaped["Qb"], 0.0, snowfall=6e-5 if precipitation else 0.0)
    used = m.heat_fluxes_used
    csi.set_(m, h=shaped["h"], aice=shaped["a"], **(dict(hs=shaped["hs"]) if snow else {}))

    def step(r, rtop, rbottom, Ps):
        csi.time_step(m, DT)
        m.synchronize()
        get = lambda f: f.interior_numpy().reshape(-1).copy()
        return dict(h=get(m.ice_thickness), aice=get(m.ice_concentration), hs=get(m.snow_thickness) if snow else np.zeros(Nx * Ny),
                    Tu=r["Tu"], q_top=get(used.top), q_bottom=get(used.bottom),
                    mf_int=get(m.mass_fluxes.intercepted_snowfall) if snow else np.zeros(Nx * Ny))

    worst = T.closure_run(st, snow, precipitation, 20, step=step)
    cpu = T.closure_run(st, snow, precipitation, 20)
    print(f"device energy closure snow={snow} precipitation={precipitation} melting={melting} partial={partial}: "
          f"{worst.max():.2e} (restatement {cpu.max():.2e})")
    assert worst.max() < (1e-13 if partial else 1e-15)
    assert np.abs(m.ice_thickness.interior_numpy() - shaped["h"]).max() > 1e-4


@pytest.mark.parametrize("snow", [False, True], ids=["bare", "snowy"])
def test_melting_in_spring_columns(snow):
    """examples/melting_in_spring.py's four columns -- (RadiativeEmission(), the solar array, the bulk flux) on 1 m of ice, bare and
    under 20 cm of snow -- after 50 steps of 10 minutes against the restatement (the full 30 days stay in the example)."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "melting_in_spring.py")
    spec = importlib.util.spec_from_file_location("melting_in_spring", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    m = ex.build(snow=snow)
    for n in range(50):
        csi.time_step(m, 600.0)
    got = ex.columns(m)
    K = ((1e-3 * 1.225) * 1004) * 5
    rtop = [R.EMISSION, ex.SOLAR.astype(np.float64), T.Linear(K, -5.0, "concentration")]
    st = dict(h=np.ones((1, 4)), a=np.ones((1, 4)), hs=np.full((1, 4), 0.2))
    r = ref_steps(st, snow, rtop, [0.0], 0.0, 50)
    want = [r["h"][0], r["aice"][0], r["tu_snow" if snow else "Tu"][0]] + ([r["hs"][0]] if snow else [])
    for x, y in zip(got, want):
        assert np.array_equal(x, y), (snow, x, y)
    melting = got[3] if snow else got[0]                                 # (under snow the snow melts first)
    assert np.unique(melting).size == 4 and np.all(melting < (0.2 if snow else 1.0))      # four different columns, all melting
