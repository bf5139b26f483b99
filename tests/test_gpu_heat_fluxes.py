"""Per-cell heat fluxes, RadiativeEmission, per-cell PrescribedTemperature and snowfall on the GPU (csrc/thermo_flux.hip) against
the NumPy restatement tests/thermo_flux_ref.py, bit for bit, in STRICT and FAST mode (the thermodynamics is the same in both)."""
import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import thermo_flux_ref as R
from test_gpu_local_tiles import run_tile_threads

pytestmark = pytest.mark.gpu

S_BOTTOM = 30.0
DT = 600.0


def mixed_state(Nx, Ny, seed):
    """Open water, thin (unconsolidated) and consolidated ice, thick melting ice and snow of every depth, cell by cell."""
    rng = np.random.default_rng(seed)
    shape = (Ny, Nx)
    h = rng.random(shape) * 2.0 * (rng.random(shape) > 0.15)
    h[rng.random(shape) < 0.2] *= 0.03                       # below the consolidation thickness 0.05
    a = np.where(h > 0, 0.2 + 0.8 * rng.random(shape), 0.0)
    hs = rng.random(shape) * 0.4 * (rng.random(shape) > 0.4) * (h > 0)
    qt = -250.0 + 400.0 * rng.random(shape)                  # from strong heating (melting) to cooling
    qb = -20.0 + 40.0 * rng.random(shape)
    ps = 3e-5 * rng.random(shape)
    tp = -25.0 + 25.0 * rng.random(shape)
    return h, a, hs, qt, qb, ps, tp


def thermo_model(g, mode, snow=False, prescribed=None, snowfall=0.0, **kw):
    bc = csi.PrescribedTemperature(prescribed) if prescribed is not None else csi.MeltingConstrainedFluxBalance()
    if snow:
        ice = csi.SlabThermodynamics(bottom_salinity=S_BOTTOM, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        return csi.SeaIceModel(g, ice_thermodynamics=ice, snow_thermodynamics=csi.snow_slab_thermodynamics(top_heat_boundary_condition=bc),
                               snowfall=snowfall, timestepper="ForwardEuler", mode=mode, **kw)
    ice = csi.SlabThermodynamics(bottom_salinity=S_BOTTOM, top_heat_boundary_condition=bc)
    return csi.SeaIceModel(g, ice_thermodynamics=ice, timestepper="ForwardEuler", mode=mode, **kw)


def grid(Nx, Ny):
    return csi.RectilinearGrid((Nx, Ny), x=(0, 1), y=(0, 1), halo=(3, 3))


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("snow", [False, True])
def test_array_equal_to_a_number_is_the_number_path(mode, snow):
    """Item 1, a thermodynamic step alone: an array holding the number everywhere gives the numeric path's bits."""
    Nx, Ny = 64, 48
    h, a, hs, *_ = mixed_state(Nx, Ny, 3)
    out = []
    for top, bottom in ((-60.0, 4.0), (np.full((Ny, Nx), -60.0), np.full((Ny, Nx), 4.0))):
        m = thermo_model(grid(Nx, Ny), mode, snow=snow, snowfall=2e-5, top_heat_flux=top, bottom_heat_flux=bottom)
        csi.set_(m, h=h, aice=a, **(dict(hs=hs) if snow else {}))
        for n in range(5):
            csi.time_step(m, DT)
        m.synchronize()
        out.append([f.interior_numpy().copy() for f in (m.ice_thickness, m.ice_concentration) + ((m.snow_thickness,) if snow else ())])
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    assert np.abs(out[0][0] - h).max() > 1e-6


@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
@pytest.mark.parametrize("snow", [False, True])
def test_array_equal_to_a_number_in_whole_steps(stepper, snow):
    """Item 1, whole FE / RK3 steps with EVP dynamics and WENO7 advection: the array path gives the numeric path's bits."""
    c = cases.make_case(Nx=48, Ny=40, substeps=8, topo=("periodic", "bounded"), patches=True, random_uv=0.02)
    rng = np.random.default_rng(5)
    hs0 = np.where(c["a"] > 0, 0.2 * rng.random(c["a"].shape), 0.0)
    out = []
    for top in (-80.0, np.full((40, 48), -80.0)):
        kw = dict(ice_thermodynamics=csi.SlabThermodynamics(bottom_salinity=S_BOTTOM,
                                                            top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance()),
                  top_heat_flux=top, bottom_heat_flux=6.0)
        if snow:
            kw.update(snow_thermodynamics=csi.snow_slab_thermodynamics(), snowfall=3e-5)
        m = cases.csi_model(c, mode="strict", timestepper=stepper, advection=csi.WENO(order=7), **kw)
        if snow:
            csi.set_(m, hs=hs0)
        for n in range(2):
            csi.time_step(m, c["dt"])
        m.synchronize()
        out.append([f.numpy().copy() for f in (m.velocities.u, m.velocities.v, m.ice_thickness, m.ice_concentration)])
    for x, y in zip(*out):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y)


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("case", ["arrays", "emission", "prescribed"])
def test_slab_step_matches_restatement(mode, case):
    """Item 2, bare ice: per-cell top and bottom arrays, RadiativeEmission (secant from Tu-), a per-cell PrescribedTemperature;
    64 x 48 cells in every regime, 20 steps with Tu carried from step to step."""
    Nx, Ny = 64, 48
    h, a, hs, qt, qb, ps, tp = mixed_state(Nx, Ny, 11)
    top = {"arrays": (qt,), "emission": (R.EMISSION, qt - 200.0), "prescribed": (R.EMISSION, qt)}[case]
    prescribed = tp if case == "prescribed" else None
    m = thermo_model(grid(Nx, Ny), mode, prescribed=prescribed, bottom_heat_flux=qb,
                     top_heat_flux=tuple(csi.RadiativeEmission() if isinstance(t, R.Emission) else t for t in top))
    csi.set_(m, h=h, aice=a)
    Tu = tp.copy() if prescribed is not None else np.zeros_like(h)
    rh, ra = h.copy(), a.copy()
    for n in range(20):
        rh, ra, Tu, mf = R.slab_step(rh, ra, Tu, DT, list(top), [qb], flux_balance=prescribed is None, S=S_BOTTOM)
        csi.time_step(m, DT)
    m.synchronize()
    for k, f, r in (("h", m.ice_thickness, rh), ("aice", m.ice_concentration, ra), ("Tu", m.ice_thermodynamics.top_surface_temperature, Tu)):
        got = f.interior_numpy()
        assert np.all(np.isfinite(got)), k
        assert np.array_equal(got, r), (case, k, np.abs(got - r).max())
    assert (rh < 0.05).any() and (rh >= 0.05).any()
    if prescribed is None:
        assert (Tu < 0).any() and (Tu == 0).any()       # frozen surfaces and melting ones capped at Tm(S_ice = 0) = 0


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("case", ["emission", "prescribed"])
def test_layered_step_matches_restatement(mode, case):
    """Item 2, snow on ice: per-cell top and bottom arrays, emission at the snow surface (secant from Tus-) or a per-cell prescribed
    snow-surface temperature, per-cell snowfall; 20 steps."""
    Nx, Ny = 64, 48
    h, a, hs, qt, qb, ps, tp = mixed_state(Nx, Ny, 17)
    prescribed = tp if case == "prescribed" else None
    top = (R.EMISSION, qt - 200.0)
    m = thermo_model(grid(Nx, Ny), mode, snow=True, prescribed=prescribed, snowfall=ps, bottom_heat_flux=qb,
                     top_heat_flux=(csi.RadiativeEmission(), qt - 200.0))
    csi.set_(m, h=h, aice=a, hs=hs)
    r = dict(h=h, aice=a, hs=hs, tu_snow=tp.copy() if prescribed is not None else np.zeros_like(h))
    for n in range(20):
        r = R.layered_step(r["h"], r["aice"], r["hs"], r["tu_snow"], DT, list(top), [qb], ps, flux_balance=prescribed is None, S=S_BOTTOM)
        csi.time_step(m, DT)
    m.synchronize()
    got = dict(h=m.ice_thickness, aice=m.ice_concentration, hs=m.snow_thickness, mf_ice=m.mass_fluxes.thermodynamics.ice,
               mf_snow=m.mass_fluxes.thermodynamics.snow, mf_int=m.mass_fluxes.intercepted_snowfall, tu_ice=m.ice_top_temperature,
               tu_snow=m.snow_top_temperature)
    for k, f in got.items():
        x = f.interior_numpy()
        assert np.all(np.isfinite(x)), k
        assert np.array_equal(x, r[k]), (case, k, np.abs(x - r[k]).max())
    assert (r["hs"] > 0).any()


def test_three_term_sum_is_right_nested():
    """Item 3: (1e16, -1e16, 1) sums to 1e16 + (-1e16 + 1) = 0, not (1e16 - 1e16) + 1 = 1 (boundary_fluxes.jl:15-22)."""
    Nx, Ny = 16, 8
    h, a, *_ = mixed_state(Nx, Ny, 23)
    top = (1e16, -1e16, 1.0)
    assert R.getflux(list(top), np.zeros(1))[0] == 0.0 and (1e16 + -1e16) + 1.0 == 1.0
    out = {}
    for spec in (top, 0.0, 1.0):
        m = thermo_model(grid(Nx, Ny), "strict", prescribed=np.full((Ny, Nx), -5.0), top_heat_flux=spec)
        csi.set_(m, h=h, aice=a)
        csi.time_step(m, DT)
        m.synchronize()
        out[spec] = m.ice_thickness.interior_numpy().copy()
    rh, *_ = R.slab_step(h, a, np.full_like(h, -5.0), DT, list(top), [0.0], flux_balance=False, S=S_BOTTOM)
    assert np.array_equal(out[top], rh) and np.array_equal(out[top], out[0.0]) and not np.array_equal(out[top], out[1.0])


def test_live_flux_field_is_read_at_the_next_step():
    """Item 4: values written into model.external_heat_fluxes.top between steps are used at the next step."""
    Nx, Ny = 64, 48
    h, a, hs, qt, qb, *_ = mixed_state(Nx, Ny, 29)
    m = thermo_model(grid(Nx, Ny), "fast", top_heat_flux=(csi.RadiativeEmission(), qt - 200.0), bottom_heat_flux=qb)
    csi.set_(m, h=h, aice=a)
    rh, ra, Tu = h, a, np.zeros_like(h)
    for n in range(6):
        q = qt - 200.0 + 30.0 * n
        m.copy_to_field(m.external_heat_fluxes.top, np.pad(q, 3))
        rh, ra, Tu, _ = R.slab_step(rh, ra, Tu, DT, [R.EMISSION, q], [qb], S=S_BOTTOM)
        csi.time_step(m, DT)
    m.synchronize()
    assert np.array_equal(m.ice_thickness.interior_numpy(), rh) and np.array_equal(m.ice_top_temperature.interior_numpy(), Tu)


@pytest.mark.parametrize("Rx, Ry", [(1, 2), (2, 2)])
def test_tiled_rk3_step_with_array_fluxes_and_emission(Rx, Ry):
    """Item 5: an RK3 step with EVP, WENO7 and the flux-term thermodynamics on an in-process tile group equals the untiled step."""
    c = cases.make_case(Nx=64, Ny=48, H=8, substeps=8, topo=("periodic", "periodic"), patches=True, random_uv=0.03)
    _, _, _, qt, qb, *_ = mixed_state(64, 48, 37)

    def build(tile=None, group=None):
        ice = csi.SlabThermodynamics(bottom_salinity=S_BOTTOM, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        return cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), tile=tile, local_group=group,
                               ice_thermodynamics=ice, top_heat_flux=(csi.RadiativeEmission(), qt - 200.0), bottom_heat_flux=qb)

    def state(m):
        m.synchronize()
        return [f.interior_numpy().copy() for f in (m.ice_thickness, m.ice_concentration, m.ice_top_temperature, m.velocities.u)]

    m = build()
    for n in range(2):
        csi.time_step(m, c["dt"])
    whole = state(m)

    def tile(rank, group):
        mt = build((Rx, Ry, rank), group)
        for n in range(2):
            csi.time_step(mt, c["dt"])
        return state(mt), mt.grid

    for (parts, g) in run_tile_threads(Rx * Ry, tile):
        for k, (x, y) in enumerate(zip(parts, whole)):
            ny, nx = x.shape
            assert np.array_equal(x, y[g.j_off:g.j_off + ny, g.i_off:g.i_off + nx]), k


def test_checkpoint_round_trip_with_emission():
    """Item 6: prognostic_state carries the top surface temperature; restoring it and stepping again gives the same bits."""
    Nx, Ny = 64, 48
    h, a, hs, qt, qb, *_ = mixed_state(Nx, Ny, 41)
    m = thermo_model(grid(Nx, Ny), "strict", top_heat_flux=(csi.RadiativeEmission(), qt - 200.0), bottom_heat_flux=qb)
    csi.set_(m, h=h, aice=a)
    for n in range(3):
        csi.time_step(m, DT)
    state = csi.prognostic_state(m)
    assert "ice_thermodynamics.top_surface_temperature" in state
    for n in range(3):
        csi.time_step(m, DT)
    first = csi.prognostic_state(m)
    m2 = thermo_model(grid(Nx, Ny), "strict", top_heat_flux=(csi.RadiativeEmission(), qt - 200.0), bottom_heat_flux=qb)
    csi.restore_prognostic_state(m2, state)
    for n in range(3):
        csi.time_step(m2, DT)
    second = csi.prognostic_state(m2)
    for k in first:
        if k != "clock":
            assert np.array_equal(first[k], second[k]), k
    assert np.abs(first["ice_thermodynamics.top_surface_temperature"]).max() > 0


def test_perpetual_night():
    """Item 7: examples/perpetual_night.jl's settings -- top flux (RadiativeEmission(), -200 W m^-2), h0 = 0.01, 960 one-hour
    steps -- on a grid of identical columns: the restatement bit for bit, h never decreases, the columns stay identical and the
    consolidated surface temperature stays below 0."""
    Nx, Ny = 8, 4
    g = grid(Nx, Ny)
    top_flux = csi.CenterField(g, "cuda:0", "top_flux")
    top_flux.set(-200.0)
    ice = csi.SlabThermodynamics(top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    m = csi.SeaIceModel(g, ice_thermodynamics=ice, top_heat_flux=(csi.RadiativeEmission(), top_flux), timestepper="ForwardEuler")
    csi.set_(m, h=0.01)
    h, a, Tu = np.full((Ny, Nx), 0.01), np.zeros((Ny, Nx)), np.zeros((Ny, Nx))
    hs = []
    for n in range(960):
        h, a, Tu, _ = R.slab_step(h, a, Tu, 3600.0, [R.EMISSION, np.full((Ny, Nx), -200.0)], [0.0])
        csi.time_step(m, 3600.0)
        if n % 48 == 47:
            m.synchronize()
            got = m.ice_thickness.interior_numpy()
            assert np.array_equal(got, h), n
            hs.append(got[0, 0])
    m.synchronize()
    got_h, got_T = m.ice_thickness.interior_numpy(), ice.top_surface_temperature.interior_numpy()
    assert np.array_equal(got_h, h) and np.array_equal(got_T, Tu) and np.array_equal(m.ice_concentration.interior_numpy(), a)
    assert np.all(np.diff(hs) >= 0) and hs[-1] > hs[0] > 0.01
    assert np.all(got_h == got_h[0, 0]) and np.all(got_T == got_T[0, 0])
    assert got_h[0, 0] >= 0.05 and got_T[0, 0] < 0


def test_2048_squared():
    """Item 8: one thermodynamic step with array fluxes and emission at 2048^2 equals the restatement; one whole RK3 step with EVP,
    WENO7 and that thermodynamics stays finite."""
    N = 2048
    h, a, hs, qt, qb, *_ = mixed_state(N, N, 43)
    top = (R.EMISSION, qt - 200.0)
    m = thermo_model(csi.RectilinearGrid((N, N), x=(0, 1), y=(0, 1), halo=(4, 4)), "fast", top_heat_flux=(csi.RadiativeEmission(), qt - 200.0),
                     bottom_heat_flux=qb)
    csi.set_(m, h=h, aice=a)
    csi.time_step(m, DT)
    rh, ra, Tu, _ = R.slab_step(h, a, np.zeros_like(h), DT, list(top), [qb], S=S_BOTTOM)
    m.synchronize()
    assert np.array_equal(m.ice_thickness.interior_numpy(), rh) and np.array_equal(m.ice_top_temperature.interior_numpy(), Tu)
    del m
    c = cases.make_case(Nx=N, Ny=N, substeps=20, topo=("periodic", "bounded"), patches=True, random_uv=0.02)
    ice = csi.SlabThermodynamics(bottom_salinity=S_BOTTOM, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), ice_thermodynamics=ice,
                        top_heat_flux=(csi.RadiativeEmission(), qt - 200.0), bottom_heat_flux=qb)
    csi.time_step(m, c["dt"])
    m.synchronize()
    for f in (m.velocities.u, m.velocities.v, m.ice_thickness, m.ice_concentration, m.ice_top_temperature):
        assert np.all(np.isfinite(f.interior_numpy()))
