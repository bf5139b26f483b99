"""ViscousRheology and the ExplicitSolver on the GPU: STRICT bit for bit against the test-side restatement (tests/momentum_ref.py,
composed with the C oracle's tracer pieces for whole steps), FAST against STRICT, the reference's own tests restated, the launch
structure, the refused configurations and the unchanged EVP default."""
import ctypes as C

import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import oracle as O
from momentum_ref import Ref

pytestmark = pytest.mark.gpu


def model_of(case, rheology=None, solver=None, **kw):
    """cases.csi_model with the dynamics' rheology / solver replaced (the rest of the case as cases.py builds it)."""
    orig = csi.SeaIceMomentumEquation

    def dynamics(g, **k):
        if rheology is not None:
            k["rheology"] = rheology
        if solver is not None:
            k["solver"] = solver
        return orig(g, **k)

    csi.SeaIceMomentumEquation = dynamics
    try:
        return cases.csi_model(case, **kw)
    finally:
        csi.SeaIceMomentumEquation = orig


IBC = ((0.02, -0.03, 0.01, 0.04), (0.03, 0.01, -0.02, 0.02))
# (name, make_case keywords): every case crosses a Coriolis kind, a stress kind, free drift or user forcing
CASES = [
    ("periodic_fplane", dict(Nx=24, Ny=20, random_uv=0.03)),
    ("periodic_none_forcing", dict(Nx=24, Ny=20, random_uv=0.03, coriolis=None, user_forcing=True, free_drift=True)),
    ("channel_noslip_beta", dict(Nx=24, Ny=20, topo=("bounded", "bounded"), noslip=True, beta=2e-11, random_uv=0.03)),
    ("channel_wind_arrays", dict(Nx=22, Ny=18, topo=("periodic", "bounded"), wind_drag="arrays", bottom="arrays", random_uv=0.03)),
    ("latlon_rows", dict(Nx=24, Ny=20, grid="latlon", random_uv=0.03, user_forcing=True)),
    ("latlon_fields_free_drift", dict(Nx=24, Ny=20, grid="latlon", topo=("periodic", "bounded"), field_forcing=True, free_drift=True, random_uv=0.03)),
    ("curvilinear_points", dict(Nx=24, Ny=20, curvilinear=0.15, coriolis_points=True, random_uv=0.03)),
    ("masked_immersed", dict(Nx=24, Ny=20, land=0.15, immersed_bc=IBC, random_uv=0.03, wind_drag="numbers", coriolis=None)),
    ("masked_channel_forcing", dict(Nx=24, Ny=20, topo=("bounded", "bounded"), land=0.12, immersed_bc=IBC, user_forcing=True,
                                    free_drift=True, beta=2e-11, random_uv=0.03)),
]
NU = 1000.0


def _same(model, p, keys=("u", "v")):
    model.synchronize()
    fields = {"u": model.velocities.u, "v": model.velocities.v, "h": model.ice_thickness, "aice": model.ice_concentration}
    for k in keys:
        a, b = fields[k].numpy(), p.f[k]
        assert np.all(np.isfinite(a)), k
        assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))


@pytest.mark.parametrize("substeps", [4, 5])
@pytest.mark.parametrize("name,kw", CASES, ids=[n for n, _ in CASES])
def test_viscous_subcycle_strict_bitwise(name, kw, substeps, oracle_lib):
    c = cases.make_case(substeps=substeps, **kw)
    p = cases.oracle_problem(c)
    ref = Ref(p, nu=NU)
    m = model_of(c, rheology=csi.ViscousRheology(nu=NU), solver=csi.SplitExplicitSolver(substeps=substeps), mode="strict")
    u0 = m.velocities.u.numpy().copy()
    csi.time_step_momentum(m, c["dt"])
    ref.time_step_momentum(c["dt"], substeps)
    _same(m, p)
    assert not np.array_equal(m.velocities.u.numpy(), u0)
    assert m.ctx.last_launches() == (2 * substeps, substeps)        # one u and one v launch per sub-step
    assert m.ctx.launches_per_substep() == 2


def _set_sigma(m, p, seed):
    rng = np.random.default_rng(seed)
    f = m.dynamics.auxiliaries.fields
    for k, fld in (("s11", f.s11), ("s22", f.s22), ("s12", f.s12), ("un", f.un), ("vn", f.vn)):
        a = 50.0 * rng.standard_normal(p.f[k].shape) if k.startswith("s") else 0.02 * rng.standard_normal(p.f[k].shape)
        p.f[k][...] = a
        m.copy_to_field(fld, a)


@pytest.mark.parametrize("viscous", [True, False], ids=["viscous", "evp"])
@pytest.mark.parametrize("name,kw", [CASES[0], CASES[3], CASES[6], CASES[8]], ids=[CASES[k][0] for k in (0, 3, 6, 8)])
@pytest.mark.parametrize("rk", [False, True], ids=["fe", "rk"])
def test_explicit_tendency_and_step_strict_bitwise(name, kw, viscous, rk, oracle_lib):
    c = cases.make_case(**kw)
    p = cases.oracle_problem(c)
    ref = Ref(p, nu=NU, viscous=viscous)
    m = model_of(c, rheology=csi.ViscousRheology(nu=NU) if viscous else None, solver=csi.ExplicitSolver(), mode="strict",
                 timestepper="SplitRungeKutta3" if rk else "ForwardEuler")
    if not viscous:
        _set_sigma(m, p, 5)
    if rk:                                            # u^- = Psi^-: a different state than u
        rng = np.random.default_rng(9)
        for k, fld in (("um", m.timestepper.Psi_minus.u), ("vm", m.timestepper.Psi_minus.v)):
            a = p.f[k[0]] + 0.01 * rng.standard_normal(p.f[k[0]].shape)
            p.f[k][...] = a
            m.copy_to_field(fld, a)
    dt = 60.0
    csi.compute_momentum_tendencies(m, dt)
    ref.compute_tendencies(dt)
    m.synchronize()
    assert np.array_equal(m.timestepper.Gn.u.numpy(), ref.Gu) and np.array_equal(m.timestepper.Gn.v.numpy(), ref.Gv)
    assert np.abs(ref.Gu).max() > 0
    csi.time_step_momentum(m, dt, rk_reset=rk)
    ref.explicit_step(dt, rk_reset=rk)
    _same(m, p)


SLAB = dict(top_heat_flux=-60.0, bottom_heat_flux=4.0, bottom_salinity=30.0, ice_salinity=5.0)


@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
@pytest.mark.parametrize("combo", ["evp_explicit", "viscous_explicit", "viscous_split"])
@pytest.mark.parametrize("slab", [False, True], ids=["bare", "slab"])
def test_whole_steps_strict_bitwise(stepper, combo, slab, oracle_lib):
    c = cases.make_case(Nx=20, Ny=16, topo=("periodic", "bounded"), substeps=3, random_uv=0.03, u0=0.05)
    p = cases.oracle_problem(c)
    viscous, explicit = combo.startswith("viscous"), combo.endswith("explicit")
    ref = Ref(p, nu=NU, viscous=viscous)
    kw = {}
    slab_o = None
    if slab:
        kw["ice_thermodynamics"] = csi.SlabThermodynamics(top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance(), **SLAB)
        slab_o = O.make_slab(top_bc_kind=1, top_flux_kind=0, Qu=-60.0, Qb=4.0, salinity=30.0, ice_salinity=5.0)
    m = model_of(c, rheology=csi.ViscousRheology(nu=NU) if viscous else None,
                 solver=csi.ExplicitSolver() if explicit else csi.SplitExplicitSolver(substeps=3), mode="strict",
                 timestepper=stepper, advection=csi.WENO(order=5), **kw)
    dt = 60.0
    for n in range(2):
        csi.time_step(m, dt)
        if stepper == "ForwardEuler":
            ref.time_step_fe(dt, 3, 5, explicit, first_iteration=(n == 0), slab=slab_o)
        else:
            ref.time_step_rk3(dt, 3, 5, explicit, slab=slab_o)
    _same(m, p, ("u", "v", "h", "aice"))


@pytest.mark.parametrize("name,kw", CASES, ids=[n for n, _ in CASES])
def test_fast_matches_strict(name, kw):
    out = {}
    for mode in ("strict", "fast"):
        c = cases.make_case(substeps=6, **kw)
        m = model_of(c, rheology=csi.ViscousRheology(nu=NU), solver=csi.SplitExplicitSolver(substeps=6), mode=mode)
        csi.time_step_momentum(m, c["dt"])
        me = model_of(c, rheology=csi.ViscousRheology(nu=NU), solver=csi.ExplicitSolver(), mode=mode)
        csi.compute_momentum_tendencies(me, 60.0)
        csi.time_step_momentum(me, 60.0)
        m.synchronize(); me.synchronize()
        out[mode] = [f.numpy().copy() for f in (m.velocities.u, m.velocities.v, me.velocities.u, me.velocities.v)]
    for k in (0, 2):
        vmax = max(np.abs(out["strict"][k]).max(), np.abs(out["strict"][k + 1]).max())
        for q in (k, k + 1):
            d = np.abs(out["fast"][q] - out["strict"][q]).max()
            assert np.isfinite(d) and d <= 1e-12 * vmax, (name, q, d, vmax)     # FAST within 1e-12 of max|u|


# ---- the reference's own tests, restated ---------------------------------------------------------------------------------------------
def _matrix():
    out = []
    for cor in ("none", "fplane", "betaplane"):
        for adv in ("weno", "upwind5"):
            for rheo in ("evp", "viscous"):
                for thermo in ("none", "slab", "slab_snow"):          # (a snow layer needs ice thermodynamics here)
                    for solver in ("explicit", "split"):
                        out.append((cor, adv, rheo, thermo, solver))
    return out


@pytest.mark.parametrize("cor,adv,rheo,thermo,solver", _matrix())
def test_reference_time_stepping_matrix(cor, adv, rheo, thermo, solver):
    """test/test_time_stepping.jl:22-54 on its 2-D grid: one step of 1.1 s from the default state, finite fields, clock advanced."""
    g = csi.RectilinearGrid((10, 10), x=(0.0, 1.0), y=(0.0, 1.0), topology=(csi.Bounded, csi.Bounded))
    coriolis = {"none": None, "fplane": csi.FPlane(latitude=45), "betaplane": csi.BetaPlane(latitude=45)}[cor]
    dyn = csi.SeaIceMomentumEquation(g, coriolis=coriolis,
                                     rheology=csi.ElastoViscoPlasticRheology() if rheo == "evp" else csi.ViscousRheology(nu=1000),
                                     solver=csi.ExplicitSolver() if solver == "explicit" else csi.SplitExplicitSolver())
    kw = {}
    if thermo != "none":
        kw["ice_thermodynamics"] = csi.SlabThermodynamics()
    if thermo == "slab_snow":
        kw["snow_thermodynamics"] = csi.snow_slab_thermodynamics(g)
    m = csi.SeaIceModel(g, dynamics=dyn, advection=csi.WENO() if adv == "weno" else csi.UpwindBiased(order=5), **kw)
    if thermo == "slab_snow":
        csi.set_(m, h=1.0, aice=1.0, hs=0.1)
    csi.time_step(m, 1.1)
    m.synchronize()
    assert m.clock.iteration == 1 and m.clock.time == 1.1
    for f in (m.velocities.u, m.velocities.v, m.ice_thickness, m.ice_concentration):
        assert np.all(np.isfinite(f.numpy()))


@pytest.mark.parametrize("rheo", ["evp", "viscous"])
@pytest.mark.parametrize("solver", ["explicit", "split"])
def test_reference_ocean_drag(rheo, solver):
    """test/test_time_stepping.jl:56-80 (EVP as there, and again with ViscousRheology): 0 < max u <= u_o after 20 steps of 60 s."""
    g = csi.RectilinearGrid((8, 8), x=(0.0, 10_000.0), y=(0.0, 10_000.0), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
    uo = 0.1
    dyn = csi.SeaIceMomentumEquation(g, bottom_momentum_stress=csi.SemiImplicitStress(ue=uo),
                                     rheology=csi.ElastoViscoPlasticRheology() if rheo == "evp" else csi.ViscousRheology(nu=1000),
                                     solver=csi.ExplicitSolver() if solver == "explicit" else csi.SplitExplicitSolver(substeps=10))
    m = csi.SeaIceModel(g, dynamics=dyn)
    csi.set_(m, h=1.0, aice=1.0, u=0.0, v=0.0)
    for _ in range(20):
        csi.time_step(m, 60.0)
    m.synchronize()
    u = m.velocities.u.interior_numpy()
    assert np.all(np.isfinite(u))
    assert u.max() > 0
    assert u.max() <= uo


def test_reference_viscous_momentum_equation_runs():
    """test/test_sea_ice_advection.jl:58-73."""
    g = csi.RectilinearGrid((10, 10), x=(0.0, 1.0), y=(0.0, 1.0), topology=(csi.Bounded, csi.Bounded))
    dyn = csi.SeaIceMomentumEquation(g, rheology=csi.ViscousRheology(nu=1000))
    m = csi.SeaIceModel(g, dynamics=dyn, ice_thermodynamics=None, advection=csi.WENO())
    assert m.velocities.u is not None and m.velocities.v is not None
    csi.time_step(m, 1.0)
    m.synchronize()
    assert np.all(np.isfinite(m.velocities.u.numpy())) and m.clock.iteration == 1


# ---- refused configurations, unchanged default ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("topo_y", [csi._lib.FULLY_CONNECTED, csi._lib.RIGHT_FOLDED], ids=["tiled", "folded"])
def test_tiled_and_folded_contexts_refuse_the_new_rheology_and_solver(topo_y):
    ctx = csi._lib.Context(0)
    met = csi._lib.Metrics()
    met.dx = met.dy = 1000.0
    ctx.call("csi_grid_set", 16, 16, 4, 4, csi._lib.PERIODIC, topo_y, csi._lib.METRIC_UNIFORM, C.byref(met))
    L = ctx.L
    assert L.csi_rheology_set(ctx.h, csi._lib.RHEOLOGY_VISCOUS, 1000.0) == -4
    assert b"ViscousRheology" in L.csi_last_error(ctx.h)
    assert L.csi_momentum_solver_set(ctx.h, csi._lib.SOLVER_EXPLICIT) == -4
    assert b"ExplicitSolver" in L.csi_last_error(ctx.h)
    assert L.csi_rheology_set(ctx.h, csi._lib.RHEOLOGY_EVP, 0.0) == 0 and L.csi_momentum_solver_set(ctx.h, csi._lib.SOLVER_SPLIT_EXPLICIT) == 0
    ctx.close()


def test_folded_model_with_viscous_rheology_is_refused():
    g = csi.TripolarGrid((32, 24), halo=(4, 4))
    dyn = csi.SeaIceMomentumEquation(g, rheology=csi.ViscousRheology(nu=1000))
    with pytest.raises(csi.CsiError, match="ViscousRheology is not supported"):
        csi.SeaIceModel(g, dynamics=dyn)


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_evp_default_unchanged_by_the_new_entry_points(mode):
    c = cases.make_case(Nx=48, Ny=40, substeps=8, random_uv=0.02)
    out = []
    for toggle in (False, True):
        m = cases.csi_model(c, mode=mode)
        if toggle:                                     # visit the other settings and come back to the defaults
            m.ctx.call("csi_rheology_set", csi._lib.RHEOLOGY_VISCOUS, 123.0)
            m.ctx.call("csi_momentum_solver_set", csi._lib.SOLVER_EXPLICIT)
            m.ctx.call("csi_rheology_set", csi._lib.RHEOLOGY_EVP, 0.0)
            m.ctx.call("csi_momentum_solver_set", csi._lib.SOLVER_SPLIT_EXPLICIT)
            m.ctx.call("csi_compute_momentum_tendencies", 120.0)       # a no-op for the split-explicit solver
        csi.time_step_momentum(m, c["dt"])
        m.synchronize()
        out.append([f.numpy().copy() for f in (m.velocities.u, m.velocities.v, m.dynamics.auxiliaries.fields.s11)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name,kw", [CASES[3], CASES[6]], ids=[CASES[3][0], CASES[6][0]])
def test_fast_matches_strict_evp_explicit(name, kw):
    """k_tendencies<FAST, EVP> and the FAST explicit steps against STRICT, on stored stresses that are not zero."""
    out = {}
    rng = np.random.default_rng(21)
    sig = None
    for mode in ("strict", "fast"):
        c = cases.make_case(**kw)
        m = model_of(c, solver=csi.ExplicitSolver(), mode=mode)
        f = m.dynamics.auxiliaries.fields
        if sig is None:
            sig = {k: (50.0 if k.startswith("s") else 0.02) * rng.standard_normal(getattr(f, k).numpy().shape) for k in ("s11", "s22", "s12", "un", "vn")}
        for k, a in sig.items():
            m.copy_to_field(getattr(f, k), a)
        csi.compute_momentum_tendencies(m, 60.0)
        csi.time_step_momentum(m, 60.0)
        m.synchronize()
        out[mode] = [x.numpy().copy() for x in (m.timestepper.Gn.u, m.timestepper.Gn.v, m.velocities.u, m.velocities.v)]
    for k in (0, 2):
        vmax = max(np.abs(out["strict"][k]).max(), np.abs(out["strict"][k + 1]).max())
        assert vmax > 0
        for q in (k, k + 1):
            d = np.abs(out["fast"][q] - out["strict"][q]).max()
            assert np.isfinite(d) and d <= 1e-12 * vmax, (name, q, d, vmax)


@pytest.mark.parametrize("topo,copies", [(("periodic", "periodic"), 1), (("bounded", "bounded"), 2)], ids=["periodic", "walls"])
def test_viscous_subcycle_launches_in_a_kernel_trace(topo, copies, tmp_path):
    """What the device ran, not what the host counted: a kernel trace of one viscous sub-cycle with an odd number of sub-steps holds
    exactly 2 x substeps velocity launches and at most one copy batch at the end (walls: a second one before the sub-cycle, which
    brings the cells beyond the walls -- that no store reaches -- into the second array)."""
    import glob
    import os
    import shutil
    import subprocess
    import sys
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        pytest.skip("no rocprofv3")
    sub = 5
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "momentum_launch_child.py")
    r = subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path), "-o", "trace", "--",
                        sys.executable, child, topo[0], topo[1], str(sub)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    files = glob.glob(os.path.join(str(tmp_path), "**", "*kernel_trace.csv"), recursive=True)
    assert files, r.stdout[-1000:]
    text = open(files[0]).read()
    assert text.count("k_visc_ustep") == sub and text.count("k_visc_vstep") == sub
    assert text.count("k_copy_batch") == copies
