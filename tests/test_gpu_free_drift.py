"""Prescribed free-drift velocity fields (`free_drift = (u, v)`, csi_free_drift_set(ctx, 2)) and StressBalanceFreeDrift as the model's
dynamics (csi_dynamics_set(ctx, 1)) on the GPU: against the C oracle and the test-side restatement (tests/free_drift_ref.py), on every
momentum path, on tiles, with the refusals.

Every prescribed-field case makes a band of rows marginal (free_drift_ref.marginal_band) and asserts, counted in the restatement,
that at least 10 % of its u points and of its v points take the marginal branch, and that the result differs from the same case run
with free_drift = None: a free-drift test on a state without marginal ice proves nothing."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import oracle as O
from free_drift_ref import FreeDriftRef, free_drift_arrays, free_drift_points, marginal_band, parent_like
from test_gpu_evp import EVP_FIELDS, cmp_region, gpu_fields
from test_gpu_local_tiles import check, reference, run_tile_threads, run_tiles

pytestmark = pytest.mark.gpu

KEEP = object()


@contextlib.contextmanager
def dynamics_replaced(free_drift=KEEP, as_dynamics=False, rheology=None, solver=None):
    """cases.csi_model builds its dynamics with csi.SeaIceMomentumEquation(g, ...): replace the `free_drift` keyword (a value, or a
    function of the model's grid -- a tile takes its slice), the rheology / solver, or the whole object by
    StressBalanceFreeDrift(top_momentum_stress, bottom_momentum_stress) built on the case's own stresses."""
    orig = csi.SeaIceMomentumEquation

    def dynamics(g, **k):
        if as_dynamics:
            return csi.StressBalanceFreeDrift(top_momentum_stress=k.get("top_momentum_stress"), bottom_momentum_stress=k.get("bottom_momentum_stress"))
        if free_drift is not KEEP:
            k["free_drift"] = free_drift(g) if callable(free_drift) else free_drift
        if rheology is not None:
            k["rheology"] = rheology
        if solver is not None:
            k["solver"] = solver
        return orig(g, **k)

    csi.SeaIceMomentumEquation = dynamics
    try:
        yield
    finally:
        csi.SeaIceMomentumEquation = orig


def model_of(case, free_drift=KEEP, as_dynamics=False, rheology=None, solver=None, **kw):
    with dynamics_replaced(free_drift, as_dynamics, rheology, solver):
        return cases.csi_model(case, **kw)


def fields_of(Fu, Fv):
    """dict(u=, v=) for the model's grid: the global interior arrays, or a tile's slices of them"""
    def make(g):
        if isinstance(g, csi.TileGrid):
            return dict(u=g.local_interior(Fu, csi.Face, csi.Center), v=g.local_interior(Fv, csi.Center, csi.Face))
        return dict(u=Fu, v=Fv)
    return make


def assert_marginal(p, least=0.10):
    """at least `least` of the u points and of the v points take the marginal branch and are not peripheral (a point with land in one
    of its two cells gets a signed zero, not the free drift: it does not count)"""
    fu, fv = free_drift_points(p, "u").mean(), free_drift_points(p, "v").mean()
    assert fu >= least and fv >= least, ("marginal u / v points", fu, fv)
    return fu, fv


def smooth_fields(p, seed=17, amp=0.04):
    """Free-drift velocities that are NOT the stress balance: smooth + noise, a few cm/s, interior-shaped."""
    rng = np.random.default_rng(seed)
    out = []
    for k in ("u", "v"):
        ny, nx = p.interior(k).shape
        X, Y = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny))
        out.append(amp * np.sin(2 * np.pi * (X + (k == "v") * 0.25)) * np.cos(2 * np.pi * Y) + 0.25 * amp * rng.standard_normal((ny, nx)))
    return out


def velocities(m):
    m.synchronize()
    return m.velocities.u.numpy().copy(), m.velocities.v.numpy().copy()


# ---- 1. prescribed fields that ARE the stress balance: EVP against the oracle's kind 1 -------------------------------------------------
ORACLE_CASES = {
    "omip_channel_land": dict(Nx=120, Ny=84, topo=("periodic", "bounded"), patches=True, random_uv=0.03, field_forcing=True, free_drift=True, land=0.25),
    "periodic_numbers": dict(Nx=64, Ny=48, patches=True, random_uv=0.05, ue=0.05, ve=-0.02, top=(0.03, -0.02), free_drift=True),
    "latlon": dict(Nx=60, Ny=44, grid="latlon", topo=("periodic", "bounded"), random_uv=0.03, field_forcing=True, free_drift=True),
    "curvilinear_points": dict(Nx=56, Ny=44, topo=("periodic", "bounded"), curvilinear=0.1, coriolis_points=True, random_uv=0.03,
                               field_forcing=True, free_drift=True),
    "folded": dict(Nx=64, Ny=48, topo=("periodic", "folded"), random_uv=0.03, field_forcing=True, free_drift=True),
}


def _oracle_setup(name, substeps):
    c = marginal_band(cases.make_case(substeps=substeps, **ORACLE_CASES[name]))
    p = cases.oracle_problem(c)                       # keeps free_drift_kind = 1
    assert_marginal(p)
    Fu, Fv = free_drift_arrays(p)
    return c, p, Fu, Fv


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_prescribed_fields_strict_bitwise_vs_oracle(name, oracle_lib):
    c, p, Fu, Fv = _oracle_setup(name, 7)
    m = model_of(c, free_drift=dict(u=Fu, v=Fv), mode="strict")
    p.initialize_rheology()
    m.ctx.call("csi_evp_initialize")
    m.copy_to_field(m.dynamics.auxiliaries.fields.P, p.f["P"])      # (P uses exp(): continue from the oracle's, as test_strict_bitwise_vs_oracle)
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    p.subcycle(c["dt"], 1, c["substeps"])
    p.L.ora_finalize_rheology(p.ptr)
    m.ctx.call("csi_evp_subcycle", c["dt"], c["substeps"], 1)
    m.ctx.call("csi_evp_finalize")
    g = gpu_fields(m)
    for k in ("u", "v", "s11", "s22", "s12"):
        assert np.all(np.isfinite(g[k])), k
        assert np.array_equal(g[k], p.f[k]), f"{name}: {k} differs, max abs diff {np.abs(g[k] - p.f[k]).max():.3e}"
    none = model_of(c, free_drift=None, mode="strict")
    none.ctx.call("csi_evp_initialize")
    none.ctx.call("csi_evp_subcycle", c["dt"], c["substeps"], 1)
    assert not np.array_equal(velocities(none)[0], g["u"])


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_prescribed_fields_fast_few_substeps_tight(name, k, oracle_lib):
    c, p, Fu, Fv = _oracle_setup(name, k)
    p.time_step_momentum(c["dt"])
    m = model_of(c, free_drift=dict(u=Fu, v=Fv), mode="fast")
    csi.time_step_momentum(m, c["dt"])
    g = gpu_fields(m)
    vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max())
    smax = max(np.abs(p.f["s11"]).max(), np.abs(p.f["s22"]).max(), np.abs(p.f["s12"]).max())
    for f in ("u", "v"):
        d = np.abs(g[f] - p.f[f]).max()
        print(name, k, f, d / vmax)
        assert d <= 1e-13 * vmax
        assert np.array_equal(g[f] == 0.0, p.f[f] == 0.0), (f, "zero sets differ")
    for f in ("s11", "s22", "s12"):
        assert np.abs(cmp_region(c, f, g[f]) - cmp_region(c, f, p.f[f])).max() <= 1e-10 * smax
    none = model_of(c, free_drift=None, mode="fast")
    csi.time_step_momentum(none, c["dt"])
    assert not np.array_equal(velocities(none)[0], g["u"])


@pytest.mark.parametrize("nsub", [4, 5])
@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_prescribed_fields_every_fusion_level_bitwise(name, nsub, oracle_lib):
    c, p, Fu, Fv = _oracle_setup(name, nsub)
    out, level = {}, {}
    for fusion in (0, 1, 2):
        m = model_of(c, free_drift=dict(u=Fu, v=Fv), mode="fast")
        m.set_fusion(fusion)
        csi.time_step_momentum(m, c["dt"])
        m.synchronize()
        level[fusion] = m.ctx.last_path()["level"]
        out[fusion] = {k: EVP_FIELDS[k](m).numpy().copy() for k in ("u", "v", "s11", "s22")}
    none = model_of(c, free_drift=None, mode="fast")
    csi.time_step_momentum(none, c["dt"])
    assert not np.array_equal(velocities(none)[0], out[2]["u"])
    kind1 = cases.csi_model(c, mode="fast")                  # the same case with StressBalanceFreeDrift(): the same paths
    csi.time_step_momentum(kind1, c["dt"])
    kind1.synchronize()
    assert level[0] == 0 and level[2] == kind1.ctx.last_path()["level"], level      # the paths StressBalanceFreeDrift() takes
    if name in ("omip_channel_land", "periodic_numbers"):
        assert level[2] == 2, level                                                # ... the two-sub-steps kernel among them
    for fusion in (1, 2):
        for k in out[0]:
            assert np.array_equal(out[0][k], out[fusion][k]), (name, nsub, fusion, k)
    # ... and kind 2 fed the stress balance equals kind 1, bit for bit
    for k in ("u", "v", "s11", "s22"):
        assert np.array_equal(out[2][k], EVP_FIELDS[k](kind1).numpy()), (name, k)


# ---- 2. prescribed fields that are NOT the stress balance ------------------------------------------------------------------------------
OTHER_CASES = {
    "periodic_fplane": dict(Nx=24, Ny=20, random_uv=0.03),
    "channel_wind_arrays": dict(Nx=22, Ny=20, topo=("periodic", "bounded"), wind_drag="arrays", bottom="arrays", random_uv=0.03),
    "masked_channel_forcing": dict(Nx=24, Ny=20, topo=("bounded", "bounded"), land=0.12, user_forcing=True, beta=2e-11, random_uv=0.03),
}
NU = 1000.0


def _same(m, p):
    u, v = velocities(m)
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(v))
    assert np.array_equal(u, p.f["u"]), float(np.abs(u - p.f["u"]).max())
    assert np.array_equal(v, p.f["v"]), float(np.abs(v - p.f["v"]).max())


def _other_setup(name, **kw):
    c = marginal_band(cases.make_case(**dict(OTHER_CASES[name], **kw)))
    p = cases.oracle_problem(c)
    Fu, Fv = smooth_fields(p)
    ref = FreeDriftRef(p, fields=(parent_like(p, "u", Fu), parent_like(p, "v", Fv)), nu=NU)
    assert_marginal(p)
    return c, p, Fu, Fv, ref


@pytest.mark.parametrize("substeps", [4, 5])
@pytest.mark.parametrize("name", sorted(OTHER_CASES))
def test_prescribed_fields_viscous_subcycle_strict_bitwise(name, substeps, oracle_lib):
    c, p, Fu, Fv, ref = _other_setup(name, substeps=substeps)
    kw = dict(rheology=csi.ViscousRheology(nu=NU), solver=csi.SplitExplicitSolver(substeps=substeps))
    m = model_of(c, free_drift=dict(u=Fu, v=Fv), mode="strict", **kw)
    csi.time_step_momentum(m, c["dt"])
    ref.time_step_momentum(c["dt"], substeps)
    _same(m, p)
    none = model_of(c, free_drift=None, mode="strict", **kw)
    csi.time_step_momentum(none, c["dt"])
    assert not np.array_equal(velocities(none)[0], p.f["u"])
    fast = model_of(c, free_drift=dict(u=Fu, v=Fv), mode="fast", **kw)
    csi.time_step_momentum(fast, c["dt"])
    vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max())
    for a, b in zip(velocities(fast), (p.f["u"], p.f["v"])):
        assert np.abs(a - b).max() <= 1e-12 * vmax                      # FAST within 1e-12 of max|u|


@pytest.mark.parametrize("rk", [False, True], ids=["fe", "rk"])
@pytest.mark.parametrize("name", sorted(OTHER_CASES))
def test_prescribed_fields_explicit_solver_strict_bitwise(name, rk, oracle_lib):
    c, p, Fu, Fv, ref = _other_setup(name)
    kw = dict(rheology=csi.ViscousRheology(nu=NU), solver=csi.ExplicitSolver(), timestepper="SplitRungeKutta3" if rk else "ForwardEuler")
    m = model_of(c, free_drift=dict(u=Fu, v=Fv), mode="strict", **kw)
    if rk:
        rng = np.random.default_rng(9)
        for k, fld in (("um", m.timestepper.Psi_minus.u), ("vm", m.timestepper.Psi_minus.v)):
            a = p.f[k[0]] + 0.01 * rng.standard_normal(p.f[k[0]].shape)
            p.f[k][...] = a
            m.copy_to_field(fld, a)
    dt = 60.0
    csi.compute_momentum_tendencies(m, dt)
    ref.compute_tendencies(dt)
    csi.time_step_momentum(m, dt, rk_reset=rk)
    ref.explicit_step(dt, rk_reset=rk)
    _same(m, p)
    none = model_of(c, free_drift=None, mode="strict", **kw)
    csi.compute_momentum_tendencies(none, dt)
    csi.time_step_momentum(none, dt, rk_reset=False)
    assert not np.array_equal(velocities(none)[0], p.f["u"])
    fast = model_of(c, free_drift=dict(u=Fu, v=Fv), mode="fast", **kw)
    if rk:
        fast.copy_to_field(fast.timestepper.Psi_minus.u, p.f["um"]); fast.copy_to_field(fast.timestepper.Psi_minus.v, p.f["vm"])
    csi.compute_momentum_tendencies(fast, dt)
    csi.time_step_momentum(fast, dt, rk_reset=rk)
    vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max())
    for a, b in zip(velocities(fast), (p.f["u"], p.f["v"])):
        assert np.abs(a - b).max() <= 1e-12 * vmax


EVP_OTHER = {
    "periodic": dict(Nx=64, Ny=48, random_uv=0.03),
    "channel_land_arrays": dict(Nx=120, Ny=84, topo=("periodic", "bounded"), random_uv=0.03, field_forcing=True, land=0.25),
    "folded_curvilinear": dict(Nx=64, Ny=48, topo=("periodic", "folded"), curvilinear=0.05, random_uv=0.03, field_forcing=True),
}


@pytest.mark.parametrize("mode,fusion", [("strict", 0), ("fast", 0), ("fast", 1), ("fast", 2)])
@pytest.mark.parametrize("name", sorted(EVP_OTHER))
def test_prescribed_fields_evp_marginal_points_hold_the_field(name, mode, fusion, oracle_lib):
    """h and aice do not move inside a sub-cycle: a marginal point takes the free-drift branch at every sub-step, so after the
    sub-cycle it holds F exactly (peripheral points a signed zero)."""
    c = marginal_band(cases.make_case(substeps=6, **EVP_OTHER[name]))
    p = cases.oracle_problem(c)
    ref = FreeDriftRef(p)
    assert_marginal(p)
    Fu, Fv = smooth_fields(p)
    m = model_of(c, free_drift=dict(u=Fu, v=Fv), mode=mode)
    m.set_fusion(fusion)
    csi.time_step_momentum(m, c["dt"])
    m.synchronize()
    Nx, Ny = c["Nx"], c["Ny"]
    for comp, F, fld in (("u", Fu, m.velocities.u), ("v", Fv, m.velocities.v)):
        got = fld.interior_numpy()[:Ny, :Nx]
        marg, per = ref.marginal(comp), ref.peripheral_points(comp)
        sel = marg & ~per
        assert sel.mean() >= 0.10
        assert np.array_equal(got[sel], F[:Ny, :Nx][sel]), (name, comp, mode, fusion)
        assert np.all(got[marg & per] == 0.0)
    none = model_of(c, free_drift=None, mode=mode)
    none.set_fusion(fusion)
    csi.time_step_momentum(none, c["dt"])
    assert not np.array_equal(velocities(none)[0], m.velocities.u.numpy())


def test_prescribed_fields_are_updated_in_place(oracle_lib):
    c = marginal_band(cases.make_case(Nx=64, Ny=48, substeps=4, random_uv=0.03))
    m = model_of(c, free_drift=dict(u=0.02, v=-0.01), mode="fast")
    csi.time_step_momentum(m, c["dt"])
    u1 = velocities(m)[0]
    m.free_drift_field("u").set(0.05)
    csi.time_step_momentum(m, c["dt"])
    u2 = velocities(m)[0]
    assert np.any(u1 == 0.02) and np.any(u2 == 0.05) and not np.any(u2 == 0.02)


# ---- 3. StressBalanceFreeDrift as the dynamics ---------------------------------------------------------------------------------------
DYN_CASES = {
    # semi-implicit bottom; explicit top a number pair, u_e / v_e numbers
    "periodic_numbers": dict(Nx=40, Ny=32, ue=0.05, ve=-0.02, top=(0.03, -0.02), random_uv=0.03),
    # ... u_e, v_e zero
    "channel_walls_zero_ue": dict(Nx=40, Ny=32, topo=("bounded", "bounded"), top=(0.02, 0.01), random_uv=0.03),
    # explicit top arrays, u_e / v_e arrays
    "channel_arrays": dict(Nx=40, Ny=32, topo=("periodic", "bounded"), field_forcing=True, random_uv=0.03),
    "masked_channel_arrays": dict(Nx=48, Ny=36, topo=("periodic", "bounded"), field_forcing=True, land=0.15, random_uv=0.03),
    "latlon_arrays": dict(Nx=40, Ny=32, grid="latlon", topo=("periodic", "bounded"), field_forcing=True, random_uv=0.03),
    "curvilinear_arrays": dict(Nx=40, Ny=32, curvilinear=0.15, field_forcing=True, random_uv=0.03),
    "folded_arrays": dict(Nx=40, Ny=32, topo=("periodic", "folded"), field_forcing=True, random_uv=0.03),
    # semi-implicit TOP (air velocities as arrays), explicit bottom arrays
    "top_semi_bottom_arrays": dict(Nx=40, Ny=32, topo=("periodic", "bounded"), wind_drag="arrays", bottom="arrays", random_uv=0.03),
    # the tau == 0 branch: a block of the stress arrays is exactly zero
    "channel_arrays_zero_block": dict(Nx=40, Ny=32, topo=("periodic", "bounded"), field_forcing=True, random_uv=0.03),
}


def _dyn_case(name, **kw):
    c = cases.make_case(**dict(DYN_CASES[name], free_drift=True, **kw))        # (free_drift: the oracle's closed forms need kind 1)
    if name.endswith("zero_block"):
        c["top_u"][8:20, :] = 0.0
        c["top_v"][8:21, :] = 0.0
    return c


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("name", sorted(DYN_CASES))
def test_free_drift_dynamics_step_bitwise(name, mode, oracle_lib):
    c = _dyn_case(name)
    p = cases.oracle_problem(c)
    ref = FreeDriftRef(p, dynamics=True)
    mag = ref.explicit_stress_magnitude("u")
    assert (mag != 0).mean() >= 0.10
    if name.endswith("zero_block"):
        assert (mag == 0).sum() > 0 and (ref.explicit_stress_magnitude("v") == 0).sum() > 0
    if "masked" in name:
        assert 1.0 - c["mask"].mean() >= 0.10
    m = model_of(c, as_dynamics=True, mode=mode)
    assert isinstance(m.dynamics, csi.StressBalanceFreeDrift) and m.substeps == 0
    u0 = velocities(m)[0]
    csi.compute_momentum_tendencies(m, c["dt"])                      # a no-op
    assert np.array_equal(velocities(m)[0], u0)
    csi.time_step_momentum(m, c["dt"])
    ref.free_drift_dynamics_step()
    _same(m, p)
    assert not np.array_equal(p.f["u"], u0)
    assert m.ctx.last_launches() == (1, 1)
    # independent of the incoming velocities (and of dt, rk_reset, the fusion switch)
    rng = np.random.default_rng(2)
    m.copy_to_field(m.velocities.u, rng.standard_normal(p.f["u"].shape))
    m.copy_to_field(m.velocities.v, rng.standard_normal(p.f["v"].shape))
    m.set_fusion(0)
    csi.time_step_momentum(m, 7.0 * c["dt"])
    u, v = velocities(m)
    s = p.s
    inner = (slice(s.Hy, s.Hy + s.Ny), slice(s.Hx, s.Hx + s.Nx))
    assert np.array_equal(u[inner], p.f["u"][inner]) and np.array_equal(v[inner], p.f["v"][inner])


SLAB = dict(top_heat_flux=-60.0, bottom_heat_flux=4.0, bottom_salinity=30.0, ice_salinity=5.0)


@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
@pytest.mark.parametrize("slab", [False, True], ids=["bare", "slab"])
@pytest.mark.parametrize("name", ["channel_arrays", "masked_channel_arrays"])
def test_free_drift_dynamics_whole_steps_strict_bitwise(name, stepper, slab, oracle_lib):
    c = _dyn_case(name, Nx=24, Ny=20)
    p = cases.oracle_problem(c)
    ref = FreeDriftRef(p, dynamics=True)
    kw, slab_o = {}, None
    if slab:
        kw["ice_thermodynamics"] = csi.SlabThermodynamics(top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance(), **SLAB)
        slab_o = O.make_slab(top_bc_kind=1, top_flux_kind=0, Qu=-60.0, Qb=4.0, salinity=30.0, ice_salinity=5.0)
    m = model_of(c, as_dynamics=True, mode="strict", timestepper=stepper, advection=csi.WENO(order=5), **kw)
    dt = 60.0
    for n in range(2):
        csi.time_step(m, dt)
        if stepper == "ForwardEuler":
            ref.time_step_fe(dt, 0, 5, False, first_iteration=(n == 0), slab=slab_o)
        else:
            ref.time_step_rk3(dt, 0, 5, False, slab=slab_o)
    m.synchronize()
    for k, fld in (("u", m.velocities.u), ("v", m.velocities.v), ("h", m.ice_thickness), ("aice", m.ice_concentration)):
        assert np.array_equal(fld.numpy(), p.f[k]), (k, float(np.abs(fld.numpy() - p.f[k]).max()))
    # prognostic_state / restore_prognostic_state work on such a model
    st = csi.prognostic_state(m)
    assert "u" in st and "Gn.h" in st and not any(k.startswith("dynamics.") for k in st)
    csi.time_step(m, dt)
    csi.restore_prognostic_state(m, st)
    assert np.array_equal(m.velocities.u.numpy(), p.f["u"]) and m.clock.iteration == 2


# ---- 4. tiles on one GPU -------------------------------------------------------------------------------------------------------------
TILE_CASES = {
    "2x2_channel_land_arrays": (2, 2, dict(Nx=256, Ny=192, topo=("periodic", "bounded"), land=0.2, field_forcing=True, free_drift=True)),
    "1x4_fold": (1, 4, dict(Nx=128, Ny=256, topo=("periodic", "folded"), curvilinear=0.04, field_forcing=True, free_drift=True)),
}


@pytest.mark.parametrize("k", [0, -1], ids=["peer", "rccl"])
@pytest.mark.parametrize("name", sorted(TILE_CASES))
def test_prescribed_fields_on_tiles_bitwise(name, k, oracle_lib):
    Rx, Ry, kw = TILE_CASES[name]
    c = marginal_band(cases.make_case(H=8, substeps=14, patches=True, random_uv=0.05, **kw))
    p = cases.oracle_problem(c)
    assert_marginal(p)
    Fu, Fv = smooth_fields(p)
    with dynamics_replaced(free_drift=fields_of(Fu, Fv)):
        mom, step = reference(c)                                  # two sub-cycles and one whole RK3 step, untiled
        tiles = run_tiles(c, Rx, Ry, k)
    with dynamics_replaced(free_drift=None):
        mom_none, _ = reference(c, full_step=False)
    assert not np.array_equal(mom["u"], mom_none["u"])
    for d in tiles:
        assert d["path"]["ranks"] == Rx * Ry and d["path"]["transport"] == ("peer" if k == 0 else "rccl"), d["path"]
        assert d["path"]["level"] == 2, d["path"]
    check(tiles, mom, step, (name, k))


@pytest.mark.parametrize("k", [0, -1], ids=["auto", "rccl"])
def test_prescribed_fields_on_tiles_with_all_eight_forcing_slots_bound(k, oracle_lib):
    """The coupled set-up: top stress arrays, ocean-velocity arrays, model.forcing arrays AND prescribed free-drift fields -- eight arrays
    whose halos travel between the tiles before every sub-cycle (two batches of the message exchange).  model.forcing with free
    drift has no instantiation of the two-sub-steps kernel: the three kernels run, on the message exchange."""
    Rx, Ry = 2, 2
    c = marginal_band(cases.make_case(H=8, substeps=14, patches=True, random_uv=0.05, Nx=256, Ny=192, topo=("periodic", "bounded"), land=0.2,
                                      field_forcing=True, user_forcing=True))
    p = cases.oracle_problem(c)
    assert_marginal(p)
    Fu, Fv = smooth_fields(p)
    with dynamics_replaced(free_drift=fields_of(Fu, Fv)):
        mom, step = reference(c)
        tiles = run_tiles(c, Rx, Ry, k)
    with dynamics_replaced(free_drift=None):
        mom_none, _ = reference(c, full_step=False)
    assert not np.array_equal(mom["u"], mom_none["u"])
    for d in tiles:
        assert d["path"]["ranks"] == Rx * Ry, d["path"]
    check(tiles, mom, step, ("eight slots", k))


@pytest.mark.parametrize("transport", ["peer", "rccl"])
@pytest.mark.parametrize("name", sorted(TILE_CASES))
def test_free_drift_dynamics_on_tiles_bitwise(name, transport, oracle_lib):
    Rx, Ry, kw = TILE_CASES[name]
    c = cases.make_case(H=8, patches=True, random_uv=0.05, **kw)

    def run(tile=None, group=None):
        extra = dict(tile=(Rx, Ry, tile), local_group=group) if tile is not None else {}
        m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), **extra)
        if tile is not None:                   # (the step's exchanges -- stress arrays, update_state! -- are messages on either setting)
            m.set_halo_transport(transport)
        csi.time_step_momentum(m, c["dt"])
        m.synchronize()
        res = {"mom_u": m.velocities.u.interior_numpy().copy(), "mom_v": m.velocities.v.interior_numpy().copy()}
        assert m.ctx.last_launches() == (1, 1)
        # the step fills no halo beyond a connected side (nor does the reference's: that is update_state!'s exchange, which ends every
        # stage of a time step) -- after a momentum step called on its own, before anything reads u, v across tiles:
        csi.update_state(m)
        csi.time_step(m, c["dt"])
        m.synchronize()
        res.update(step_u=m.velocities.u.interior_numpy().copy(), step_v=m.velocities.v.interior_numpy().copy(),
                   step_h=m.ice_thickness.interior_numpy().copy(), step_a=m.ice_concentration.interior_numpy().copy())
        g = m.grid
        res["offsets"] = (getattr(g, "i_off", 0), getattr(g, "j_off", 0), g.Nx, g.Ny)
        return res

    with dynamics_replaced(as_dynamics=True):
        whole = run()
        tiles = run_tile_threads(Rx * Ry, lambda rank, group: run(rank, group))
    assert np.abs(whole["mom_u"]).max() > 0 and not np.array_equal(whole["step_h"], c["h"])
    check(tiles, {f: whole[f"mom_{f}"] for f in ("u", "v")}, {f: whole[f"step_{f}"] for f in ("u", "v", "h", "a")}, name)


@pytest.mark.parametrize("mode", ["fast"])
def test_tile_activity_on_equals_off_with_prescribed_fields(mode, oracle_lib):
    """An ice-edge case (there for the activity cut, not for the branch: at least 1 % of its points marginal)."""
    c = cases.make_case(Nx=392, Ny=260, topo=("periodic", "bounded"), patches=True, random_uv=0.03, land=0.3, field_forcing=True,
                        ice_free_rows=(0.1, 0.6), substeps=12)
    marginal_band(c, rows=(0.60, 0.66))                           # thin ice along the edge
    p = cases.oracle_problem(c)
    assert_marginal(p, least=0.01)
    Fu, Fv = smooth_fields(p)
    out, acts = [], []
    for on in (True, False):
        m = model_of(c, free_drift=dict(u=Fu, v=Fv), mode=mode)
        m.set_tile_skipping(on)
        for step in range(3):
            csi.time_step_momentum(m, c["dt"])
            m.synchronize()
            if step == 0:
                acts.append(m.tile_activity())
        out.append([EVP_FIELDS[k](m).numpy().copy() for k in ("u", "v", "s11", "s22", "s12")])
    (tiles, live, used), (_, _, used_off) = acts
    assert used >= 1 and 0 < live < tiles and used_off == 0, acts     # something was skipped, something ran
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    none = model_of(c, free_drift=None, mode=mode)
    for _ in range(3):
        csi.time_step_momentum(none, c["dt"])
    assert not np.array_equal(velocities(none)[0], out[0][0])


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_kind_2_with_a_slot_unbound_is_refused_by_name():
    c = cases.make_case(Nx=32, Ny=24, substeps=4)
    m = model_of(c, free_drift=dict(u=0.01, v=0.02), mode="strict")
    L = m.ctx.L
    assert L.csi_field_bind(m.ctx.h, csi._lib.F["FREE_DRIFT_V"], None, 0, 0, 0) == 0
    assert L.csi_time_step_momentum(m.ctx.h, 60.0, 4, 0) == -2                     # CSI_ERR_NOT_BOUND
    assert b"free_drift_v" in L.csi_last_error(m.ctx.h)
    assert L.csi_free_drift_set(m.ctx.h, 3) == -1 and L.csi_free_drift_set(m.ctx.h, 2) == 0
    # kind 2 needs no SemiImplicitStress
    c2 = cases.make_case(Nx=32, Ny=24, substeps=4, bottom=None)
    m2 = model_of(c2, free_drift=dict(u=0.01, v=0.02), mode="strict")
    csi.time_step_momentum(m2, c2["dt"])
    assert np.all(np.isfinite(velocities(m2)[0]))


def test_free_drift_dynamics_refusals():
    c = cases.make_case(Nx=32, Ny=24)
    g = c["g"]
    semi = csi.SemiImplicitStress(ue=0.1)
    with pytest.raises(ValueError, match="not both"):
        csi.SeaIceModel(g, dynamics=csi.StressBalanceFreeDrift(top_momentum_stress=semi, bottom_momentum_stress=semi))
    with pytest.raises(ValueError, match="requires using a `SemiImplicitStress`"):
        csi.SeaIceModel(g, dynamics=csi.StressBalanceFreeDrift(top_momentum_stress=(0.01, 0.0)))
    # the library checks it too (a C or Julia caller), with the reference's wording
    m = csi.SeaIceModel(g, dynamics=csi.StressBalanceFreeDrift(top_momentum_stress=(0.01, 0.0), bottom_momentum_stress=semi))
    L, S = m.ctx.L, csi._lib.Stress
    both = S(kind=csi._lib.STRESS_SEMI_IMPLICIT, rho_e=1.3, Cd=1e-3)
    assert L.csi_stress_set(m.ctx.h, csi._lib.STRESS_TOP, C.byref(both)) == 0
    assert L.csi_time_step_momentum(m.ctx.h, 60.0, 0, 0) == -1 and b"not both" in L.csi_last_error(m.ctx.h)
    none = S(kind=csi._lib.STRESS_NONE)
    for side in (csi._lib.STRESS_TOP, csi._lib.STRESS_BOTTOM):
        assert L.csi_stress_set(m.ctx.h, side, C.byref(none)) == 0
    assert L.csi_time_step_momentum(m.ctx.h, 60.0, 0, 0) == -1 and b"requires using a `SemiImplicitStress`" in L.csi_last_error(m.ctx.h)
    assert L.csi_dynamics_set(m.ctx.h, 2) == -1 and b"unknown dynamics kind" in L.csi_last_error(m.ctx.h)
    assert L.csi_dynamics_set(m.ctx.h, 0) == 0 and L.csi_dynamics_set(m.ctx.h, 1) == 0


def test_viscous_rheology_on_a_tiled_context_is_still_refused():
    ctx = csi._lib.Context(0)
    met = csi._lib.Metrics()
    met.dx = met.dy = 1000.0
    ctx.call("csi_grid_set", 16, 16, 4, 4, csi._lib.PERIODIC, csi._lib.FULLY_CONNECTED, csi._lib.METRIC_UNIFORM, C.byref(met))
    ctx.call("csi_dynamics_set", csi._lib.DYNAMICS_FREE_DRIFT)
    assert ctx.L.csi_rheology_set(ctx.h, csi._lib.RHEOLOGY_VISCOUS, 1000.0) == -4 and b"ViscousRheology" in ctx.L.csi_last_error(ctx.h)
    ctx.close()
