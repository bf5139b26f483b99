"""Every store path leaves filled halos behind.

Every kernel that stores a prognostic field also writes that value's halo images (csrc/csi_dev.h store_with_images, which every
velocity kernel and the fills call, and its specialisations in advect.hip and evp_fused2.hip).  After a public entry that advances a field,
the returned parent must therefore be its own fill: tests/halo_ref.py's fill of the parent equals the parent on every SPECIFIED cell,
BIT FOR BIT.  Two conditions keep that from passing emptily: every point within H of an edge (a source of some image) changed its bits
between input and output, and that is asserted -- the inputs are chosen for it: ice everywhere above the minimum mass with
concentrations below one, seeded random velocities, non-zero stresses.  (The only points that may keep their bits are velocity
components ON a wall that a path holds at zero, before and after: their images are checked all the same.)

Paths: csi_time_step_momentum in STRICT; in FAST at fusion levels 0, 1, 2 with an even and an odd number of sub-steps (the pair kernel's
`single` mode stores too); csi_evp_subcycle from an even first sub-step (the u-first pair instantiations) and csi_evp_finalize; the
fold band; the viscous sub-cycle; the explicit u and v steps; StressBalanceFreeDrift as the dynamics; the tracer update followed by
csi_update_state (csi_dynamic_step_tracers itself leaves the halos to update_state!, as the reference's dynamic_time_step! does; inside
csi_time_step_fe / _rk3 its stores write the images); the one-launch-per-stage RK3 of an advection-only model at N = 2H, where the
scalar image form of advect.hip runs, and at N = 2H - 1, where it must decline and the general store runs; whole FE and RK3 steps.
Topologies (P,P), (B,B), (P,B) with ValueBoundaryConditions on u, and the north fold where the path takes one; halos (4,4), (5,3),
(3,5); grids just above 2H and one that crosses a 64-column block edge.  The kernel family csi_last_path / csi_last_advection reports is
asserted wherever csi_plan_pair or the fusion level determines it, so that a silent fall-back cannot make a case pass.
"""
import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import halo_ref as R
from test_gpu_free_drift import model_of
from test_gpu_unequal_halos import expected_level, hid, record_path

pytestmark = pytest.mark.gpu

HALOS = [(4, 4), (5, 3), (3, 5)]
VALUES = (0.02, -0.015)                     # ValueBoundaryCondition numbers of u on the south / north wall
TOPOS = {"PP": ("periodic", "periodic"), "BB": ("bounded", "bounded"), "PBv": ("periodic", "bounded"), "PF": ("periodic", "folded")}
LETTER = {"periodic": "P", "bounded": "B", "folded": "F"}
LOC = {"u": (R.FACE, R.CENTER), "v": (R.CENTER, R.FACE), "s11": (R.CENTER, R.CENTER), "s22": (R.CENTER, R.CENTER), "s12": (R.FACE, R.FACE),
       "h": (R.CENTER, R.CENTER), "aice": (R.CENTER, R.CENTER)}
EVP5 = ("u", "v", "s11", "s22", "s12")


def sizes_of(halo, topo):
    Hx, Hy = halo
    if topo == "PF":                        # (even Nx; Ny >= 3 Hy + 12: the smallest grid the fold band takes, csi_fold.hip)
        return [(2 * Hx + 2, 3 * Hy + 12), (70, 3 * Hy + 13)]
    return [(2 * Hx + 1, 2 * Hy + 2), (70, 2 * Hy + 3)]


def make(topo, halo, N, n, seed=3):
    c = cases.make_case(Nx=N[0], Ny=N[1], H=halo, topo=TOPOS[topo], substeps=n, patches=False, random_uv=0.05, seed=seed)
    rng = np.random.default_rng(seed + 100)
    c["a"] = 0.6 + 0.3 * rng.random(c["a"].shape)          # below one everywhere: a tracer update changes every cell
    kw = {}
    if topo == "PBv":
        V = csi.ValueBoundaryCondition
        kw["boundary_conditions"] = dict(u=csi.FieldBoundaryConditions(south=V(VALUES[0]), north=V(VALUES[1])), v=csi.FieldBoundaryConditions())
    return c, kw


def fields_of(m, names):
    aux = getattr(getattr(m.dynamics, "auxiliaries", None), "fields", None)
    get = {"u": lambda: m.velocities.u, "v": lambda: m.velocities.v, "h": lambda: m.ice_thickness, "aice": lambda: m.ice_concentration,
           "s11": lambda: aux.s11, "s22": lambda: aux.s22, "s12": lambda: aux.s12}
    return {k: get[k]() for k in names}


def seed_stresses(m, c):
    """Non-zero stresses with filled halos (what a previous momentum step leaves)."""
    rng = np.random.default_rng(c["Nx"] + 31 * c["Ny"])
    for k, f in fields_of(m, ("s11", "s22", "s12")).items():
        s = 40.0 * rng.standard_normal(tuple(f.interior().shape))
        if c.get("mask") is not None:
            # an immersed grid (Periodic x, no extra points): no stress on land, nor on a node that touches land -- the kernels leave
            # those alone, and a seeded value there would neither change nor matter
            wet = c["mask"].astype(bool)
            if k == "s12":
                south = np.vstack([np.zeros((1, wet.shape[1]), dtype=bool), wet[:-1]])
                wet = wet & np.roll(wet, 1, axis=1) & south & np.roll(south, 1, axis=1)
            s = np.where(wet, s, 0.0)
        f.set(s)
        m.ctx.call("csi_fill_halo_local", csi._lib.F[k.upper()])
    m.synchronize()


def snapshot(m, names):
    m.synchronize()
    return {k: f.numpy().copy() for k, f in fields_of(m, names).items()}


def assert_own_fill(c, topo, before, after, what):
    Nx, Ny, Hx, Hy = c["Nx"], c["Ny"], c["Hx"], c["Hy"]
    letters = LETTER[c["topo"][0]] + LETTER[c["topo"][1]]
    for k, a in after.items():
        loc = LOC[k]
        kw = dict(value_y=VALUES) if (topo == "PBv" and k == "u") else {}
        filled, cls = R.fill(a, Nx, Ny, Hx, Hy, loc, letters, fold_sign=-1 if k in ("u", "v") else 1, **kw)
        assert np.all(np.isfinite(a[cls != R.UNTOUCHED])), (what, k)
        bad = ~R.same_bits(filled, a) & (cls == R.SPECIFIED)
        assert (cls == R.SPECIFIED).any() or letters == "BB"
        if bad.any():
            j, i = np.argwhere(bad)[0]
            raise AssertionError(f"{what}: {k} is not its own fill on {bad.sum()} SPECIFIED cells, first at array [{j}, {i}]: "
                                 f"holds {a[j, i]!r}, its source gives {filled[j, i]!r}")
        # ... and the sources of those images changed: every point within H of an edge, except velocity components on a wall
        ny, nx = a.shape[0] - 2 * Hy, a.shape[1] - 2 * Hx
        jj, ii = np.meshgrid(np.arange(1, ny + 1), np.arange(1, nx + 1), indexing="ij")
        near = (ii <= Hx) | (ii > Nx - Hx) | (jj <= Hy) | (jj > Ny - Hy - (1 if letters[1] == "F" else 0))
        on_wall = np.zeros_like(near)
        if k == "u" and letters[0] == "B":
            on_wall |= (ii == 1) | (ii == Nx + 1)
        if k == "v" and letters[1] in "BF":
            on_wall |= (jj == 1) | (jj == Ny + 1)
        inner = (slice(Hy, Hy + ny), slice(Hx, Hx + nx))
        # (the explicit and free-drift steps do update column 1; on an immersed grid land and peripheral nodes stay zero as well)
        held = (on_wall | (c.get("mask") is not None)) & (before[k][inner] == 0.0) & (a[inner] == 0.0)
        same = R.same_bits(before[k][inner], a[inner]) & near & ~held
        assert not same.any(), (what, k, "points near an edge kept their bits", int(same.sum()), np.argwhere(same)[:4])


# ---- the momentum paths --------------------------------------------------------------------------------------------------------------
MOMENTUM = {
    "strict_n4": dict(mode="strict", fusion=2, n=4), "strict_n5": dict(mode="strict", fusion=2, n=5),
    "fast_f0_n4": dict(mode="fast", fusion=0, n=4), "fast_f0_n5": dict(mode="fast", fusion=0, n=5),
    "fast_f1_n4": dict(mode="fast", fusion=1, n=4), "fast_f1_n5": dict(mode="fast", fusion=1, n=5),
    "fast_f2_n4": dict(mode="fast", fusion=2, n=4), "fast_f2_n5": dict(mode="fast", fusion=2, n=5),
}


@pytest.mark.parametrize("halo", HALOS, ids=hid)
@pytest.mark.parametrize("topo", list(TOPOS))
@pytest.mark.parametrize("path", list(MOMENTUM))
def test_time_step_momentum_leaves_filled_halos(path, topo, halo):
    """csi_time_step_momentum (EVP, split-explicit): u, v and -- after finalize_rheology!'s fill -- sigma."""
    spec = MOMENTUM[path]
    for N in sizes_of(halo, topo):
        c, kw = make(topo, halo, N, spec["n"])
        m = cases.csi_model(c, mode=spec["mode"], **kw)
        m.set_fusion(spec["fusion"])
        seed_stresses(m, c)
        before = snapshot(m, EVP5)
        csi.time_step_momentum(m, c["dt"])
        after = snapshot(m, EVP5)
        level = m.ctx.last_path()["level"]
        what = f"time_step_momentum {path} {topo} {hid(halo)} N={N}"
        record_path("invariant", what, f"level {level}")
        assert level == expected_level(c, spec["mode"], spec["fusion"], spec["n"]), (what, level)
        assert_own_fill(c, topo, before, after, what)


@pytest.mark.parametrize("halo", HALOS, ids=hid)
@pytest.mark.parametrize("topo", list(TOPOS))
@pytest.mark.parametrize("n", [2, 3])
def test_subcycle_from_an_even_substep_leaves_filled_halos(n, topo, halo):
    """csi_evp_subcycle(dt, n, first = 2): the u-first instantiations of the pair kernel where it applies (n = 3: a pair and a u-first
    single).  The sub-cycle's own stores fill u and v; sigma's halos are finalize_rheology!'s, checked after csi_evp_finalize."""
    for N in sizes_of(halo, topo):
        c, kw = make(topo, halo, N, n)
        m = cases.csi_model(c, mode="fast", **kw)
        m.set_fusion(2)
        seed_stresses(m, c)
        m.ctx.call("csi_evp_initialize")
        before = snapshot(m, EVP5)
        m.ctx.call("csi_evp_subcycle", float(c["dt"]), n, 2)
        after = snapshot(m, EVP5)
        level = m.ctx.last_path()["level"]
        what = f"evp_subcycle first=2 n={n} {topo} {hid(halo)} N={N}"
        record_path("invariant", what, f"level {level}")
        assert level == expected_level(c, "fast", 2, n), (what, level)
        assert_own_fill(c, topo, before, {k: after[k] for k in ("u", "v")}, what)
        m.ctx.call("csi_evp_finalize")
        assert_own_fill(c, topo, before, snapshot(m, ("s11", "s22", "s12")), what + " + finalize")


@pytest.mark.parametrize("halo", [(4, 4), (5, 4), (4, 5)], ids=hid)
@pytest.mark.parametrize("n", [4, 5])
def test_fold_band_on_a_small_tripolar_grid_leaves_filled_halos(n, halo):
    """csi.TripolarGrid (curvilinear cap, analytic land, north fold) at the smallest height the band takes: the pair kernel below row
    Ny - Hy - 4, three kernels with the fold's images next to it (csi_fold.hip), and the same grid on the three kernels alone."""
    Hy = halo[1]
    for fusion in (2, 0):
        c = cases.make_case(Nx=32, Ny=3 * Hy + 12, H=halo, grid="tripolar", substeps=n, patches=False, random_uv=0.05)
        m = cases.csi_model(c, mode="fast")
        m.set_fusion(fusion)
        seed_stresses(m, c)
        before = snapshot(m, EVP5)
        csi.time_step_momentum(m, c["dt"])
        after = snapshot(m, EVP5)
        level = m.ctx.last_path()["level"]
        what = f"tripolar fold band n={n} fusion {fusion} {hid(halo)} N=({c['Nx']}, {c['Ny']})"
        record_path("invariant", what, f"level {level}")
        assert level == fusion == expected_level(c, "fast", fusion, n), (what, level)
        assert_own_fill(c, "PF", before, after, what)


VARIANTS = {
    "viscous_strict_n4": dict(mode="strict", rheology="viscous", n=4), "viscous_fast_n5": dict(mode="fast", rheology="viscous", n=5),
    "explicit_strict": dict(mode="strict", solver="explicit"), "explicit_fast": dict(mode="fast", solver="explicit"),
    "viscous_explicit_fast": dict(mode="fast", rheology="viscous", solver="explicit"),
    "free_drift_dynamics_strict": dict(mode="strict", as_dynamics=True), "free_drift_dynamics_fast": dict(mode="fast", as_dynamics=True),
}


@pytest.mark.parametrize("halo", HALOS, ids=hid)
@pytest.mark.parametrize("topo", ["PP", "BB", "PBv"])
@pytest.mark.parametrize("path", list(VARIANTS))
def test_momentum_variants_leave_filled_halos(path, topo, halo):
    """The viscous sub-cycle, the explicit u and v steps (momentum_viscous.hip, momentum_explicit.hip) and StressBalanceFreeDrift as the
    dynamics (momentum_free_drift.hip): all of them store through store_with_images."""
    spec = VARIANTS[path]
    for N in sizes_of(halo, topo):
        n = spec.get("n", 4)
        c, kw = make(topo, halo, N, n)
        m = model_of(c, as_dynamics=spec.get("as_dynamics", False),
                     rheology=csi.ViscousRheology(nu=1000.0) if spec.get("rheology") == "viscous" else None,
                     solver=csi.ExplicitSolver() if spec.get("solver") == "explicit" else (csi.SplitExplicitSolver(substeps=n) if "n" in spec else None),
                     mode=spec["mode"], **kw)
        before = snapshot(m, ("u", "v"))
        if spec.get("solver") == "explicit":
            if spec.get("rheology") != "viscous":
                seed_stresses(m, c)
            csi.compute_momentum_tendencies(m, c["dt"])
        csi.time_step_momentum(m, c["dt"])
        what = f"{path} {topo} {hid(halo)} N={N}"
        level = m.ctx.last_path()["level"]
        record_path("invariant", what, f"level {level}")
        assert level == 0, (what, level)                  # (none of these has a fused sub-cycle)
        assert_own_fill(c, topo, before, snapshot(m, ("u", "v")), what)


# ---- tracers -------------------------------------------------------------------------------------------------------------------------
def advection_for(halo):
    """WENO7 needs four halo layers in both directions, WENO5 three"""
    return (7, csi.WENO(order=7)) if min(halo) >= 4 else (5, csi.WENO(order=5))


@pytest.mark.parametrize("halo", HALOS, ids=hid)
@pytest.mark.parametrize("topo", ["PP", "BB", "PBv"])
def test_tracer_update_then_update_state_leaves_filled_halos(topo, halo):
    scheme, adv = advection_for(halo)
    for N in sizes_of(halo, topo):
        c, kw = make(topo, halo, N, 4)
        m = cases.csi_model(c, mode="fast", advection=adv, **kw)
        before = snapshot(m, ("h", "aice"))
        m.ctx.call("csi_compute_tracer_tendencies", scheme)
        m.ctx.call("csi_dynamic_step_tracers", float(c["dt"]), 0)
        m.ctx.call("csi_update_state")
        what = f"dynamic_step_tracers + update_state {topo} {hid(halo)} N={N}"
        last = m.ctx.last_advection()
        record_path("invariant", what, f"advection {last}")
        assert last["stage_fused"] == 0, (what, last)     # (the separate tendency and update kernels)
        assert_own_fill(c, topo, before, snapshot(m, ("h", "aice")), what)


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("halo", HALOS, ids=hid)
@pytest.mark.parametrize("topo", ["PP", "BB", "PBv"])
def test_rk3_advection_only_stage_leaves_filled_halos(topo, halo, mode):
    """The one-launch-per-stage RK3 of an advection-only model: at N = 2H the scalar image form of advect.hip ("N >= 2 H and no fold")
    runs; at N = 2H - 1 in either direction advect_stage_supported must decline and the separate kernels with the general store run.
    csi_last_advection says which."""
    Hx, Hy = halo
    scheme, adv = advection_for(halo)
    for N, staged in (((2 * Hx, 2 * Hy), 1), ((2 * Hx - 1, 2 * Hy), 0), ((2 * Hx, 2 * Hy - 1), 0), ((70, 2 * Hy + 1), 1)):
        c, _ = make(topo, halo, N, 4)
        rng = np.random.default_rng(5)
        m = csi.SeaIceModel(c["g"], dynamics=None, advection=adv, timestepper="SplitRungeKutta3", mode=mode)
        csi.set_(m, h=c["h"], aice=c["a"], u=c["u"] + 0.2 * rng.standard_normal(c["u"].shape) * (c["u"] != 0), v=c["v"] + 0.2 * rng.standard_normal(c["v"].shape) * (c["v"] != 0))
        before = snapshot(m, ("h", "aice"))
        csi.time_step(m, 300.0)
        last = m.ctx.last_advection()
        what = f"rk3 advection only {mode} {topo} {hid(halo)} N={N}"
        record_path("invariant", what, f"advection {last}")
        assert last["stage_fused"] == staged, (what, last)
        assert_own_fill(c, topo, before, snapshot(m, ("h", "aice")), what)


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
@pytest.mark.parametrize("halo", HALOS, ids=hid)
@pytest.mark.parametrize("topo", list(TOPOS))
def test_whole_steps_leave_filled_halos(topo, halo, stepper, mode):
    """csi_time_step_fe / csi_time_step_rk3 with EVP dynamics and WENO advection: u, v, sigma, h, aice.  Without a mask and without
    thermodynamics the tracer update's own stores write the images of h and aice (update_state! then fills the velocities only)."""
    scheme, adv = advection_for(halo)
    names = EVP5 + ("h", "aice")
    for N in sizes_of(halo, topo):
        c, kw = make(topo, halo, N, 4)
        m = cases.csi_model(c, mode=mode, timestepper=stepper, advection=adv, **kw)
        seed_stresses(m, c)
        before = snapshot(m, names)
        csi.time_step(m, c["dt"])
        level = m.ctx.last_path()["level"]
        what = f"{stepper} {mode} {topo} {hid(halo)} N={N}"
        record_path("invariant", what, f"level {level}, advection {m.ctx.last_advection()}")
        assert level == expected_level(c, mode, 2, 4), (what, level)
        assert_own_fill(c, topo, before, snapshot(m, names), what)
