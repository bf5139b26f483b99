"""The advected tracers on the GPU (csrc/tracers.hip, csrc/csi_tracers.hip; include/csi.h "advected ice tracers and ice age") against the
NumPy restatement of tests/tracers_ref.py and, for a plain nonnegative tracer, against the oracle's snow thickness.

STRICT: G and c bit for bit.  FAST: G within G_TOL (tests/test_gpu_steps.py) of the oracle's, c bit for bit against the restatement fed
the device's own G (and, where a tracer is weighted, the device's own aice tendency).  Every test asserts the launch counts and the
reported layout before it looks at values."""
import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import output_ref
import tracers_ref as tr
from test_gpu_steps import G_TOL

pytestmark = pytest.mark.gpu
_L = csi._lib
SHAPES = {"one_column_last_block": (37, 29), "fewer_rows_than_a_tile": (127, 23), "narrow_rows": (130, 9), "exact_multiples": (128, 24)}
TOPOS = {"pp": ("periodic", "periodic"), "bb": ("bounded", "bounded"), "pb": ("periodic", "bounded")}
METRICS = [dict(grid="rectilinear"), dict(grid="latlon"), dict(grid="rectilinear", curvilinear=0.05)]
SCHEMES = (7, 5, 3, -5, -3, 1)
TX, TY = 63, 7
POISON = 1e300
UNSUPPORTED = -4          # CSI_ERR_UNSUPPORTED (include/csi.h)


def advection_of(scheme, weight_dtype="f64"):
    return csi.WENO(order=scheme, weight_dtype=weight_dtype) if scheme > 0 and scheme != 1 else csi.UpwindBiased(order=abs(scheme))


def flow_case(Nx, Ny, topo, metric=0, land=True, seed=5, cfl=0.2, H=4, **kw):
    """seeded divergent velocities with |U| dt / dx <= cfl, aice in [0.2, 0.9] with an open-water patch, hand-placed land: a block in
    the interior, cells on the first and last column and row, a cell in a corner"""
    rng = np.random.default_rng(seed)
    c = cases.make_case(Nx=Nx, Ny=Ny, H=H, topo=topo, spacing=1000.0, patches=False, noise=0.0, top=None, bottom=None, coriolis=None,
                        **dict(METRICS[metric], **kw))
    g = c["g"]
    dxmin = 1000.0 if metric == 0 else float(np.min(g.metrics()["dxc" if metric == 1 else "dxcc"]))
    vmax = cfl * dxmin / c["dt"]
    c["u"] = vmax * (2 * rng.random(c["u"].shape) - 1)
    c["v"] = vmax * (2 * rng.random(c["v"].shape) - 1)
    if topo[0] == "bounded":
        c["u"][:, 0] = 0.0; c["u"][:, -1] = 0.0
    if topo[1] in ("bounded", "folded"):
        c["v"][0, :] = 0.0
    if topo[1] == "bounded":
        c["v"][-1, :] = 0.0
    wet = np.ones((Ny, Nx), bool) if c["mask"] is None else c["mask"].astype(bool)
    if land:
        wet[Ny // 3:Ny // 3 + 3, Nx // 4:Nx // 4 + 5] = False
        wet[2, 0] = wet[Ny - 3, Nx - 1] = wet[0, Nx // 2] = wet[Ny - 1, Nx // 3] = wet[0, 0] = False
        c["mask"] = wet
    c["a"] = np.where(wet, 0.2 + 0.7 * rng.random((Ny, Nx)), 0.0)
    c["a"][Ny // 2:Ny // 2 + 2, Nx // 2:Nx // 2 + 6] = 0.0
    c["h"] = np.where(c["a"] > 0, 0.3 + 0.2 * rng.random((Ny, Nx)), 0.0)
    c["values"] = [np.where(wet, 0.1 + rng.random((Ny, Nx)), 0.0) for _ in range(8)]
    return c


SPECS8 = [("plain", None, True, 0.0), ("age", "concentration", True, 1.0), ("signed", None, False, -2e-3), ("wsigned", "concentration", False, 5e-4),
          ("p4", None, True, 1e-3), ("w5", "concentration", True, 0.0), ("p6", None, True, 0.0), ("w7", "concentration", True, 2.0)]


def specs_of(n, names=None):
    return [csi.Tracer(nm, weighting=w, nonnegative=nn, source=s) for nm, w, nn, s in SPECS8[:n]]


def model_of(c, specs, mode="strict", stepper="SplitRungeKutta3", scheme=7, weight_dtype="f64", dynamics=False, values=None, **kw):
    """prescribed velocities (dynamics = nothing) unless dynamics: the EVP model of tests/cases.py"""
    if dynamics:
        m = cases.csi_model(c, mode=mode, timestepper=stepper, advection=advection_of(scheme, weight_dtype), tracers=specs, **kw)
    else:
        m = csi.SeaIceModel(c["g"], advection=advection_of(scheme, weight_dtype), timestepper=stepper, mode=mode, tracers=specs, **kw)
        if c.get("mask") is not None:
            m.set_mask(c["mask"])
        csi.set_(m, h=c["h"], aice=c["a"], u=c["u"], v=c["v"])
    values = c["values"] if values is None else values
    csi.set_(m, **{s.name: values[k] for k, s in enumerate(specs)})
    return m


def ref_of(c, specs, values=None):
    p = cases.oracle_problem(c)
    values = c["values"] if values is None else values
    return p, [tr.tracer(p, values[k], weighted=s.weighting is not None, nonneg=s.nonnegative, source=s.source) for k, s in enumerate(specs)]


def inactive_parent(p):
    """parent elements no stencil may read: immersed cells and their images, everything beyond a wall, and the halo corners (outside the
    interior in both directions: no x or y line through an interior cell reaches them, periodic or not)"""
    s = p.s
    bad = (p._mask == 0) if s.has_mask else np.zeros(p.f["h"].shape, bool)
    for rows in (slice(0, s.Hy), slice(s.Hy + s.Ny, None)):
        for cols in (slice(0, s.Hx), slice(s.Hx + s.Nx, None)):
            bad[rows, cols] = True
    import oracle as O
    if s.topo_x == O.BOUNDED:
        bad[:, :s.Hx] = True; bad[:, s.Hx + s.Nx:] = True
    if s.topo_y == O.BOUNDED:
        bad[:s.Hy, :] = True; bad[s.Hy + s.Ny:, :] = True
    return bad


def expected_layout(n, force=0):
    ntr = force if force else (4 if n >= 3 else n)
    return dict(tracers_per_thread=ntr, tile_x=TX, tile_y=TY, groups=-(-n // ntr))


def same_G(mode, got, want, what):
    assert np.all(np.isfinite(got)), what
    if mode == "strict":
        assert np.array_equal(got, want), (what, np.abs(got - want).max())
    else:
        assert np.abs(got - want).max() <= G_TOL * np.abs(want).max(), (what, np.abs(got - want).max() / np.abs(want).max())


def G_of(m, s):
    return getattr(m.timestepper.Gn, s.name).interior_numpy().copy()


def sync_oracle_to_device(p, m, keys):
    """FAST: the restatement is fed the device's own h / aice state and tendencies"""
    fields = {"h": m.ice_thickness, "aice": m.ice_concentration, "Gh": m.timestepper.Gn.h, "Ga": m.timestepper.Gn.aice}
    m.synchronize()
    for k in keys:
        p.f[k][...] = fields[k].numpy()


# ---- the two halves, stand-alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("topo", sorted(TOPOS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_halves_against_the_restatement(shape, topo, mode, oracle_lib):
    """Three tracers of mixed weighting in one launch, six schemes, land and everything beyond a wall poisoned with 1e300 in the tracers;
    the metric kind rotates with the case"""
    Nx, Ny = SHAPES[shape]
    metric = (sorted(SHAPES).index(shape) + sorted(TOPOS).index(topo)) % 3
    c = flow_case(Nx, Ny, TOPOS[topo], metric)
    specs = specs_of(3)
    m = model_of(c, specs, mode=mode, stepper="ForwardEuler")
    p, ts = ref_of(c, specs)
    assert m.ctx.tracers_stats() == (0, 0) and m.ctx.tracers_last()["tracers_per_thread"] == 0
    bad = inactive_parent(p)
    for t, s in zip(ts, specs):
        t["c"][bad] = POISON
        m.copy_to_field(m.tracer(s.name), t["c"])
    start = {k: p.f[k].copy() for k in ("h", "aice")}
    start_c = [t["c"].copy() for t in ts]
    dt = c["dt"]
    for n, scheme in enumerate(SCHEMES):
        for k in ("h", "aice"):
            p.f[k][...] = start[k]
        m.copy_to_field(m.ice_thickness, start["h"]); m.copy_to_field(m.ice_concentration, start["aice"])
        for t, s, c0 in zip(ts, specs, start_c):
            t["c"][...] = c0
            m.copy_to_field(m.tracer(s.name), c0)
        p.compute_tracer_tendencies(scheme)
        m.ctx.call("csi_compute_tracer_tendencies", scheme)
        m.ctx.tracers_tendencies(scheme, dt, False)
        m.synchronize()
        assert m.ctx.tracers_stats() == (n + 1, n) and m.ctx.tracers_last() == expected_layout(3)
        want = [tr.tendency(p, scheme, t["c"], t["weighted"]) for t in ts]
        got = [G_of(m, s) for s in specs]
        for s, g_, w_ in zip(specs, got, want):
            assert np.abs(w_).max() > 0
            same_G(mode, g_, w_, (shape, topo, scheme, "G", s.name))
        if mode == "fast":
            sync_oracle_to_device(p, m, ("Gh", "Ga"))
        tr.stage_first(p, ts, scheme, dt, G_given=got)
        p.dynamic_step_tracers(dt, False)
        m.ctx.call("csi_dynamic_step_tracers", dt, 0)
        if mode == "fast":
            sync_oracle_to_device(p, m, ("h", "aice"))
        tr.stage_second(p, ts, dt)
        m.ctx.tracers_update(dt)
        m.synchronize()
        assert m.ctx.tracers_stats() == (n + 1, n + 1)
        for t, s in zip(ts, specs):
            got_c = m.tracer(s.name).numpy()
            assert np.array_equal(got_c, t["c"]), (shape, topo, scheme, s.name, np.argwhere(got_c != t["c"])[:4])      # whole parents: images included
            inner = tr.interior(p, got_c)
            assert np.all(inner[~tr.active(p)] == 0.0) and np.all(inner[p.interior("aice") <= 0] == 0.0)
            assert np.abs(inner).max() < 1e6          # the poison reached nothing


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_f32_weights_and_no_advection(mode, oracle_lib):
    """WENO weights in single precision (the weight dtype h sees), and scheme 0: G = 0 and no stencil launch"""
    Nx, Ny = SHAPES["one_column_last_block"]
    c = flow_case(Nx, Ny, TOPOS["pb"], 1)
    specs = specs_of(2)
    m = model_of(c, specs, mode=mode, stepper="ForwardEuler", scheme=7, weight_dtype="f32")
    p, ts = ref_of(c, specs)
    p.s.weno_weights_f32 = 1
    dt = c["dt"]
    for n, scheme in enumerate((7, 5, 3)):
        p.compute_tracer_tendencies(scheme)
        m.ctx.call("csi_compute_tracer_tendencies", scheme)
        m.ctx.tracers_tendencies(scheme, dt, False)
        m.synchronize()
        assert m.ctx.tracers_stats() == (n + 1, 0) and m.ctx.tracers_last() == expected_layout(2)
        for t, s in zip(ts, specs):
            same_G(mode, G_of(m, s), tr.tendency(p, scheme, t["c"], t["weighted"]), (scheme, s.name))
    p.s.weno_weights_f32 = 0
    q, us = ref_of(c, specs)
    tr.zero_tendencies(q)
    m.ctx.call("csi_update_state")
    before = m.ctx.tracers_stats()
    for f in (m.timestepper.Gn.h, m.timestepper.Gn.aice):
        f.data.zero_()
    torch.cuda.synchronize()
    m.ctx.tracers_tendencies(0, dt, False)
    tr.stage_first(q, us, 0, dt)
    tr.stage_second(q, us, dt)
    m.ctx.tracers_update(dt)
    m.synchronize()
    assert m.ctx.tracers_stats() == (before[0], before[1] + 2)
    for t, s in zip(us, specs):
        assert np.all(G_of(m, s) == 0.0)
        assert np.array_equal(m.tracer(s.name).numpy(), t["c"]), s.name


# ---- whole steps -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("topo", ["pp", "bb"])
def test_plain_tracer_is_the_oracles_snow_thickness_over_steps(topo, mode, oracle_lib):
    """Prescribed velocities, one FE step and three RK3 steps: STRICT the plain nonnegative tracer equals the oracle's hs (and G its
    Ghs) bit for bit; FAST within the stated tolerances"""
    Nx, Ny = SHAPES["one_column_last_block"]
    c = flow_case(Nx, Ny, TOPOS[topo], 0)
    specs = specs_of(1)
    for stepper, steps in (("ForwardEuler", 1), ("SplitRungeKutta3", 3)):
        m = model_of(c, specs, mode=mode, stepper=stepper, scheme=7)
        p = cases.oracle_problem(c)
        p.s.has_snow = 1
        p.interior("hs")[...] = c["values"][0]
        p.update_state()
        for n in range(steps):
            tr.step_fe(p, [], c["dt"], 7, n == 0) if stepper == "ForwardEuler" else tr.step_rk3(p, [], c["dt"], 7)
            csi.time_step(m, c["dt"])
        m.synchronize()
        stages = 1 if stepper == "ForwardEuler" else 9
        assert m.ctx.tracers_stats() == (stages, stages) and m.ctx.tracers_last() == expected_layout(1)
        assert m.ctx.last_advection()["stage_fused"] == 0
        got, G = m.tracer("plain").numpy(), G_of(m, specs[0])
        if mode == "strict":
            assert np.array_equal(G, p.interior("Ghs")) and np.array_equal(got, p.f["hs"]), (stepper, np.abs(got - p.f["hs"]).max())
            assert np.array_equal(m.ice_concentration.numpy(), p.f["aice"])
        else:
            same_G(mode, G, p.interior("Ghs"), stepper)
            assert np.abs(got - p.f["hs"]).max() <= 1e-13 * np.abs(p.f["hs"]).max()
            assert np.array_equal(got == 0.0, p.f["hs"] == 0.0)


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_tracer_follows_the_bound_snow_thickness_without_any_tolerance(mode):
    """A context with hs / Ghs / hs^- bound, EVP dynamics (4 sub-steps) and a plain nonnegative tracer initialised to hs: after three
    RK3 steps and three FE steps c == hs bit for bit, in both modes -- the velocities used, the base state and the zero rule"""
    for stepper in ("SplitRungeKutta3", "ForwardEuler"):
        c = cases.make_case(Nx=37, Ny=29, substeps=4, random_uv=0.05, land=0.15)
        c["values"] = [np.where(c["mask"], 0.05 + 0.1 * np.random.default_rng(3).random((29, 37)), 0.0)]
        m = model_of(c, specs_of(1), mode=mode, stepper=stepper, scheme=5, dynamics=True)
        g, dev = c["g"], m.device
        hs, Ghs, hsm = (csi.CenterField(g, dev, n) for n in ("hs", "Ghs", "hs-"))
        hs.set(c["values"][0])
        torch.cuda.synchronize()
        m._bind("HS", hs); m._bind("GHS", Ghs)
        if stepper == "SplitRungeKutta3":
            m._bind("HSM", hsm)
        m.ctx.call("csi_update_state")
        for _ in range(3):
            csi.time_step(m, c["dt"])
        m.synchronize()
        stages = 9 if stepper == "SplitRungeKutta3" else 3
        assert m.ctx.tracers_stats() == (stages, stages)
        assert np.abs(hs.interior_numpy() - c["values"][0]).max() > 1e-6
        assert np.array_equal(m.tracer("plain").numpy(), hs.numpy()), (stepper, mode)
        assert np.array_equal(G_of(m, specs_of(1)[0]), Ghs.interior_numpy())


def test_the_model_steps_the_same_with_and_without_tracers():
    c = cases.make_case(Nx=37, Ny=29, substeps=4, random_uv=0.05)
    c["values"] = [0.5 + np.random.default_rng(k).random((29, 37)) for k in range(8)]
    out = []
    for specs in ([], specs_of(5)):
        m = model_of(c, specs, mode="fast", stepper="SplitRungeKutta3", scheme=7, dynamics=True)
        for _ in range(2):
            csi.time_step(m, c["dt"])
        m.synchronize()
        assert m.ctx.tracers_stats() == ((6, 6) if specs else (0, 0))
        out.append([f.numpy().copy() for f in (m.ice_thickness, m.ice_concentration, m.velocities.u, m.velocities.v)])
    for a, b, k in zip(out[0], out[1], "h aice u v".split()):
        assert np.array_equal(a, b), k


# ---- layout independence ---------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_layout(monkeypatch):
    """Tracer k computes the same bits alone, as the 8th of 8, and in every group size: n = 1, 2, 3, 5, 8 with mixed weightings in
    one launch, 1 / 2 / 4 tracers per thread"""
    Nx, Ny = SHAPES["fewer_rows_than_a_tile"]
    c = flow_case(Nx, Ny, TOPOS["pb"], 0)

    def run(ks, force):
        if force:
            monkeypatch.setenv("CSI_TRACERS_NTR", str(force))
        else:
            monkeypatch.delenv("CSI_TRACERS_NTR", raising=False)
        specs = [specs_of(8)[k] for k in ks]
        m = model_of(c, specs, mode="fast", stepper="SplitRungeKutta3", scheme=7, values=[c["values"][k] for k in ks])
        csi.time_step(m, c["dt"])
        m.synchronize()
        assert m.ctx.tracers_stats() == (3, 3) and m.ctx.tracers_last() == expected_layout(len(ks), force)
        return {k: (m.tracer(s.name).numpy().copy(), G_of(m, s)) for k, s in zip(ks, specs)}
    alone = {k: run([k], 0)[k] for k in range(8)}
    for n, force in ((8, 0), (8, 1), (8, 2), (5, 0), (5, 2), (3, 0), (3, 1), (2, 0), (2, 4), (1, 4), (1, 2)):
        got = run(list(range(n)), force)
        for k in range(n):
            assert np.array_equal(got[k][0], alone[k][0]) and np.array_equal(got[k][1], alone[k][1]), (n, force, k)
    last = run([7], 0)[7]          # the 8th of 8, alone
    assert np.array_equal(last[0], run(list(range(8)), 0)[7][0])


# ---- thermodynamics, the fold, the example's invariant, checkpoints, output ------------------------------------------------------------------------
def test_age_vanishes_with_the_ice_and_restarts_in_refrozen_cells():
    """Slab thermodynamics with a per-cell bottom heat flux: a patch melts to extinction (age == 0 there), then refreezes (age == dt after
    the first step with ice, 2 dt after the second); elsewhere age grows by dt per step.  Velocities are zero and the concentrations
    powers of two, so every figure is exact."""
    Nx, Ny, dt = 37, 29, 120.0
    g = csi.RectilinearGrid((Nx, Ny), x=(0, Nx * 1e3), y=(0, Ny * 1e3), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
    patch = np.zeros((Ny, Nx), bool)
    patch[5:9, 30:37] = True
    qb = np.where(patch, 1e5, 0.0)
    for stepper in ("ForwardEuler", "SplitRungeKutta3"):
        m = csi.SeaIceModel(g, advection=csi.WENO(order=7), timestepper=stepper, mode="fast", tracers=(csi.IceAge(),),
                            ice_thermodynamics=csi.SlabThermodynamics(top_temperature=-1.0), bottom_heat_flux=qb)
        csi.set_(m, h=np.where(patch, 0.01, 1.0), aice=np.where(patch, 0.5, 1.0))
        for n in range(1, 3):
            csi.time_step(m, dt)
        m.synchronize()
        a, age = m.ice_concentration.interior_numpy(), m.tracer("age").interior_numpy()
        assert np.all(a[patch] == 0.0) and np.all(age[patch] == 0.0), (stepper, a[patch].max())
        assert np.all(age[~patch] == 2 * dt)
        m.external_heat_fluxes.bottom.set(np.where(patch, -1e5, 0.0))
        torch.cuda.synchronize()
        for n in (1, 2):
            csi.time_step(m, dt)
            m.synchronize()
            a, age = m.ice_concentration.interior_numpy(), m.tracer("age").interior_numpy()
            assert np.all(a[patch] > 0.0), stepper
            assert np.all(age[patch] == n * dt), (stepper, n, age[patch][:3])
            assert np.all((age[~patch] >= (2 + n) * dt * (1 - 1e-15)) & (age[~patch] <= (2 + n) * dt * (1 + 1e-15)))
        stages = 4 * (1 if stepper == "ForwardEuler" else 3)
        assert m.ctx.tracers_stats() == (stages, stages)


def test_masked_north_fold_against_the_oracles_snow_thickness(oracle_lib):
    c = flow_case(64, 44, ("periodic", "folded"), 0, land=False, curvilinear=0.04)
    c2 = cases.make_case(Nx=64, Ny=44, topo=("periodic", "folded"), patches=False, noise=0.0, land=0.2, curvilinear=0.04, top=None, bottom=None, coriolis=None)
    wet = c2["mask"].astype(bool)
    c = dict(c, g=c2["g"], mask=c2["mask"], a=np.where(wet, c["a"], 0.0), h=np.where(wet, c["h"], 0.0), values=[np.where(wet, c["values"][0], 0.0)])
    specs = specs_of(1)
    m = model_of(c, specs, mode="strict", stepper="ForwardEuler", scheme=7)
    p = cases.oracle_problem(c)
    p.s.has_snow = 1
    p.interior("hs")[...] = c["values"][0]
    p.update_state()
    for n in range(2):
        tr.step_fe(p, [], c["dt"], 7, n == 0)
        csi.time_step(m, c["dt"])
    m.synchronize()
    assert m.ctx.tracers_stats() == (2, 2)
    assert np.array_equal(G_of(m, specs[0]), p.interior("Ghs"))
    assert np.array_equal(m.tracer("plain").numpy(), p.f["hs"])          # the rows beyond the fold included


WENO7_DRIFT = 1e-7


@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
@pytest.mark.parametrize("scheme", [1, 7])
def test_age_stays_between_zero_and_the_model_time(scheme, stepper):
    """examples/anticyclone_with_ice_age.py's invariant 0 <= age <= t, after every step, under both steppers (RK3 stages reconstruct the
    source-free copy of the stage before: include/csi.h).
    Scheme 1 (first-order upwind, a convex combination): as stated, to rounding (1e-12).
    WENO7 (the example): WENO-Z's eps = 1e-8 makes the reconstruction of aice * age inhomogeneous in the scale of age, so a uniform age
    drifts.  The issue records that drift for the ORACLE, not for the code under test: 1.9e-8 per FE step for WENO7 on 37 x 29 (6.2e-8 for
    WENO3).  Bound: 1e-7 per stencil evaluation -- five times the recorded WENO7 figure, for other data -- with one evaluation per FE
    step and three per RK3 step: age <= t (1 + 1e-7 n) and t (1 + 3e-7 n) after n steps."""
    from test_gpu_steps import anticyclone_case
    c = anticyclone_case(48)
    m = csi.SeaIceModel(c["g"], advection=advection_of(scheme), timestepper=stepper, mode="fast", tracers=("dye", csi.IceAge()))
    csi.set_(m, h=c["h"], aice=c["a"], u=c["u"], v=c["v"], dye=(c["h"] > 0.35).astype(float))
    per_step = 1 if stepper == "ForwardEuler" else 3
    a0 = c["a"]
    for n in range(1, 11):
        csi.time_step(m, c["dt"])
        m.synchronize()
        age = m.tracer("age").interior_numpy()
        t = m.clock.time
        bound = t * (1 + 1e-12) if scheme == 1 else t * (1 + WENO7_DRIFT * per_step * n)
        print(stepper, scheme, n, "age in", age.min(), age.max(), "t", t, "excess", age.max() / t - 1)
        assert age.min() >= 0.0 and age.max() <= bound, (n, age.min(), age.max(), t)
        assert np.all(age[m.ice_concentration.interior_numpy() <= 0] == 0.0)
    assert age.max() > 0.9 * t
    entered = (a0 == 0) & (m.ice_concentration.interior_numpy() > 0)
    assert entered.any()                      # ice was carried into the open-water patch: the cells the bound is about
    stages = 10 * per_step
    assert m.ctx.tracers_stats() == (stages, stages) and m.ctx.tracers_last() == expected_layout(2)


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_rk3_steps_of_tracers_with_sources_against_the_restatement(mode, oracle_lib):
    """Two RK3 steps, prescribed velocities, five tracers of mixed weighting, three of them with a source: from the second stage on
    their stencils read the source-free copy.  STRICT: c bit for bit, G of the last stage bit for bit; FAST: within the tolerances."""
    Nx, Ny = SHAPES["one_column_last_block"]
    c = flow_case(Nx, Ny, TOPOS["pb"], 0)
    specs = specs_of(5)
    m = model_of(c, specs, mode=mode, stepper="SplitRungeKutta3", scheme=7)
    p, ts = ref_of(c, specs)
    for _ in range(2):
        tr.step_rk3(p, ts, c["dt"], 7)
        csi.time_step(m, c["dt"])
    m.synchronize()
    assert m.ctx.tracers_stats() == (6, 6) and m.ctx.tracers_last() == expected_layout(5)
    for t, s in zip(ts, specs):
        got = m.tracer(s.name).numpy()
        if mode == "strict":
            assert np.array_equal(G_of(m, s), t["G"]), s.name
            assert np.array_equal(got, t["c"]), (s.name, np.abs(got - t["c"]).max())
        else:
            same_G(mode, G_of(m, s), t["G"], s.name)
            assert np.abs(got - t["c"]).max() <= 1e-13 * max(np.abs(t["c"]).max(), 2 * c["dt"] * abs(s.source)), s.name
            assert np.array_equal(got == 0.0, t["c"] == 0.0)


def test_checkpoint_mid_run(tmp_path):
    c = flow_case(37, 29, TOPOS["pb"], 1)
    specs = specs_of(3)
    m = model_of(c, specs, mode="fast", stepper="SplitRungeKutta3", scheme=7)
    for _ in range(2):
        csi.time_step(m, c["dt"])
    state = csi.prognostic_state(m)
    assert {"tracers." + s.name for s in specs} <= set(state)
    for _ in range(2):
        csi.time_step(m, c["dt"])
    m.synchronize()
    want = {s.name: m.tracer(s.name).numpy().copy() for s in specs}
    m2 = model_of(c, specs, mode="fast", stepper="SplitRungeKutta3", scheme=7)
    csi.restore_prognostic_state(m2, state)
    assert m2.clock.iteration == 2
    for _ in range(2):
        csi.time_step(m2, c["dt"])
    m2.synchronize()
    for s in specs:
        assert np.array_equal(m2.tracer(s.name).numpy(), want[s.name]), s.name
    assert not any(k.startswith("tracers.") for k in csi.prognostic_state(model_of(c, [], mode="fast")))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_output_of_a_tracer(dtype, tmp_path):
    """A snapshot and a time average of a tracer, masked: the records equal the stand-in's arithmetic (tests/output_ref.py)"""
    c = flow_case(37, 29, TOPOS["pp"], 0)
    specs = specs_of(2)
    m = model_of(c, specs, mode="fast", stepper="ForwardEuler", scheme=5)
    m.output_writers["snap"] = csi.OutputWriter(m, ["age", "aice"], csi.IterationInterval(2), str(tmp_path / "s"), dtype=dtype, mask=True, fill_value=-999.0)
    m.output_writers["avg"] = csi.OutputWriter(m, ["age"], csi.AveragedTimeInterval(2 * c["dt"]), str(tmp_path / "a"), dtype=dtype, mask=True, fill_value=-999.0)
    seen = []
    for _ in range(2):
        csi.time_step(m, c["dt"])
        m.synchronize()
        seen.append(m.tracer("age").interior_numpy().copy())
    for w in m.output_writers.values():
        w.close()
    mask = c["mask"].astype(np.uint8)
    snap = np.load(tmp_path / "s" / "age.npy")
    assert np.array_equal(snap[-1], output_ref.element(seen[-1], dtype, mask, -999.0), equal_nan=True)
    acc = np.zeros_like(seen[0])
    for x in seen:
        acc = output_ref.accumulate(acc, x, c["dt"])
    avg = np.load(tmp_path / "a" / "age.npy")
    assert avg.shape[0] == 1 and np.array_equal(avg[0], output_ref.element(output_ref.average(acc, 2 * c["dt"]), dtype, mask, -999.0), equal_nan=True)
    # csi_tracers_set after csi_output_create invalidates the set, like a re-bind
    h = m.ctx.output_create([("TRACER:1", _L.OUT_F64, 0, 0, 0.0)], 1)
    m.ctx.tracers_set(None)
    with pytest.raises(csi.CsiError, match="re-bound"):
        m.ctx.output_snapshot(h)
    with pytest.raises(csi.CsiError, match="tracer 1 is not bound"):
        m.ctx.output_create([("TRACER:1", _L.OUT_F64, 0, 0, 0.0)], 1)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_and_tiles_by_name():
    c = flow_case(37, 29, TOPOS["pp"], 0, land=False)
    m = model_of(c, specs_of(2), mode="fast")
    ctx, good = m.ctx, m._tracers_struct

    def variant(**kw):
        t = _L.Tracers.from_buffer_copy(good)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(t, k)[v[0]] = v[1]
            else:
                setattr(t, k, v)
        return t
    ptr = lambda f: f.data.data_ptr()      # noqa: E731
    for t, word in ((variant(n=0), "n must be between 1 and CSI_TRACERS_MAX"), (variant(n=9), "n must be between 1"),
                    (variant(weighting=(1, 2)), "tracer 1: unknown weighting"), (variant(nonnegative=(0, 3)), "tracer 0: nonnegative"),
                    (variant(source=(1, float("inf"))), "tracer 1: source must be finite"), (variant(c=(0, None)), "tracer 0: c == NULL"),
                    (variant(c=(1, ptr(m.tracer("plain")))), "tracer 1: c aliases c of tracer 0"),
                    (variant(G=(1, ptr(m.tracer("plain")))), "tracer 1: G aliases c of tracer 0"),
                    (variant(c=(0, ptr(m.ice_concentration))), "tracer 0: c aliases field aice"),
                    (variant(c=(0, ptr(m.ice_thickness) + 8 * 40)), "tracer 0: c aliases field h")):
        with pytest.raises(csi.CsiError, match=word):
            ctx.tracers_set(t)
    # a shape that is not h's: an allocation of its own that cannot hold a parent of h
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    tiny = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(tiny), ctypes.c_size_t(512)) == 0
    try:
        with pytest.raises(csi.CsiError, match="tracer 0: c is smaller than the parent of h"):
            ctx.tracers_set(variant(c=(0, tiny.value)))
    finally:
        hip.hipFree(tiny)
    ctx.tracers_set(good)          # the refusals changed nothing: the model still steps
    csi.time_step(m, c["dt"])
    with pytest.raises(csi.CsiError, match="csi_tracers_tendencies before it"):
        ctx.tracers_update(c["dt"])
    with pytest.raises(csi.CsiError, match="dt must be finite"):
        ctx.tracers_tendencies(7, float("nan"), False)
    with pytest.raises(csi.CsiError, match="unknown advection scheme"):
        ctx.tracers_tendencies(4, c["dt"], False)
    # tiles, whichever call comes second
    with pytest.raises(csi.CsiError, match="advected tracers are not supported on tiled contexts") as e:
        ctx.call("csi_tile_set", 0, 0, 2, 1, 1, 1)
    assert e.value.code == UNSUPPORTED
    ctx.tracers_set(None)
    ctx.call("csi_tile_set", 0, 0, 2, 1, 1, 1)
    with pytest.raises(csi.CsiError, match="tracers: tiled contexts are not supported"):
        ctx.tracers_set(good)
    with pytest.raises(csi.CsiError, match="csi_tracers_set has not been called"):
        ctx.tracers_tendencies(7, c["dt"], False)
    with pytest.raises(NotImplementedError, match="tiled"):
        g8 = csi.RectilinearGrid((8, 8), x=(0, 8.0), y=(0, 8.0), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
        csi.SeaIceModel(csi.TileGrid(g8, 2, 1, 0, 0), tracers=("dye",))


def test_a_model_without_tracers_makes_none_of_the_calls(monkeypatch):
    c = flow_case(37, 29, TOPOS["pp"], 0, land=False)
    m = model_of(c, [], mode="fast", stepper="SplitRungeKutta3", scheme=7)
    called = []
    for name in ("tracers_set", "tracers_tendencies", "tracers_update"):
        monkeypatch.setattr(type(m.ctx), name, lambda self, *a, _n=name: called.append(_n))
    for _ in range(2):
        csi.time_step(m, c["dt"])
    m.synchronize()
    monkeypatch.undo()
    assert called == [] and m.tracers == {} and m.ctx.tracers_stats() == (0, 0)
    assert m.ctx.last_advection()["stage_fused"] == 1          # the advection-only stage launch is still taken
