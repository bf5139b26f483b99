"""The advected tracers' rule without a GPU (include/csi.h, "advected ice tracers and ice age"; tests/tracers_ref.py restates it):
the plain tracer against the oracle's snow thickness bit for bit, a uniform field under divergent flow in the concentration-weighted
mode, mistakes that must show, exact ice age, the struct as gcc, ctypes and the Julia stub lay it out, and the Python front end."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import oracle as O
import output_ref
import tracers_ref as tr
from climaseaice_jl_amd import _lib as L
from climaseaice_jl_amd import model as M
from climaseaice_jl_amd import output as Out
from climaseaice_jl_amd import tracers as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def flow_case(topo, land, seed=11, amin=0.2, amax=0.9, cfl=0.2):
    """37 x 29, divergent seeded velocities with |U| dt / dx <= cfl, aice in [amin, amax]; the oracle's own steps move the velocities with
    its momentum step (ten EVP sub-steps, no stresses, no Coriolis), steps composed with dynamics = False keep them as prescribed"""
    rng = np.random.default_rng(seed)
    c = cases.make_case(Nx=37, Ny=29, H=4, topo=topo, spacing=1000.0, patches=False, noise=0.0, land=land, top=None, bottom=None, coriolis=None)
    vmax = cfl * 1000.0 / c["dt"]
    c["u"] = vmax * (2 * rng.random(c["u"].shape) - 1)
    c["v"] = vmax * (2 * rng.random(c["v"].shape) - 1)
    if topo[0] == "bounded":
        c["u"][:, 0] = 0.0; c["u"][:, -1] = 0.0
    if topo[1] == "bounded":
        c["v"][0, :] = 0.0; c["v"][-1, :] = 0.0
    wet = np.ones((29, 37), bool) if c["mask"] is None else c["mask"].astype(bool)
    c["a"] = np.where(wet, amin + (amax - amin) * rng.random((29, 37)), 0.0)
    c["h"] = np.where(wet, 0.3 + 0.2 * rng.random((29, 37)), 0.0)
    c["tracer0"] = np.where(wet, 0.1 + rng.random((29, 37)), 0.0)
    return c


def oracle_with_snow(c):
    p = cases.oracle_problem(c)
    p.s.has_snow = 1
    p.interior("hs")[...] = c["tracer0"]
    p.update_state()
    return p


# ---- 1. the plain tracer IS the oracle's snow thickness ----------------------------------------------------------------------------------
@pytest.mark.parametrize("land", [0.0, 0.2])
@pytest.mark.parametrize("topo", [("periodic", "periodic"), ("bounded", "bounded")])
def test_plain_tracer_equals_the_oracles_snow_thickness_bitwise(topo, land, oracle_lib):
    c = flow_case(topo, land)
    for scheme in (7, -5, 1):
        # one FE step: the oracle's own time_step_fe carries hs; the restatement carries c beside a problem stepped by the same verbs
        p, q = oracle_with_snow(c), oracle_with_snow(c)
        t = tr.tracer(q, c["tracer0"])
        p.time_step_fe(c["dt"], scheme, True)
        tr.step_fe(q, [t], c["dt"], scheme, first_iteration=True, dynamics=True)
        for k in ("h", "aice", "hs", "u", "v"):
            assert np.array_equal(p.f[k], q.f[k]), (scheme, k)           # the composition of verbs is the oracle's step
        assert np.array_equal(t["c"], p.f["hs"]), (scheme, "FE")           # whole parents: halos included
        assert np.abs(p.interior("hs") - c["tracer0"]).max() > 0
        # three RK3 steps: hs from Psi^- (the oracle's verbs with hsm cached), h and aice also against the oracle's own time_step_rk3
        p, q, r = oracle_with_snow(c), oracle_with_snow(c), cases.oracle_problem(c)
        t = tr.tracer(q, c["tracer0"])
        for _ in range(3):
            tr.step_rk3(p, [], c["dt"], scheme, dynamics=True)
            tr.step_rk3(q, [t], c["dt"], scheme, dynamics=True)
            r.time_step_rk3(c["dt"], scheme)
        for k in ("h", "aice", "u", "v"):
            assert np.array_equal(p.f[k], r.f[k]), (scheme, k)
        assert np.array_equal(t["c"], p.f["hs"]), (scheme, "RK3")
        if land:
            assert np.all(tr.interior(q, t["c"])[~tr.active(q)] == 0.0)


# ---- 2. a uniform field under divergent flow --------------------------------------------------------------------------------------------
def uniform_deviation(c, scheme, weighted, value=7.0):
    p = cases.oracle_problem(c)
    t = tr.tracer(p, np.full((29, 37), value), weighted=weighted)
    tr.step_fe(p, [t], c["dt"], scheme, first_iteration=True)
    ice = p.interior("aice") > 0
    return np.abs(tr.interior(p, t["c"])[ice] / value - 1.0).max(), p, t


def test_uniform_stays_uniform_by_concentration(oracle_lib):
    """c = 7 everywhere, aice in [0.2, 0.9], |U| dt / dx <= 0.2, one FE step.  LINEAR schemes (1, -3, -5): q = aice * 7 is aice scaled and
    the reconstruction is linear, so in exact arithmetic G_q = 7 G_a and c* = (aice 7 + dt 7 G_a) / (aice + dt G_a) = 7.  First-order
    bound on the rounding, in units of u = 2^-53 and relative to q: the product aice * 7 (1), its counterpart inside every stencil value of
    G_q, carried through n_ops <= 12 rounded operations (a 5-point polynomial, two products per flux, the 4-term divergence, / V) and
    the 4 flux terms' own roundings, all scaled by |dt G| / q <= 4 cfl; the product dt * G and the sum (2); the quotient (1): the
    numerator and denominator together (4 + 4 cfl (n_ops + 4)) u.  The quotient divides by aice* >= aice (1 - 4 cfl), and an absolute
    error relative to q = amax * 7 meets a denominator as small as amin * 7: the factor amax / (amin (1 - 4 cfl)).
    Measured: 4 u, 5 u, 5 u; measured / bound 0.011 - 0.013.
    WENO schemes: WENO-Z's eps = 1e-8 makes the weights inhomogeneous in the scale of q, so only the ratio to the plain mode's deviation
    on the same data is asserted (< 1e-3).  Measured: WENO3 3.9e-7, WENO5 3.4e-8, WENO7 5.4e-8 against 0.68 for the plain mode."""
    c = flow_case(("periodic", "periodic"), 0.0)
    plain = {s: uniform_deviation(c, s, False)[0] for s in (1, -3, -5, 3, 5, 7)}
    cfl, n_ops = 0.2, 12.0           # <= 12 rounded operations between a stencil value and G (5-point polynomial, 2 products, 4-term sum, / V)
    amin, amax = 0.2, 0.9
    bound = (4 + 4 * cfl * (n_ops + 4.0)) * U * amax / (amin * (1 - 4 * cfl))
    for s in (1, -3, -5):
        dev = uniform_deviation(c, s, True)[0]
        print(f"scheme {s}: weighted deviation {dev:.3e} = {dev / U:.1f} u, bound {bound:.3e}, measured / bound {dev / bound:.3f}; plain {plain[s]:.3e}")
        assert dev <= bound, (s, dev, bound)
        assert plain[s] > 1e-3
    for s in (3, 5, 7):
        dev = uniform_deviation(c, s, True)[0]
        print(f"scheme {s} (WENO): weighted deviation {dev:.3e}, plain {plain[s]:.3e}, ratio {dev / plain[s]:.3e}")
        assert dev < 1e-3 * plain[s], (s, dev, plain[s])


# ---- 3. mistakes that must show ------------------------------------------------------------------------------------------------------------
def test_mistakes_show(oracle_lib):
    c = flow_case(("periodic", "periodic"), 0.0, amin=0.0)
    c["a"][5:9, 6:12] = 0.0; c["h"][5:9, 6:12] = 0.0          # open water: the zero rule and the source in ice-free cells
    c["a"][20:24, 20:30] = 0.97                               # ... and cells that ridge (aice* > 1 where the flow converges)
    dt, scheme = c["dt"], 5
    # the plain mode on a uniform field (test 2): 5e-2 there
    assert uniform_deviation(flow_case(("periodic", "periodic"), 0.0), 5, False)[0] > 1e-2

    def run(first=tr.first_half, second=tr.second_half, steps=1, stepper="fe", source=1.0):
        p = cases.oracle_problem(c)
        t = tr.tracer(p, c["tracer0"], weighted=True, source=source)
        keep = tr.first_half, tr.second_half
        tr.first_half, tr.second_half = first, second
        try:
            for n in range(steps):
                tr.step_fe(p, [t], dt, scheme, n == 0) if stepper == "fe" else tr.step_rk3(p, [t], dt, scheme)
        finally:
            tr.first_half, tr.second_half = keep
        return tr.interior(p, t["c"]).copy(), p

    right, p = run()
    ice_free = p.interior("aice") <= 0
    assert ice_free.any() and np.all(right[ice_free] == 0.0)

    def a_after(G, cb, ab, Ga, dtau, weighted):          # aice AFTER instead of before the update in q^-
        a_star = ab + dtau * Ga
        return np.where(a_star > 0, ((a_star * cb) + dtau * G) / a_star, 0.0)

    def a_clipped(G, cb, ab, Ga, dtau, weighted):        # aice* with the clip applied
        a_star = ab + dtau * Ga
        return np.where(a_star > 0, ((ab * cb) + dtau * G) / np.minimum(a_star, 1.0), 0.0)

    def source_everywhere(star, a, act, dtau, nonneg, source):      # the source added in ice-free cells
        return np.where(act, np.where(a > 0, np.maximum(0.0, star), 0.0) + dtau * source, 0.0)

    for name, kw in (("aice after", dict(first=a_after)), ("aice* clipped", dict(first=a_clipped)), ("source in ice-free cells", dict(second=source_everywhere))):
        wrong = run(**kw)[0]
        d = np.abs(wrong - right).max()
        print(f"{name}: max |difference| {d:.3e}")
        assert d > 1e-6, name
    # stage steps accumulated: every stage continuing from the stage before it instead of restarting from Psi^- -- a source then accrues
    # dt / 3 + dt / 2 + dt = 11/6 dt per RK3 step
    c2 = dict(c, u=np.zeros_like(c["u"]), v=np.zeros_like(c["v"]), a=np.full_like(c["a"], 0.5), h=np.full_like(c["h"], 0.3))

    def rk3(accumulate):
        p = cases.oracle_problem(c2)
        t = tr.tracer(p, np.zeros((29, 37)), weighted=True, source=1.0)
        if not accumulate:
            tr.step_rk3(p, [t], dt, scheme)
        else:
            for m, k in (("hm", "h"), ("am", "aice")):
                p.f[m][...] = p.f[k]
            for beta in (3, 2, 1):
                p.compute_tracer_tendencies(scheme)
                tr.stage_first(p, [t], scheme, dt / beta)          # base: the current fields, not Psi^-
                p.dynamic_step_tracers(dt / beta, True)
                tr.stage_second(p, [t], dt / beta)
                p.update_state()
        return tr.interior(p, t["c"]).copy()
    assert np.all(rk3(False) == dt)
    wrong = rk3(True)
    print(f"stage steps accumulated: age after one step {wrong.max():.6g} s against dt = {dt:g} s")
    assert np.all(np.abs(wrong - 11.0 / 6.0 * dt) < 1e-9) and np.abs(wrong - dt).min() > 0.8 * dt
    # the stage's own result, source included, as the next stage's stencil input: cells that ice enters collect 11/6 dt
    def rk3_moving(source_free):
        p = cases.oracle_problem(c)
        t = tr.tracer(p, np.zeros((29, 37)), weighted=True, source=1.0)
        keep = tr.free_half
        if not source_free:
            tr.free_half = lambda star, a, act, nonneg: tr.second_half(star, a, act, 0.0, nonneg, 0.0) + np.where((a > 0) & act, p.stage_dt, 0.0)
        try:
            for m_, k_ in (("hm", "h"), ("am", "aice")):
                p.f[m_][...] = p.f[k_]
            base = [t["c"].copy()]
            t["free"] = None
            for beta in (3, 2, 1):
                p.stage_dt = dt / beta
                p.compute_tracer_tendencies(1)
                tr.stage_first(p, [t], 1, dt / beta, base=base, a_base=p.f["am"])
                p.dynamic_step_tracers(dt / beta, True)
                tr.stage_second(p, [t], dt / beta, rk=True)
                p.update_state()
        finally:
            tr.free_half = keep
        return tr.interior(p, t["c"]).copy()
    good, bad = rk3_moving(True), rk3_moving(False)
    print(f"stencil input with the stage's source: max age {bad.max():.6g} s, source-free {good.max():.6g} s, dt = {dt:g} s")
    assert good.max() <= dt * (1 + 1e-12) and bad.max() > 1.5 * dt


# ---- 4. exact ice age ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepper", ["fe", "rk3"])
def test_age_is_exactly_n_dt_at_rest(stepper, oracle_lib):
    """Zero velocity, ice everywhere: age == n dt exactly.  The concentrations are powers of two, so that (aice * age) / aice is exact;
    n dt is exact in doubles for dt = 120 and small n."""
    c = flow_case(("periodic", "periodic"), 0.0)
    c["u"][...] = 0.0; c["v"][...] = 0.0
    c["a"] = np.where(np.arange(37)[None, :] % 2 == 0, 1.0, 0.5) * np.ones((29, 37))
    p = cases.oracle_problem(c)
    t = tr.tracer(p, np.zeros((29, 37)), weighted=True, source=1.0)
    for n in range(1, 6):
        tr.step_fe(p, [t], c["dt"], 7, n == 1) if stepper == "fe" else tr.step_rk3(p, [t], c["dt"], 7)
        assert np.all(tr.interior(p, t["c"]) == n * c["dt"]), n


@pytest.mark.parametrize("stepper", ["fe", "rk3"])
def test_age_never_exceeds_the_model_time(stepper, oracle_lib):
    """0 <= age <= t under both steppers, with ice carried into open water: first-order upwind (a convex combination of the stencil
    values), so the bound holds to rounding.  Under RK3 this is what the source-free stencil input buys: with the stage's own result as
    the input the cells that ice enters end the first step at 11/6 dt (test_mistakes_show)."""
    c = flow_case(("periodic", "periodic"), 0.0)
    c["a"][5:9, 6:12] = 0.0; c["h"][5:9, 6:12] = 0.0
    p = cases.oracle_problem(c)
    t = tr.tracer(p, np.zeros((29, 37)), weighted=True, source=1.0)
    for n in range(1, 6):
        tr.step_fe(p, [t], c["dt"], 1, n == 1) if stepper == "fe" else tr.step_rk3(p, [t], c["dt"], 1)
        age = tr.interior(p, t["c"])
        assert age.min() >= 0.0 and age.max() <= n * c["dt"] * (1 + 1e-12), (n, age.max())
    entered = (c["a"] == 0) & (p.interior("aice") > 0)
    assert entered.any() and np.all(age[entered] > 0)


# ---- 5. layouts ----------------------------------------------------------------------------------------------------------------------------
def test_c_layout_matches_ctypes_and_the_julia_stub(tmp_path):
    exe = str(tmp_path / "tracers_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tracers_layout.c"), "-o", exe])
    got = json.loads(subprocess.check_output([exe]))
    assert got["CSI_TRACERS_MAX"] == L.TRACERS_MAX == 8
    assert (got["CSI_TRACER_PLAIN"], got["CSI_TRACER_BY_CONCENTRATION"]) == (L.TRACER_PLAIN, L.TRACER_BY_CONCENTRATION) == (0, 1)
    assert [got[f"CSI_TRACER_FIELD_{k}"] for k in (0, 7)] == [L.tracer_field(0), L.tracer_field(7)] == [4096, 4103]
    assert L.slot_id("TRACER:3") == 4099
    assert got["CSI_TRACER_FIELD_0"] > got["CSI_F_COUNT_SHORTWAVE"]          # no slot number is a tracer field id
    assert got["sizeof_tracers"] == C.sizeof(L.Tracers) == 264
    for f in ("n", "c", "G", "weighting", "nonnegative", "source"):
        assert got[f"csi_tracers.{f}"] == getattr(L.Tracers, f).offset, f
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    assert re.search(r"@assert sizeof\(CsiTracers\) == 264", stub)
    assert re.search(r"const TRACERS_MAX = 8", stub) and re.search(r"tracer_field\(k\) = Int32\(4096 \+ k\)", stub)
    m = re.search(r"struct CsiTracers\n(.*?)\nend", stub, re.S)
    assert [ln.split("::")[0].strip() for ln in m.group(1).splitlines()] == ["n", "pad", "c", "G", "weighting", "nonnegative", "source"]
    for name in ("csi_tracers_set", "csi_tracers_tendencies", "csi_tracers_update", "csi_tracers_stats", "csi_tracers_last"):
        assert f"(:{name}, libcsi)" in stub, name
    assert "function attach_tracers!(" in stub


def test_library_exports_the_entries():
    lib = L.load()
    for name, nargs in (("csi_tracers_set", 2), ("csi_tracers_tendencies", 4), ("csi_tracers_update", 2), ("csi_tracers_stats", 3), ("csi_tracers_last", 5)):
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert lib.csi_tracers_set(None, None) == -1          # CSI_ERR_INVALID_ARGUMENT: no context


# ---- 6. the front end ------------------------------------------------------------------------------------------------------------------------
def test_specs_and_argument_errors_by_name():
    s = T.tracer_specs(("dye", csi.IceAge(), csi.Tracer("salt", weighting="concentration", nonnegative=False, source=-1e-3)))
    assert [t.name for t in s] == ["dye", "age", "salt"]
    assert (s[0].weighting, s[0].nonnegative, s[0].source) == (None, True, 0.0)
    assert (s[1].weighting, s[1].nonnegative, s[1].source) == ("concentration", True, 1.0)
    assert csi.IceAge(units="days").source == 1.0 / 86400.0 and csi.IceAge("floe_age").name == "floe_age"
    assert T.tracer_specs(None) == [] and T.tracer_specs(()) == [] and [t.name for t in T.tracer_specs("dye")] == ["dye"]
    for name in ("ice_thickness", "ice_concentration", "aice", "shear", "top_x", "sigma11", "top_u", "snowfall", "forcing_u"):
        with pytest.raises(ValueError, match="taken"):          # a tracer of that name would shadow a key of set_ or of bound_fields
            csi.Tracer(name)
    for bad, exc, word in ((lambda: csi.Tracer("h"), ValueError, "taken"), (lambda: csi.Tracer("two words"), ValueError, "identifier"),
                           (lambda: csi.Tracer("x", weighting="volume"), ValueError, "weighting"),
                           (lambda: csi.Tracer("x", nonnegative=2), ValueError, "nonnegative"),
                           (lambda: csi.Tracer("x", source=float("nan")), ValueError, "finite"),
                           (lambda: csi.Tracer("x", source=np.zeros(3)), NotImplementedError, "array-valued"),
                           (lambda: csi.IceAge(units="years"), ValueError, "units"),
                           (lambda: T.tracer_specs(("a", "a")), ValueError, "twice"),
                           (lambda: T.tracer_specs([3.0]), TypeError, "csi.Tracer"),
                           (lambda: T.tracer_specs([f"t{k}" for k in range(9)]), ValueError, "at most 8")):
        with pytest.raises(exc, match=word):
            bad()
    g = csi.RectilinearGrid((8, 8), x=(0, 8.0), y=(0, 8.0), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
    with pytest.raises(NotImplementedError, match="tiled"):
        T.tracer_specs(("dye",), csi.TileGrid(g, 2, 1, 0, 0))
    with pytest.raises(TypeError):
        csi.EnthalpyMethodSeaIceModel(csi.ColumnGrid(4, (-1.0, 0.0)), tracers=("dye",))


class _Fld:
    def __init__(self, ptr):
        self.data = type("D", (), {"data_ptr": staticmethod(lambda: ptr)})()


def test_struct_of_a_model():
    specs = T.tracer_specs(("dye", csi.IceAge()))
    t = T.tracers_struct(specs, [_Fld(4096), _Fld(8192)], [_Fld(12288), None])
    assert t.n == 2 and list(t.c)[:3] == [4096, 8192, None] and list(t.G)[:2] == [12288, None]
    assert list(t.weighting)[:2] == [0, 1] and list(t.nonnegative)[:2] == [1, 1] and list(t.source)[:2] == [0.0, 1.0]


def stand_in_model(g, tracer_names):
    """A model-like object on the CPU with what output.bound_fields and model._state_fields read, its tracers as CPU Fields"""
    from collections import OrderedDict
    from types import SimpleNamespace
    CC = (csi.Center, csi.Center)
    rng = np.random.default_rng(4)

    def fld(loc, name):
        f = csi.Field(loc, g, None, name)
        f.data.copy_(torch.from_numpy(rng.standard_normal(tuple(f.data.shape))))
        return f
    m = SimpleNamespace(grid=g, clock=SimpleNamespace(time=0.0, iteration=0), output_writers=OrderedDict(), mask_interior=None,
                        velocities=SimpleNamespace(u=fld((csi.Face, csi.Center), "u"), v=fld((csi.Center, csi.Face), "v")),
                        ice_thickness=fld(CC, "h"), ice_concentration=fld(CC, "aice"), snow_thickness=None,
                        timestepper=SimpleNamespace(Gn=SimpleNamespace(), Psi_minus=None), dynamics=None, mass_fluxes=None, ocean=None,
                        _stress_fields={}, _free_drift_fields={}, external_heat_fluxes=SimpleNamespace(top=None, bottom=None), snowfall=0.0,
                        tracers=OrderedDict((n, fld(CC, n)) for n in tracer_names), synchronize=lambda: None, drifters=None)
    # the stand-in recorder looks a spec's slot up in model.fields
    m.fields = {slot: f for f, slot in Out.bound_fields(m).values()}
    return m


class _Recorder(output_ref.RefRecorder):
    bound_fields = staticmethod(Out.bound_fields)


def test_writer_hook_and_checkpoint_keys_on_the_stand_in(tmp_path):
    """bound_fields lists the tracers under CSI_TRACER_FIELD(k); a writer over a tracer name records it on the stand-in recorder of
    tests/output_ref.py; prognostic_state carries tracers.<name> only when tracers are set"""
    g = csi.RectilinearGrid((8, 6), x=(0, 8.0), y=(0, 6.0), topology=(csi.Periodic, csi.Bounded), halo=(2, 2))
    m = stand_in_model(g, ("dye", "age"))
    b = Out.bound_fields(m)
    assert b["dye"] == (m.tracers["dye"], "TRACER:0") and b["age"] == (m.tracers["age"], "TRACER:1")
    assert [L.slot_id(b[n][1]) for n in ("dye", "age")] == [L.tracer_field(0), L.tracer_field(1)]
    assert L.slot_location("TRACER:1") == (csi.Center, csi.Center)
    w = csi.OutputWriter(m, ["h", "age"], csi.IterationInterval(1), str(tmp_path / "o"), dtype="f64", recorder=_Recorder)
    w.write(m)
    w.close()
    assert np.array_equal(np.load(tmp_path / "o" / "age.npy")[0], m.tracers["age"].interior_numpy())
    with pytest.raises(Exception, match="salt"):
        csi.OutputWriter(m, ["salt"], csi.IterationInterval(1), str(tmp_path / "p"), recorder=_Recorder)
    state = M.prognostic_state(m)
    assert {"tracers.dye", "tracers.age"} <= set(state) and np.array_equal(state["tracers.age"], m.tracers["age"].numpy())
    assert not any(k.startswith("tracers.") for k in M.prognostic_state(stand_in_model(g, ())))
