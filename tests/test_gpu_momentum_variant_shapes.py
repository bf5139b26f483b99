"""The viscous and explicit momentum kernels beyond one block: k_visc_ustep, k_visc_vstep, k_tendencies, k_expl_ustep, k_expl_vstep
(csrc/momentum_viscous.hip, csrc/momentum_explicit.hip) on the cases of tests/momentum_variant_shapes.py.

tests/test_gpu_momentum_variants.py checks these kernels' values on grids of at most 24 x 20 cells, all with halo (4, 4), with 3 to 10
sub-steps, and FAST against STRICT only.  A 64 x 4 launch over such a grid is one block in x.  Here:

  * STRICT, whole parents bit for bit (the sign of a zero included) against tests/momentum_ref.py on grids of 63 x 3, 64 x 4, 65 x 5 and
    130 x 9 cells with halos (2, 2), (4, 4), (5, 3), (3, 5), every topology and metric kind, for three configurations -- the viscous
    sub-cycle, the explicit solver with ViscousRheology and with the stored stresses of EVP --, the launch counts asserted first;
  * FAST on the same cases within the stated 1e-12 of max|u| of STRICT, a zero of STRICT a zero of FAST with the same sign;
  * sub-cycles of one and two sub-steps (the results end in the scratch arrays / in the bound arrays), and two consecutive sub-cycles
    on one model: the second must not see what the first left in the scratch arrays;
  * whole time steps on 130 x 9 with halo (6, 4) and WENO7;
  * STRICT and FAST against exact arithmetic: the error of each against the 80-digit evaluation of the same expressions, STRICT's equal
    to the restatement's own, FAST's within K_FAST times it.
"""
import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import momentum_variant_shapes as mv
from fast_math_ref import CTX, U
from momentum_ref import Ref, rel_error
from test_gpu_momentum_variants import model_of

pytestmark = pytest.mark.gpu

TABLE_IDS = [c["name"] for c in mv.TABLE]
EXPLICIT_DT = 60.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_parent(label, got, want):
    """a whole parent array, finite and bit for bit"""
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert np.all(np.isfinite(got)), label
    w = np.argwhere(bits(got) != bits(want))
    assert len(w) == 0, (label, f"{len(w)} elements differ, first at (row, column) {tuple(w[0])}: {got[tuple(w[0])]!r} != {want[tuple(w[0])]!r}",
                         float(np.abs(got - want).max()))


def build(kw, configuration, mode, substeps=mv.SPLIT_SUBSTEPS, reference=True, **model_kw):
    """(model, oracle problem, Ref) of one configuration on one case; evp_explicit: stored sigma, u^n, v^n seeded on both sides as
    test_gpu_momentum_variants._set_sigma does; the explicit configurations: u^- = Psi^- set to a state that is not u."""
    viscous, explicit = configuration.startswith("viscous"), configuration.endswith("explicit")
    c = cases.make_case(substeps=substeps, **kw)
    p = cases.oracle_problem(c)
    model_kw.setdefault("timestepper", "SplitRungeKutta3" if explicit else "ForwardEuler")
    m = model_of(c, rheology=csi.ViscousRheology(nu=mv.NU) if viscous else None,
                 solver=csi.ExplicitSolver() if explicit else csi.SplitExplicitSolver(substeps=substeps), mode=mode, **model_kw)
    if not viscous:
        f = m.dynamics.auxiliaries.fields
        for k, a in mv.seed_sigma(p).items():
            m.copy_to_field(getattr(f, k), a)
    if explicit and model_kw["timestepper"] == "SplitRungeKutta3":
        rng = np.random.default_rng(9)
        for k, fld in (("um", m.timestepper.Psi_minus.u), ("vm", m.timestepper.Psi_minus.v)):
            a = p.f[k[0]] + 0.01 * rng.standard_normal(p.f[k[0]].shape)
            p.f[k][...] = a
            m.copy_to_field(fld, a)
    return c, m, p, (Ref(p, nu=mv.NU, viscous=viscous) if reference else None)


def run(m, c, configuration):
    """The configuration's launches on a model, the launch counts asserted before any value is looked at.  Returns the parents
    {name: array}.  Explicit: one tendency launch, a step from the velocities (rk_reset = False), a step from u^- (rk_reset = True)."""
    out = {}
    if configuration == "viscous_split":
        n = m.substeps
        csi.time_step_momentum(m, c["dt"])
        assert m.ctx.last_launches() == (2 * n, n) and m.ctx.launches_per_substep() == 2
        m.synchronize()
        out["u"], out["v"] = m.velocities.u.numpy().copy(), m.velocities.v.numpy().copy()
        return out
    csi.compute_momentum_tendencies(m, EXPLICIT_DT)
    for rk in (False, True):
        csi.time_step_momentum(m, EXPLICIT_DT, rk_reset=rk)
        assert m.ctx.last_launches() == (2, 1) and m.ctx.launches_per_substep() == 2
        m.synchronize()
        out[f"u_rk{int(rk)}"], out[f"v_rk{int(rk)}"] = m.velocities.u.numpy().copy(), m.velocities.v.numpy().copy()
    out["Gu"], out["Gv"] = m.timestepper.Gn.u.numpy().copy(), m.timestepper.Gn.v.numpy().copy()
    return out


def run_ref(ref, p, c, configuration):
    out = {}
    if configuration == "viscous_split":
        ref.time_step_momentum(c["dt"], c["substeps"])
        out["u"], out["v"] = p.f["u"].copy(), p.f["v"].copy()
        return out
    ref.compute_tendencies(EXPLICIT_DT)
    out["Gu"], out["Gv"] = ref.Gu.copy(), ref.Gv.copy()
    for rk in (False, True):
        ref.explicit_step(EXPLICIT_DT, rk_reset=rk)
        out[f"u_rk{int(rk)}"], out[f"v_rk{int(rk)}"] = p.f["u"].copy(), p.f["v"].copy()
    return out


# ---- STRICT: the restatement bit for bit on whole parents ------------------------------------------------------------------------------
@pytest.mark.parametrize("configuration", mv.CONFIGURATIONS)
@pytest.mark.parametrize("case", mv.TABLE, ids=TABLE_IDS)
def test_strict_bitwise(case, configuration, oracle_lib):
    c, m, p, ref = build(case["kw"], configuration, "strict")
    before = {"u": m.velocities.u.numpy().copy(), "v": m.velocities.v.numpy().copy()}
    got = run(m, c, configuration)
    want = run_ref(ref, p, c, configuration)
    assert sorted(got) == sorted(want)
    for k in sorted(got):                                   # (G first: a wrong tendency explains a wrong step)
        assert_parent((case["name"], configuration, k), got[k], want[k])
    last = "" if configuration == "viscous_split" else "_rk1"
    assert not np.array_equal(got["u" + last], before["u"]) and not np.array_equal(got["v" + last], before["v"])
    if configuration != "viscous_split":
        assert np.abs(got["Gu"]).max() > 0 and np.abs(got["Gv"]).max() > 0
        assert not np.array_equal(got["u_rk0"], got["u_rk1"])                      # u^- was another state


# ---- FAST on the same cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("configuration", mv.CONFIGURATIONS)
@pytest.mark.parametrize("case", mv.TABLE, ids=TABLE_IDS)
def test_fast_matches_strict(case, configuration, oracle_lib):
    out = {}
    for mode in ("strict", "fast"):
        c, m, _, _ = build(case["kw"], configuration, mode, reference=False)
        out[mode] = run(m, c, configuration)
    strict, fast = out["strict"], out["fast"]
    pairs = [("u", "v")] if configuration == "viscous_split" else [("Gu", "Gv"), ("u_rk0", "v_rk0"), ("u_rk1", "v_rk1")]
    for pair in pairs:
        vmax = max(np.abs(strict[k]).max() for k in pair)
        assert vmax > 0
        for k in pair:
            d = np.abs(fast[k] - strict[k]).max()
            assert np.isfinite(d) and d <= 1e-12 * vmax, (case["name"], configuration, k, d, vmax)     # FAST within 1e-12 of max|u|
            # a zero of STRICT (a peripheral point's strong zero, open water, a wall, a cell no store reaches) is the same zero in FAST
            zero = strict[k] == 0.0
            assert np.array_equal(bits(fast[k])[zero], bits(strict[k])[zero]), (case["name"], configuration, k, "zeros differ")


# ---- sub-cycles of one and two sub-steps -----------------------------------------------------------------------------------------------
SHORT = {
    "walls_65x5": mv.case_kw((65, 5), (2, 2), ("bounded", "bounded"), "uniform", "noslip_beta"),
    "channel_130x9": mv.case_kw((130, 9), (3, 5), ("periodic", "bounded"), "latlon", "wind_arrays"),
}


@pytest.mark.parametrize("substeps", [1, 2])
@pytest.mark.parametrize("name", list(SHORT))
def test_short_subcycles_strict_bitwise(name, substeps, oracle_lib):
    """One sub-step: v, then u, both results end in the scratch arrays and are copied back.  Two: both end in the bound arrays."""
    c, m, p, ref = build(SHORT[name], "viscous_split", "strict", substeps=substeps)
    got = run(m, c, "viscous_split")
    assert m.ctx.last_launches() == (2 * substeps, substeps)
    want = run_ref(ref, p, c, "viscous_split")
    for k in ("u", "v"):
        assert_parent((name, substeps, k), got[k], want[k])


def test_consecutive_subcycles_do_not_share_scratch_state(oracle_lib):
    """Two sub-cycles on one model, of one and then two sub-steps, on a grid with walls (where the halos beyond the walls reach the
    scratch arrays by the copy before the loop only): the second sub-cycle equals the restatement, which has no scratch arrays."""
    c, m, p, ref = build(SHORT["walls_65x5"], "viscous_split", "strict", substeps=1)
    for n in (1, 2):
        m.dynamics.solver.substeps = n
        assert m.substeps == n
        csi.time_step_momentum(m, c["dt"])
        assert m.ctx.last_launches() == (2 * n, n)
        ref.time_step_momentum(c["dt"], n)
        m.synchronize()
        for k, f in (("u", m.velocities.u), ("v", m.velocities.v)):
            assert_parent(("consecutive", n, k), f.numpy(), p.f[k])


# ---- whole steps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepper", ["ForwardEuler", "SplitRungeKutta3"])
@pytest.mark.parametrize("configuration", mv.CONFIGURATIONS)
def test_whole_steps_strict_bitwise(stepper, configuration, oracle_lib):
    """Two time steps with WENO7 on 130 x 9, halo (6, 4), periodic x bounded, as test_gpu_momentum_variants.test_whole_steps_strict_bitwise
    on its 20 x 16 grid, three sub-steps per sub-cycle as there."""
    substeps = mv.SPLIT_SUBSTEPS
    kw = dict(Nx=130, Ny=9, H=(6, 4), topo=("periodic", "bounded"), random_uv=0.03, u0=0.05)
    c, m, p, ref = build(kw, configuration, "strict", substeps=substeps, timestepper=stepper, advection=csi.WENO(order=7))
    explicit = configuration.endswith("explicit")
    dt = 60.0
    for n in range(2):
        csi.time_step(m, dt)
        if stepper == "ForwardEuler":
            ref.time_step_fe(dt, substeps, 7, explicit, first_iteration=(n == 0))
        else:
            ref.time_step_rk3(dt, substeps, 7, explicit)
    m.synchronize()
    fields = {"u": m.velocities.u, "v": m.velocities.v, "h": m.ice_thickness, "aice": m.ice_concentration}
    for k, f in fields.items():
        assert_parent((configuration, stepper, k), f.numpy(), p.f[k])


# ---- STRICT and FAST against exact arithmetic ------------------------------------------------------------------------------------------
# K_FAST.  FAST replaces each division of the reference order by a reciprocal and a multiply ((1 / m) a, 1 / dy, 1 / Az: at most one more
# rounding per division) and fuses the rest (fewer roundings), so in the terms that divide it may lose about a factor two against the
# reference order's own error; K_FAST = 4 is twice that allowance.  It is not taken from what FAST gives.  e_ref below is the error of
# the reference's operation order in double, max|Q_float - Q_exact| / max|Q_exact|, floored at one rounding of the result (2^-53).
def device_quantities(name, mode):
    kw = dict(mv.EXACT_CASES)[name]
    inner = lambda a, c: a[c["Hy"]:c["Hy"] + c["Ny"], c["Hx"]:c["Hx"] + c["Nx"]].copy()
    q = {}
    c, m, _, _ = build(kw, "viscous_split", mode, substeps=1, reference=False)
    csi.time_step_momentum(m, c["dt"])
    m.synchronize()
    q["visc_v"], q["visc_u"] = inner(m.velocities.v.numpy(), c), inner(m.velocities.u.numpy(), c)
    for rheology in ("viscous", "evp"):
        c, m, _, _ = build(kw, rheology + "_explicit", mode, reference=False, timestepper="ForwardEuler")
        csi.compute_momentum_tendencies(m, mv.EXACT_DT)
        csi.time_step_momentum(m, mv.EXACT_DT)
        m.synchronize()
        q[f"G{rheology}_u"], q[f"G{rheology}_v"] = inner(m.timestepper.Gn.u.numpy(), c), inner(m.timestepper.Gn.v.numpy(), c)
        q[f"step{rheology}_u"], q[f"step{rheology}_v"] = inner(m.velocities.u.numpy(), c), inner(m.velocities.v.numpy(), c)
    return q


@pytest.mark.parametrize("name", [n for n, _ in mv.EXACT_CASES])
def test_strict_and_fast_against_exact_arithmetic(name, oracle_lib):
    ref = mv.exact_references(name)
    strict, fast = device_quantities(name, "strict"), device_quantities(name, "fast")
    assert sorted(ref) == sorted(strict) == sorted(fast)
    failures = []
    for quantity, (Qf, Qx) in ref.items():
        e_ref = rel_error(Qf, Qx, CTX)
        e_strict, e_fast = rel_error(strict[quantity], Qx, CTX), rel_error(fast[quantity], Qx, CTX)
        ratio = e_fast / max(e_ref, U)
        print(f"[fast-error] {name} | {quantity} | e_ref {e_ref / U:.2f} u | STRICT {e_strict / U:.2f} u | FAST {e_fast / U:.2f} u | ratio {ratio:.2f}")
        if not e_strict == e_ref:                           # STRICT is the restatement: the same error, not a similar one
            failures.append((quantity, "STRICT", e_strict, e_ref))
        if not e_fast <= mv.K_FAST * max(e_ref, U):
            failures.append((quantity, "FAST", e_fast, e_ref, ratio))
    assert not failures, (name, failures)
