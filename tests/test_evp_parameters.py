"""The conditions the parameter sets of tests/evp_parameter_sets.py must meet, on the CPU oracle alone (no GPU).

The GPU tests on these sets (tests/test_gpu_evp_parameters.py) compare kernels with the oracle; that only says something where the oracle's
state reaches the branches the parameters select.  So, for every set, on the 40 x 28 periodic case after a 12-sub-step cycle:
  * alpha sits on the lower clamp, between the clamps and on the upper clamp in at least 5 % of the icy cells each;
  * Delta sits on its floor and above it in at least 5 % each;
  * the active, marginal and zero branches of both velocity steps are non-empty, and the marginal set differs from the one the default
    thresholds give on the same h, aice;
  * the C oracle equals its NumPy twin bit for bit with the set's numbers and separate dx, dy;
  * the oracle's uniform-metric branch with dx != dy equals, bit for bit over a sub-cycle and an RK3 step with WENO7, the same grid
    handed over as twelve metric arrays (a path lat-lon grids already exercise with dx != dy).
With the new keywords of tests/cases.py absent every case is unchanged: tests/test_golden.py and tests/test_momentum_ref_exact.py check
that; test_default_keywords_change_nothing states it for the new keywords given their default values.
"""
import numpy as np
import pytest

import cases
import evp_parameter_sets as ps
import oracle_np as ONP

COVERAGE = dict(Nx=40, Ny=28, topo=("periodic", "periodic"), patches=True, random_uv=0.03, substeps=12)


def cycled(name):
    c = cases.make_case(**dict(COVERAGE, **ps.CELLS[name]))
    p = cases.oracle_problem(c)
    p.time_step_momentum(c["dt"])
    return c, p


@pytest.mark.parametrize("name", list(ps.CELLS))
def test_the_oracle_problem_carries_the_set(name, oracle_lib):
    c = cases.make_case(**dict(COVERAGE, **ps.CELLS[name]))
    p = cases.oracle_problem(c)
    want = ps.params_of(c)
    for k, v in want.items():
        assert getattr(p.s, k) == v, k
    assert np.all(p.f["alpha"] == want["alpha_max"])                      # the pre-filled alpha+
    dx, dy = ps.CELLS[name].get("cell", (c["spacing"], c["spacing"]))
    assert (p.s.dx, p.s.dy) == (dx, dy) and c["g"].metrics()["kind"] == "uniform"
    assert (p.s.pressure_kind != 0) == (ps.CELLS[name].get("pressure") == "ice_strength")


def test_default_keywords_change_nothing(oracle_lib):
    kw = dict(Nx=24, Ny=20, substeps=5, random_uv=0.03)
    a = cases.make_case(**kw)
    b = cases.make_case(cell=(a["spacing"], a["spacing"]), evp=dict(ps.DEFAULTS), marginal=(5e-4, 1e-3), **kw)
    out = []
    for c in (a, b):
        p = cases.oracle_problem(c)
        p.time_step_rk3(c["dt"], 7)
        out.append({k: p.f[k].copy() for k in ("u", "v", "h", "aice", "s11", "s22", "s12", "alpha", "Delta")})
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


@pytest.mark.parametrize("name", ps.PARAMETER_CELLS)
def test_alpha_and_delta_coverage(name, oracle_lib):
    c, p = cycled(name)
    prm = ps.params_of(c)
    icy = (p.interior("h") * p.interior("aice")) > 0
    alpha, delta = p.interior("alpha")[icy], p.interior("Delta")[icy]
    frac = {"alpha == alpha-": (alpha == prm["alpha_min"]).mean(),
            "alpha- < alpha < alpha+": ((alpha > prm["alpha_min"]) & (alpha < prm["alpha_max"])).mean(),
            "alpha == alpha+": (alpha == prm["alpha_max"]).mean(),
            "Delta == Delta_min": (delta == prm["delta_min"]).mean(), "Delta > Delta_min": (delta > prm["delta_min"]).mean()}
    print(name, {k: round(float(v), 3) for k, v in frac.items()})
    for k, v in frac.items():
        assert v >= 0.05, (name, k, v)


@pytest.mark.parametrize("name", ps.PARAMETER_CELLS)
def test_velocity_branches_and_threshold_sensitivity(name, oracle_lib):
    c = cases.make_case(**dict(COVERAGE, **ps.CELLS[name]))
    own = ps.face_branches(c["h"], c["a"], ps.params_of(c))
    dflt = ps.face_branches(c["h"], c["a"], dict(ps.DEFAULTS, rho_ice=ps.params_of(c)["rho_ice"]))
    for comp in ("u", "v"):
        active, marginal, zero = own[comp]
        assert active.sum() > 0 and marginal.sum() > 0 and zero.sum() > 0, (name, comp, active.sum(), marginal.sum(), zero.sum())
        changed = (marginal != dflt[comp][1]).sum()
        print(name, comp, "active / marginal / zero:", int(active.sum()), int(marginal.sum()), int(zero.sum()), "| marginal set changes at", int(changed))
        assert changed >= 4, (name, comp, "the marginal set does not depend on the set's thresholds")
    # the oracle's own selection: after one sub-step with free drift off, the marginal points hold zero, the active ones do not
    c1 = dict(c, substeps=1)
    p = cases.oracle_problem(c1)
    p.time_step_momentum(c1["dt"])
    u = p.interior("u")
    assert np.all(u[own["u"][1]] == 0.0) and np.all(u[own["u"][2]] == 0.0) and np.all(u[own["u"][0]] != 0.0)


@pytest.mark.parametrize("free_drift", [False, True])
@pytest.mark.parametrize("topo", [("periodic", "periodic"), ("bounded", "bounded")], ids=["periodic", "bounded"])
@pytest.mark.parametrize("name", list(ps.CELLS))
def test_c_oracle_equals_numpy_restatement_bitwise(name, topo, free_drift, oracle_lib):
    """tests/test_oracle_properties.py's cross-check with the set's numbers: every parameter is read by both restatements, and dx, dy
    are not interchangeable in either."""
    kw = dict(ps.CELLS[name])
    c = cases.make_case(Nx=28, Ny=22, substeps=6, random_uv=0.05, ue=0.05, ve=-0.02, top=(0.01, 0.02), free_drift=free_drift, topo=topo, **kw)
    p = cases.oracle_problem(c)
    g, prm = c["g"], ps.params_of(c)
    m = g.metrics()
    n = ONP.NP(g.Nx, g.Ny, g.Hx, g.Hy, tuple(0 if t == "periodic" else 1 for t in topo), dx=m["dx"], dy=m["dy"])
    assert ("cell" in kw) == (m["dx"] != m["dy"])
    n.P_star, n.C_star, n.ecc, n.Dmin = prm["P_star"], prm["C_star"], prm["ecc"], prm["delta_min"]
    n.amin, n.amax, n.ca = prm["alpha_min"], prm["alpha_max"], prm["c_alpha"]
    n.min_mass, n.min_conc, n.rho = prm["min_mass"], prm["min_conc"], prm["rho_ice"]
    n.replacement = c["pressure"] == "replacement"
    n.f, n.top, n.bottom = c["coriolis"], ("const",) + tuple(c["top"]), ("semi", c["ue"], c["ve"], 1026.0, 5.5e-3)
    n.free_drift = free_drift
    for k, v in p.f.items():
        n.fld[k] = v.copy()
    p.initialize_rheology()
    n.initialize()
    assert np.abs(p.f["P"] - n.fld["P"]).max() <= 4e-16 * np.abs(p.f["P"]).max()   # exp(): libm vs numpy
    n.fld["P"][...] = p.f["P"]
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    n.fill_halo("u", 1, 0); n.fill_halo("v", 0, 1)
    p.subcycle(c["dt"], 1, 6)
    n.subcycle(c["dt"], 1, 6)
    for k in ("u", "v", "s11", "s22", "s12", "alpha", "zeta_c", "zeta_f", "Delta"):
        assert np.array_equal(p.f[k], n.fld[k]), k


@pytest.mark.parametrize("topo", [("periodic", "periodic"), ("bounded", "bounded"), ("periodic", "bounded")], ids=["pp", "bb", "pb"])
@pytest.mark.parametrize("name", list(ps.CELLS))
def test_uniform_rectangular_cells_equal_the_twelve_metric_arrays(name, topo, oracle_lib):
    """test_full_2d_metrics_reduce_to_the_regular_grids on rectangular cells: the uniform dx / dy branch of the oracle against its
    twelve-array path, over a sub-cycle alone and over a whole RK3 step with WENO7; exchanging dx and dy changes the answer."""
    kw = dict(ps.CELLS[name])
    out = {}
    for curv in (None, 0.0, "swapped"):
        k2 = dict(kw)
        if curv == "swapped":
            dx, dy = kw.get("cell", (2000.0, 2000.0))
            k2["cell"] = (dy, dx)
        c = cases.make_case(Nx=28, Ny=24, substeps=8, topo=topo, random_uv=0.03, curvilinear=0.0 if curv == 0.0 else None, **k2)
        assert c["g"].metrics()["kind"] == ("full" if curv == 0.0 else "uniform")
        p = cases.oracle_problem(c)
        p.time_step_momentum(c["dt"])
        res = {"cycle_" + k: p.f[k].copy() for k in ("u", "v", "s11", "s22", "s12", "alpha", "Delta")}
        p = cases.oracle_problem(c)
        p.time_step_rk3(c["dt"], 7)
        res.update({k: p.f[k].copy() for k in ("u", "v", "h", "aice", "s11", "s12")})
        out[curv] = res
    for k in out[None]:
        assert np.all(np.isfinite(out[None][k])), k
        assert np.array_equal(out[None][k], out[0.0][k]), (name, k)
    if "cell" in kw:
        assert np.abs(out["swapped"]["cycle_u"] - out[None]["cycle_u"]).max() > 1e-6 * np.abs(out[None]["cycle_u"]).max()
        assert np.abs(out["swapped"]["h"] - out[None]["h"]).max() > 1e-9
