"""The momentum, advection and diagnostic kernels off the default parameters and on rectangular cells (tests/evp_parameter_sets.py).

Every other GPU test takes square cells on the uniform-metric grids and the default rheology / dynamics numbers, so a dx written for a
dy in the uniform family's coefficients, a host-folded FAST constant that is only right at e = 2, or a constant left at its default
anywhere between the front end and a kernel passes them.  Here, for default/rectangular, A/square, A/rectangular and B/rectangular
(a failure names the axis), on 40 x 28 (one tile), 130 x 33 periodic and bounded (three strips, the last ragged), a masked channel, a
north fold, and for A and B a lat-lon and a curvilinear grid:

  * STRICT equals the oracle bit for bit after 1, 2, 7 and 12 sub-steps (P copied from the oracle: exp());
  * FAST on the three kernels equals the oracle after 1 and 2 sub-steps on test_gpu_evp.test_fast_few_substeps_tight's bounds, with the
    zero-velocity sets and the alpha plateaus (at the set's alpha-, alpha+) identical and alpha, zeta, Delta on
    test_fast_vs_oracle_full_cycle's bounds;
  * fusion levels 1 and 2 equal level 0 bit for bit after 1, 2, 7 and 12 sub-steps, the pair kernel asserted where it is expected, and
    the north-fold band, through its fused launches and through the three kernels plus copies, equals the three-kernel run;
  * the pair kernel restarted from every second state of the oracle's 12-sub-step cycle stays on the tight bounds;
  * StressBalanceFreeDrift, whose marginal select reads minimum_mass / minimum_concentration.
Beyond the EVP sub-cycle, one rectangular-cell case each through the comparison of the path's own test file: ViscousRheology(nu = 3.7e3)
and the ExplicitSolver, the advection schemes and the extra tracers, a whole RK3 step, the momentum terms and their power, the derived
fields and the energy budget, the advection timescale.  tests/test_evp_parameters.py shows on the CPU that the sets reach the branches.
"""
import math

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import evp_parameter_sets as ps
from test_gpu_evp import EVP_FIELDS, cmp_region, gpu_fields

pytestmark = pytest.mark.gpu

PP, BB, PB, PF = ("periodic", "periodic"), ("bounded", "bounded"), ("periodic", "bounded"), ("periodic", "folded")
GRIDS = {
    "p40x28": dict(Nx=40, Ny=28, topo=PP, random_uv=0.03),                    # one tile, under one block in x
    "p130x33": dict(Nx=130, Ny=33, topo=PP, random_uv=0.05),                  # three 56-column strips, the last ragged
    "b130x33": dict(Nx=130, Ny=33, topo=BB, random_uv=0.05),
    "masked_channel": dict(Nx=72, Ny=40, topo=PB, land=0.2, random_uv=0.03),
    "folded": dict(Nx=64, Ny=48, topo=PF, random_uv=0.05),
}
METRIC_GRIDS = {                                                               # only the parameters are new there
    "latlon": dict(Nx=48, Ny=40, topo=PB, grid="latlon", random_uv=0.03),
    "curvilinear": dict(Nx=48, Ny=36, topo=PP, curvilinear=0.1, random_uv=0.03),
}
CASES = [(cell, grid) for cell in ps.CELLS for grid in GRIDS] + [(cell, grid) for cell in ("A_rect", "B_rect") for grid in METRIC_GRIDS]
SET_NAME = {"A_rect": "A", "B_rect": "B"}          # make() drops `cell` on the lat-lon grid: only the parameters are new there
IDS = [f"{SET_NAME[cell] if grid == 'latlon' else cell}-{grid}" for cell, grid in CASES]
ONLY_PAIR_FUSES = ("masked_channel", "curvilinear")         # no one-sub-step fused kernel takes a mask or metric planes
SUBSTEPS = [1, 2, 7, 12]


def make(cell, grid, **kw):
    k = dict(GRIDS.get(grid) or METRIC_GRIDS[grid], **ps.CELLS[cell])
    if k.get("grid") == "latlon":
        k.pop("cell", None)
    k.update(kw)
    return cases.make_case(**k)


def scales(p):
    return (max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max()),
            max(np.abs(p.f["s11"]).max(), np.abs(p.f["s22"]).max(), np.abs(p.f["s12"]).max()))


@pytest.mark.parametrize("cell", list(ps.CELLS))
def test_the_model_carries_the_set(cell):
    """front end -> csi_evp_params: the rheology, the momentum equation and the model hold the set's numbers, alpha is pre-filled with
    the set's alpha+, and the grid's metrics are the rectangular cell's"""
    c = make(cell, "p40x28")
    m = cases.csi_model(c, mode="fast")
    prm, r = ps.params_of(c), m.dynamics.rheology
    got = dict(P_star=r.ice_compressive_strength, C_star=r.ice_compaction_hardening, ecc=r.yield_curve_eccentricity,
               delta_min=r.minimum_plastic_stress, alpha_min=r.min_relaxation_parameter, alpha_max=r.max_relaxation_parameter,
               c_alpha=r.relaxation_strength, min_mass=m.dynamics.minimum_mass, min_conc=m.dynamics.minimum_concentration,
               rho_ice=m.sea_ice_density)
    assert got == prm
    assert np.all(m.dynamics.auxiliaries.fields.alpha.numpy() == prm["alpha_max"])
    met = c["g"].metrics()
    assert (met["dx"], met["dy"]) == ps.CELLS[cell].get("cell", (c["spacing"],) * 2)


# ---- 1. STRICT against the oracle, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsub", SUBSTEPS)
@pytest.mark.parametrize("cell,grid", CASES, ids=IDS)
def test_strict_bitwise_vs_oracle(cell, grid, nsub, oracle_lib):
    c = make(cell, grid, substeps=nsub)
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode="strict")
    for k in ("u", "v"):
        assert np.array_equal(EVP_FIELDS[k](m).numpy(), p.f[k]), f"{k} after update_state!"
    p.initialize_rheology()
    m.ctx.call("csi_evp_initialize")
    g = gpu_fields(m)
    ulp = int(np.abs(np.ascontiguousarray(g["P"]).view(np.int64) - p.f["P"].view(np.int64)).max())
    assert ulp <= 4, ("P", ulp)                                      # exp(): device libm against glibc
    m.copy_to_field(m.dynamics.auxiliaries.fields.P, p.f["P"])
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    p.subcycle(c["dt"], 1, nsub)
    p.L.ora_finalize_rheology(p.ptr)
    m.ctx.call("csi_evp_subcycle", c["dt"], nsub, 1)
    m.ctx.call("csi_evp_finalize")
    g = gpu_fields(m)
    for k in ("u", "v", "s11", "s22", "s12", "alpha", "zeta_c", "zeta_f", "Delta"):          # whole parents
        assert np.all(np.isfinite(g[k])), k
        assert np.array_equal(g[k], p.f[k]), f"{cell} {grid}: {k} differs, max abs diff {np.abs(g[k] - p.f[k]).max():.3e}"
    assert np.abs(g["u"]).max() > 0 and np.abs(g["s11"]).max() > 0


# ---- 2. FAST, three kernels, against the oracle after 1 and 2 sub-steps ----------------------------------------------------------------
@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("cell,grid", CASES, ids=IDS)
def test_fast_three_kernels_few_substeps_tight(cell, grid, nsub, oracle_lib):
    """The bounds are test_gpu_evp's own: 1e-13 max|u| on u, v and 1e-10 max|sigma| on sigma (test_fast_few_substeps_tight); alpha within
    1e-11 alpha+ and zeta, Delta within 1e-10 of their maxima (test_fast_vs_oracle_full_cycle), with the set's alpha+ for the 300 there."""
    c = make(cell, grid, substeps=nsub)
    prm = ps.params_of(c)
    p = cases.oracle_problem(c)
    p.time_step_momentum(c["dt"])
    m = cases.csi_model(c, mode="fast")
    m.set_fusion(0)
    csi.time_step_momentum(m, c["dt"])
    g = gpu_fields(m)
    assert m.ctx.last_path()["level"] == 0
    vmax, smax = scales(p)
    for f in ("u", "v"):
        d = np.abs(g[f] - p.f[f]).max()
        print(cell, grid, nsub, f, d / vmax)
        assert np.all(np.isfinite(g[f])) and d <= 1e-13 * vmax, (f, d, vmax)
        assert np.array_equal(g[f] == 0.0, p.f[f] == 0.0), (f, "zero sets differ")
    for f in ("s11", "s22", "s12"):
        d = np.abs(cmp_region(c, f, g[f]) - cmp_region(c, f, p.f[f])).max()
        print(cell, grid, nsub, f, d / smax)
        assert d <= 1e-10 * smax, (f, d, smax)
    ga, pa = cmp_region(c, "alpha", g["alpha"]), cmp_region(c, "alpha", p.f["alpha"])
    for bound in (prm["alpha_min"], prm["alpha_max"]):
        assert np.array_equal(ga == bound, pa == bound), ("alpha plateau", bound)
    assert np.abs(ga - pa).max() <= 1e-11 * prm["alpha_max"]
    for k in ("zeta_c", "zeta_f", "Delta"):
        scale = np.abs(p.f[k]).max()
        assert np.abs(cmp_region(c, k, g[k]) - cmp_region(c, k, p.f[k])).max() <= 1e-10 * scale, k


# ---- 3. the fused kernels equal the three kernels bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("nsub", SUBSTEPS)
@pytest.mark.parametrize("cell,grid", CASES, ids=IDS)
def test_fused_kernels_bitwise_equal_three_kernel_path(cell, grid, nsub):
    """test_gpu_evp.test_fused_kernels_bitwise_equal_three_kernel_path's fields and regions: level 1 on whole parents; level 2 on whole
    parents of u, v, sigma11, sigma22 (sigma12: without walls) and on the interiors of the diagnostics and of sigma12 next to walls."""
    c = make(cell, grid, substeps=nsub)
    walls = "bounded" in c["topo"] or "folded" in c["topo"]
    out, level = {}, {}
    for fusion in (0, 1, 2):
        m = cases.csi_model(c, mode="fast")
        m.set_fusion(fusion)
        csi.time_step_momentum(m, c["dt"])
        m.synchronize()
        level[fusion] = m.ctx.last_path()["level"]
        assert m.ctx.launches_per_substep() == (1 if level[fusion] else 3)
        out[fusion] = {k: EVP_FIELDS[k](m).numpy().copy() for k in ("u", "v", "s11", "s22") + (() if walls else ("s12",))}
        out[fusion].update({k: (EVP_FIELDS[k](m).numpy().copy(), EVP_FIELDS[k](m).interior_numpy().copy())
                            for k in ("alpha", "zeta_c", "zeta_f", "Delta") + (("s12",) if walls else ())})
    single = 0 if (grid in ONLY_PAIR_FUSES or grid == "folded") else 1
    assert level[0] == 0 and level[1] == single, level
    assert level[2] == (2 if nsub >= 2 else single), level                      # the pair kernel (below the band of a north fold)
    if level[2] == 2 and grid != "folded":
        assert m.ctx.last_launches() == ((nsub + 1) // 2, nsub)
    assert np.abs(out[0]["u"]).max() > 0
    for fusion in (1, 2):
        for k in out[0]:
            a, b = out[0][k], out[fusion][k]
            if isinstance(a, tuple):
                a, b = (a[1], b[1]) if level[fusion] == 2 else (a[0], b[0])
            assert np.all(np.isfinite(b)), k
            assert np.array_equal(a, b), (cell, grid, nsub, fusion, k, np.abs(a - b).max(), np.argwhere(a != b)[:5])


def band_env(monkeypatch, fused):
    """the fold band's launch variant of the contexts created from here on (the knob is read when a context is created)"""
    if fused:
        monkeypatch.delenv("CSI_BAND_FUSED", raising=False)
    else:
        monkeypatch.setenv("CSI_BAND_FUSED", "0")


@pytest.mark.parametrize("band", ["band_fused", "band_unfused"])
@pytest.mark.parametrize("nsub", [2, 7, 12])
@pytest.mark.parametrize("cell", list(ps.CELLS))
def test_north_fold_band_bitwise(cell, nsub, band, monkeypatch):
    """test_gpu_evp.test_north_fold_band_bitwise's comparison: the pair kernel below the fold and the band of rows next to it against
    the three kernels on the whole grid, two sub-cycles in a row.  The band runs either through its own fused launches (the default,
    csi_fold.hip band_substeps_fused) or, with CSI_BAND_FUSED=0, through the three kernels and two copies per step (band_substep):
    separate host launch code with its own row ranges, fed the same host-folded coefficients.  That the knob took effect shows in the
    launch count of a sub-cycle, which is smaller with the fused band: a model of the other variant is run beside for that count."""
    fused = band == "band_fused"
    band_env(monkeypatch, fused)
    c = make(cell, "folded", substeps=nsub)
    ref = cases.csi_model(c, mode="fast"); ref.set_fusion(0)
    new = cases.csi_model(c, mode="fast")
    for _ in range(2):
        csi.time_step_momentum(ref, c["dt"]); csi.time_step_momentum(new, c["dt"])
    ref.synchronize(); new.synchronize()
    assert ref.ctx.last_path()["level"] == 0 and new.ctx.last_path()["level"] == 2
    band_env(monkeypatch, not fused)
    other = cases.csi_model(c, mode="fast")
    for _ in range(2):
        csi.time_step_momentum(other, c["dt"])
    other.synchronize()
    assert other.ctx.last_path()["level"] == 2
    launches = {fused: new.ctx.last_launches()[0], (not fused): other.ctx.last_launches()[0]}
    assert launches[True] < launches[False], launches
    for f in ("u", "v", "s11", "s22", "s12"):
        a, b = cmp_region(c, f, EVP_FIELDS[f](ref).numpy()), cmp_region(c, f, EVP_FIELDS[f](new).numpy())
        assert np.all(np.isfinite(b)), f
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])
    for f in ("alpha", "zeta_c", "zeta_f", "Delta"):
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](new).interior_numpy()
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])


# ---- 4. the pair kernel restarted from the oracle's states -----------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["p40x28", "b130x33"])
@pytest.mark.parametrize("cell", list(ps.CELLS))
def test_fast_two_substeps_from_every_state_of_the_oracle_cycle(cell, grid, oracle_lib):
    """test_gpu_evp's restart test over a 12-sub-step cycle: six restarts from the oracle's state (u, v, sigma, P, u^n, v^n, parents),
    two sub-steps through the pair kernel beside it, each on the tight bounds.  With the 1- and 2-sub-step comparison above this stands
    in for a long-cycle comparison and its sensitivity branch."""
    nsub = 12
    c = make(cell, grid, substeps=nsub)
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode="fast")
    p.initialize_rheology()
    m.ctx.call("csi_evp_initialize")
    m.synchronize()
    for s in range(1, nsub, 2):
        for k in ("u", "v", "s11", "s22", "s12", "P", "un", "vn"):
            EVP_FIELDS[k](m).data.copy_(torch.from_numpy(np.ascontiguousarray(p.f[k])))
        torch.cuda.synchronize()
        p.subcycle(c["dt"], s, s + 1)
        m.ctx.call("csi_evp_subcycle", float(c["dt"]), 2, s)
        g = gpu_fields(m)
        assert m.ctx.last_path()["level"] == 2, "the two sub-steps did not run through the pair kernel"
        vmax, smax = scales(p)
        for k in ("u", "v"):
            d = np.abs(g[k] - p.f[k]).max()
            assert np.all(np.isfinite(g[k])) and d <= 1e-13 * vmax, (cell, "sub-steps", s, s + 1, k, d, vmax)
            assert np.array_equal(g[k] == 0.0, p.f[k] == 0.0), (cell, s, k, "zero set")
        for k in ("s11", "s22", "s12"):
            d = np.abs(EVP_FIELDS[k](m).interior_numpy() - p.interior(k)).max()
            assert d <= 1e-10 * smax, (cell, "sub-steps", s, s + 1, k, d, smax)


# ---- 5. free drift: the marginal select reads minimum_mass / minimum_concentration ------------------------------------------------------
def free_drift_case(cell, **kw):
    """64 x 48 periodic, number-valued stresses; rows [0.4 Ny, 0.7 Ny) hold the set's thin-ice values (tests/evp_parameter_sets.py: they
    change branch between the set's thresholds and the default ones)"""
    from free_drift_ref import marginal_band
    c = make(cell, "p40x28", Nx=64, Ny=48, ue=0.05, ve=-0.02, top=(0.03, -0.02), free_drift=True, **kw)
    if ps.CELLS[cell].get("marginal") is None:
        return marginal_band(c)
    rows = cases.marginal_rows(ps.CELLS[cell]["marginal"])
    j0, jm, j1 = int(0.4 * c["Ny"]), int(0.55 * c["Ny"]), int(0.7 * c["Ny"])
    for (a, h), sl in zip(rows, (slice(j0, jm), slice(jm, j1))):
        c["a"][sl, :], c["h"][sl, :] = a, h
    return c


@pytest.mark.parametrize("cell", list(ps.CELLS))
def test_stress_balance_free_drift(cell, oracle_lib):
    """tests/test_gpu_free_drift.py's comparisons with the oracle's StressBalanceFreeDrift: STRICT bit for bit after 7 sub-steps, FAST on
    the tight bounds after 1 and 2 with identical zero sets, every fusion level equal; at least 10 % of the u and v points take the
    free-drift branch under the set's thresholds, and the result is not the one without free drift."""
    from free_drift_ref import free_drift_points
    c = free_drift_case(cell, substeps=7)
    p = cases.oracle_problem(c)
    fu, fv = free_drift_points(p, "u").mean(), free_drift_points(p, "v").mean()
    assert fu >= 0.10 and fv >= 0.10, (fu, fv)
    branches = ps.face_branches(c["h"], c["a"], ps.params_of(c))
    assert np.array_equal(branches["u"][1], free_drift_points(p, "u")[:c["Ny"], :c["Nx"]])          # (no land: marginal = takes the free drift)
    m = cases.csi_model(c, mode="strict")
    p.initialize_rheology()
    m.ctx.call("csi_evp_initialize")
    m.copy_to_field(m.dynamics.auxiliaries.fields.P, p.f["P"])
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    p.subcycle(c["dt"], 1, 7)
    p.L.ora_finalize_rheology(p.ptr)
    m.ctx.call("csi_evp_subcycle", c["dt"], 7, 1)
    m.ctx.call("csi_evp_finalize")
    g = gpu_fields(m)
    for k in ("u", "v", "s11", "s22", "s12"):
        assert np.all(np.isfinite(g[k])) and np.array_equal(g[k], p.f[k]), (k, np.abs(g[k] - p.f[k]).max())
    none = cases.csi_model(dict(c, free_drift=False), mode="strict")
    none.ctx.call("csi_evp_initialize")
    none.ctx.call("csi_evp_subcycle", c["dt"], 7, 1)
    none.synchronize()
    assert not np.array_equal(none.velocities.u.numpy(), g["u"])
    for k in (1, 2):
        ck = dict(c, substeps=k)
        p = cases.oracle_problem(ck)
        p.time_step_momentum(c["dt"])
        out = {}
        for fusion in (0, 1, 2):
            m = cases.csi_model(ck, mode="fast")
            m.set_fusion(fusion)
            csi.time_step_momentum(m, c["dt"])
            out[fusion] = gpu_fields(m)
        assert m.ctx.last_path()["level"] == (2 if k == 2 else 0)       # (free drift: only the pair kernel fuses)
        vmax, smax = scales(p)
        for f in ("u", "v"):
            assert np.abs(out[0][f] - p.f[f]).max() <= 1e-13 * vmax, (k, f)
            assert np.array_equal(out[0][f] == 0.0, p.f[f] == 0.0), (k, f, "zero sets differ")
        for f in ("s11", "s22", "s12"):
            assert np.abs(cmp_region(c, f, out[0][f]) - cmp_region(c, f, p.f[f])).max() <= 1e-10 * smax
        for fusion in (1, 2):
            for f in ("u", "v", "s11", "s22"):
                assert np.array_equal(out[0][f], out[fusion][f]), (k, fusion, f)


# ---- beyond the EVP sub-cycle ----------------------------------------------------------------------------------------------------------
NU = 3.7e3
VARIANT_CASES = {
    "A_rect_channel_130x9": dict(Nx=130, Ny=9, H=4, topo=PB, random_uv=0.03, u0=0.05, **ps.CELLS["A_rect"]),
    "B_rect_walls_65x17": dict(Nx=65, Ny=17, H=(5, 3), topo=BB, random_uv=0.03, u0=0.05, **ps.CELLS["B_rect"]),
}


@pytest.mark.parametrize("configuration", ["viscous_split", "viscous_explicit", "evp_explicit"])
@pytest.mark.parametrize("name", list(VARIANT_CASES))
def test_viscous_and_explicit_momentum_on_rectangular_cells(name, configuration, oracle_lib):
    """tests/test_gpu_momentum_variant_shapes.py's comparison: STRICT equals tests/momentum_ref.py bit for bit on whole parents (the
    launch counts first), FAST stays within 1e-12 max|u| of STRICT with STRICT's zeros; nu = 3.7e3 instead of the default."""
    import momentum_variant_shapes as mv
    from momentum_ref import Ref
    from test_gpu_momentum_variant_shapes import assert_parent, bits, run, run_ref
    from test_gpu_momentum_variants import model_of
    viscous, explicit = configuration.startswith("viscous"), configuration.endswith("explicit")
    substeps = mv.SPLIT_SUBSTEPS
    c = cases.make_case(substeps=substeps, **VARIANT_CASES[name])
    out = {}
    for mode in ("strict", "fast"):
        p = cases.oracle_problem(c)
        m = model_of(c, rheology=csi.ViscousRheology(nu=NU) if viscous else None,
                     solver=csi.ExplicitSolver() if explicit else csi.SplitExplicitSolver(substeps=substeps), mode=mode,
                     timestepper="SplitRungeKutta3" if explicit else "ForwardEuler")
        if not viscous:
            for k, a in mv.seed_sigma(p).items():
                m.copy_to_field(getattr(m.dynamics.auxiliaries.fields, k), a)
        if explicit:
            rng = np.random.default_rng(9)
            for k, fld in (("um", m.timestepper.Psi_minus.u), ("vm", m.timestepper.Psi_minus.v)):
                a = p.f[k[0]] + 0.01 * rng.standard_normal(p.f[k[0]].shape)
                p.f[k][...] = a
                m.copy_to_field(fld, a)
        out[mode] = run(m, c, configuration)
        if mode == "strict":
            want = run_ref(Ref(p, nu=NU, viscous=viscous), p, c, configuration)
            assert sorted(out[mode]) == sorted(want)
            for k in sorted(want):
                assert_parent((name, configuration, k), out[mode][k], want[k])
                assert np.abs(want[k]).max() > 0, k
    for pair in ([("u", "v")] if configuration == "viscous_split" else [("Gu", "Gv"), ("u_rk0", "v_rk0"), ("u_rk1", "v_rk1")]):
        vmax = max(np.abs(out["strict"][k]).max() for k in pair)
        for k in pair:
            s = out["strict"][k]
            d = np.abs(out["fast"][k] - s).max()
            assert np.isfinite(d) and d <= 1e-12 * vmax, (name, configuration, k, d, vmax)
            assert np.array_equal(bits(out["fast"][k])[s == 0.0], bits(s)[s == 0.0]), (name, configuration, k, "zeros differ")


ADVECTION_GRIDS = {"periodic": dict(topo=PP), "bounded": dict(topo=BB), "masked_channel": dict(topo=PB, land=0.2)}


def advection_case(grid, cell=ps.RECT_A):
    rng = np.random.default_rng(9)
    kw = ADVECTION_GRIDS[grid]
    c = cases.make_case(Nx=150, Ny=21, H=4, cell=cell, patches=False, noise=0.0, **kw)
    topo = kw["topo"]
    wet = np.ones(c["h"].shape, bool) if c["mask"] is None else c["mask"].astype(bool)
    c["u"] = 0.4 * rng.standard_normal(c["u"].shape)
    c["v"] = 0.4 * rng.standard_normal(c["v"].shape)
    if topo[0] == "bounded":
        c["u"][:, 0] = 0.0; c["u"][:, -1] = 0.0
    if topo[1] == "bounded":
        c["v"][0, :] = 0.0; c["v"][-1, :] = 0.0
    c["h"] = np.where(wet, 0.3 + 0.2 * rng.random(wet.shape), 0.0)
    c["a"] = np.where(wet, np.clip(0.5 + 0.6 * rng.random(wet.shape), 0, 1), 0.0)
    return c


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("scheme", [7, 5, 3, 1])
@pytest.mark.parametrize("grid", list(ADVECTION_GRIDS))
def test_tracer_tendencies_and_update_on_rectangular_cells(grid, scheme, mode, oracle_lib):
    """tests/test_gpu_steps.py's test_tracer_tendencies_and_update_bitwise with dx = 3000, dy = 1250: the face areas Ax = dy, Ay = dx of
    the flux form are not interchangeable (STRICT bit for bit; FAST on that file's stated tolerances, zero sets identical)."""
    from test_gpu_steps import same_tendency
    c = advection_case(grid)
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode=mode, timestepper="SplitRungeKutta3")
    p.compute_tracer_tendencies(scheme)
    m.ctx.call("csi_compute_tracer_tendencies", scheme)
    m.synchronize()
    for k, f in (("Gh", m.timestepper.Gn.h), ("Ga", m.timestepper.Gn.aice)):
        got, want = f.interior_numpy(), p.interior(k)
        assert np.abs(want).max() > 0
        same_tendency(mode, got, want, k)
    p.L.ora_dynamic_step_tracers(p.ptr, 120.0, 0)
    m.ctx.call("csi_dynamic_step_tracers", 120.0, 0)
    m.synchronize()
    same_tendency(mode, m.ice_thickness.interior_numpy(), p.interior("h"), "h")
    same_tendency(mode, m.ice_concentration.interior_numpy(), p.interior("aice"), "aice")
    if mode == "fast":
        m.ice_thickness.set(p.interior("h").copy()); m.ice_concentration.set(p.interior("aice").copy())
    p.f["hm"][...] = p.f["h"]; p.f["am"][...] = p.f["aice"]
    m.ctx.call("csi_cache_current_fields")
    p.L.ora_dynamic_step_tracers(p.ptr, 40.0, 1)
    m.ctx.call("csi_dynamic_step_tracers", 40.0, 1)
    m.synchronize()
    same_tendency(mode, m.ice_thickness.interior_numpy(), p.interior("h"), "h (RK)")
    same_tendency(mode, m.ice_concentration.interior_numpy(), p.interior("aice"), "aice (RK)")
    # the reference with dx and dy exchanged is another answer: the comparison above sees the cell's shape
    q = cases.oracle_problem(advection_case(grid, cell=ps.RECT_A[::-1]))
    q.compute_tracer_tendencies(scheme)
    assert np.abs(q.interior("Gh") - p.interior("Gh")).max() > 1e-3 * np.abs(p.interior("Gh")).max()


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("topo", ["pp", "bb"])
def test_extra_tracers_on_rectangular_cells(topo, mode, oracle_lib):
    """csrc/tracers.hip through tests/test_gpu_tracers.py's reference: three tracers of mixed weighting, four schemes, hand-placed land,
    130 x 9 cells of 3000 m x 1250 m.  G: STRICT bit for bit, FAST within G_TOL; c bit for bit given the device's own G."""
    import test_gpu_tracers as tt
    import tracers_ref as tr
    c = tt.flow_case(130, 9, tt.TOPOS[topo], 0, cell=ps.RECT_A)
    assert c["g"].metrics()["dx"] == 3000.0 and c["g"].metrics()["dy"] == 1250.0
    specs = tt.specs_of(3)
    m = tt.model_of(c, specs, mode=mode, stepper="ForwardEuler")
    p, ts = tt.ref_of(c, specs)
    start = {k: p.f[k].copy() for k in ("h", "aice")}
    start_c = [t["c"].copy() for t in ts]
    dt = c["dt"]
    for scheme in (7, 5, 3, 1):
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
        assert m.ctx.tracers_last() == tt.expected_layout(3)
        want = [tr.tendency(p, scheme, t["c"], t["weighted"]) for t in ts]
        got = [tt.G_of(m, s) for s in specs]
        for s, g_, w_ in zip(specs, got, want):
            assert np.abs(w_).max() > 0
            tt.same_G(mode, g_, w_, (topo, scheme, "G", s.name))
        if mode == "fast":
            tt.sync_oracle_to_device(p, m, ("Gh", "Ga"))
        tr.stage_first(p, ts, scheme, dt, G_given=got)
        p.dynamic_step_tracers(dt, False)
        m.ctx.call("csi_dynamic_step_tracers", dt, 0)
        if mode == "fast":
            tt.sync_oracle_to_device(p, m, ("h", "aice"))
        tr.stage_second(p, ts, dt)
        m.ctx.tracers_update(dt)
        m.synchronize()
        for t, s in zip(ts, specs):
            got_c = m.tracer(s.name).numpy()
            assert np.array_equal(got_c, t["c"]), (topo, scheme, s.name, np.argwhere(got_c != t["c"])[:4])


@pytest.mark.parametrize("grid", ["p40x28", "masked_channel"])
def test_full_rk3_step_with_set_A_vs_oracle(grid, oracle_lib):
    """tests/test_gpu_steps.py's test_full_time_step_vs_oracle (its tolerances): two RK3 steps with WENO7 and 12 sub-steps, set A on
    3000 m x 1250 m cells."""
    c = make("A_rect", grid, substeps=12)
    for mode, tol in (("strict", 1e-12), ("fast", 1e-11)):
        p = cases.oracle_problem(c)
        m = cases.csi_model(c, mode=mode, timestepper="SplitRungeKutta3", advection=csi.WENO(order=7))
        for n in range(2):
            p.time_step_rk3(c["dt"], 7)
            csi.time_step(m, c["dt"])
        m.synchronize()
        vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max())
        for k, f in (("u", m.velocities.u), ("v", m.velocities.v)):
            assert np.abs(f.numpy() - p.f[k]).max() <= tol * vmax, (mode, k)
        for k, f in (("h", m.ice_thickness), ("aice", m.ice_concentration)):
            assert np.abs(f.numpy() - p.f[k]).max() <= tol * np.abs(p.f[k]).max(), (mode, k)
            assert np.array_equal(f.numpy() == 0.0, p.f[k] == 0.0), (mode, k, "zero set")
        assert not np.array_equal(p.interior("h"), c["h"])


@pytest.mark.parametrize("cell", ["A_rect", "B_rect"])
def test_momentum_terms_and_power_on_rectangular_cells(cell, oracle_lib):
    """tests/test_gpu_momentum_terms.py's comparison: the ten term fields, both interface stresses and the five powers equal
    momentum_terms_ref.TermsRef bit for bit in both modes; the restatement reads the set's thresholds and density from the problem."""
    import diagnostics_ref as dref
    import momentum_terms_ref as ref
    from test_gpu_momentum_terms import check_fields, evp_pair
    c, p, m = evp_pair(dict(Nx=65, Ny=33, topo=PB, random_uv=0.03, user_forcing=True, wind_drag="numbers", **ps.CELLS[cell]))
    assert p.s.rho_ice == m.sea_ice_density == ps.params_of(c)["rho_ice"]
    t = ref.TermsRef(p)
    want = check_fields(m, t, cell)
    assert all(np.abs(want[n]).max() > 0 for n in ref.FIELDS)
    b = m.momentum_budget()
    for k, v in t.budget().items():
        assert math.isfinite(v) and dref.same_bits(getattr(b, k), v), (cell, k, getattr(b, k), v)


@pytest.mark.parametrize("cell", ["A_rect", "B_rect"])
def test_derived_fields_and_budget_on_rectangular_cells(cell):
    """tests/test_gpu_derived.py's comparison (derived_ref.Ref, rho = the set's) for the seven fields and the three sums, bit for bit in
    both modes."""
    import derived_ref as ref
    import diagnostics_ref as dref
    from test_gpu_derived import budget_bits, load, set_land
    c = make(cell, "p40x28", Nx=65, Ny=33, topo=PB, substeps=4, patches=False)
    g = c["g"]
    m = cases.csi_model(c, mode="fast")
    assert m.sea_ice_density == ps.params_of(c)["rho_ice"] != 900.0
    for land in (False, True):
        par, wet = ref.white_noise(g, seed=11 + land, land=land, poison="derived")
        mask = set_land(m, wet)
        load(m, par)
        want = ref.Ref(g, par, mask).fields()
        for mode in ("strict", "fast"):
            m.set_mode(mode)
            fields = m.compute_derived(*ref.NAMES)
            m.synchronize()
            for n, fld in zip(ref.NAMES, fields):
                got = fld.interior_numpy()
                assert np.all(np.isfinite(got)) and ref.same_bits(got, want[n]), (n, mode, land, np.argwhere(got != want[n])[:4])
        par, _ = ref.white_noise(g, seed=11 + land, land=land, poison="budget")
        load(m, par)
        sums = ref.Ref(g, par, mask, rho=m.sea_ice_density).budget()
        assert all(math.isfinite(v) for v in sums.values())
        assert not all(dref.same_bits(sums[k], v) for k, v in ref.Ref(g, par, mask, rho=900.0).budget().items())
        for mode in ("strict", "fast"):
            m.set_mode(mode)
            assert budget_bits(m.energy_budget(), sums) == [], (mode, land)


@pytest.mark.parametrize("cell", ["A_rect", "B_rect"])
def test_advection_timescale_on_rectangular_cells(cell):
    """tests/test_gpu_diagnostics.py's comparison (diagnostics_ref) for the advection timescale 1 / max(|u| / dx + |v| / dy) and the
    velocity maxima, bit for bit in both modes, on the state after one RK3 step."""
    import diagnostics_ref as dref
    m2 = cases.csi_model(make(cell, "p130x33", substeps=4), mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    csi.time_step(m2, 120.0)
    keys = ("inv_timescale_max", "advection_timescale", "max_abs_u", "max_abs_v")
    want = dref.of_model(m2, what="velocity")
    for mode in ("strict", "fast"):
        m2.set_mode(mode)
        rec = m2.diagnostics("velocity")
        assert not dref.compare(rec, want, keys), dref.compare(rec, want, keys)
    assert rec.advection_timescale > 0 and math.isfinite(rec.advection_timescale)
