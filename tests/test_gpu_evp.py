"""GPU parity tests of the EVP sub-cycle: HIP kernels (through the C ABI) against the CPU oracle.

Tolerances (fp64), also stated in DESIGN.md:
  STRICT mode  : bit-for-bit equal to the oracle on every field, given the same ice strength P
                 (P itself involves exp(): device libm vs glibc may differ in the last bits,
                 checked to <= 4 ulp).
  FAST mode    : differs from the oracle by rounding only (hoisted reciprocals, FMA, shared
                 strain rates).  Measured on MI355X: <= 3e-15 * max|u| on u, v and <= 1e-14 *
                 max|sigma| on sigma after a full 120-sub-step cycle on well-conditioned inputs.
                 Asserted: max|du|, max|dv| <= 1e-12 * max(|u|,|v|), sigma <= 1e-11 * max|sigma|.
                 The mEVP iteration itself is chaotic where the pack is rigid (Delta = Delta_min and
                 gamma > alpha+: a uniformly moving, fully compact pack): there the ORACLE's own
                 answer moves by 1e-3 relative under a 1e-15 relative perturbation of its inputs
                 (scripts/diag_fast_tolerance.py), so for every case the bound is
                 max(stated tolerance, 10 x the oracle's measured self-sensitivity).
                 Threshold decisions (zero-velocity cells, alpha clamp plateaus) agree exactly
                 on the well-conditioned cases.
"""
import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi

pytestmark = pytest.mark.gpu

EVP_FIELDS = {"u": lambda m: m.velocities.u, "v": lambda m: m.velocities.v,
              "s11": lambda m: m.dynamics.auxiliaries.fields.s11, "s22": lambda m: m.dynamics.auxiliaries.fields.s22,
              "s12": lambda m: m.dynamics.auxiliaries.fields.s12, "alpha": lambda m: m.dynamics.auxiliaries.fields.alpha,
              "zeta_c": lambda m: m.dynamics.auxiliaries.fields.zeta_c, "zeta_f": lambda m: m.dynamics.auxiliaries.fields.zeta_f,
              "Delta": lambda m: m.dynamics.auxiliaries.fields.Delta, "P": lambda m: m.dynamics.auxiliaries.fields.P,
              "un": lambda m: m.dynamics.auxiliaries.fields.un, "vn": lambda m: m.dynamics.auxiliaries.fields.vn}

CASES = {
    "periodic_patches": dict(Nx=64, Ny=48, topo=("periodic", "periodic"), patches=True, random_uv=0.05),
    "periodic_full_ice": dict(Nx=96, Ny=80, topo=("periodic", "periodic"), patches=False, random_uv=0.0),
    "bounded": dict(Nx=40, Ny=56, topo=("bounded", "bounded"), patches=True, random_uv=0.05),
    "channel": dict(Nx=48, Ny=40, topo=("periodic", "bounded"), patches=True, random_uv=0.02),
    "latlon_bounded": dict(Nx=40, Ny=40, topo=("bounded", "bounded"), grid="latlon", patches=True, random_uv=0.05),
    "latlon_channel": dict(Nx=64, Ny=40, topo=("periodic", "bounded"), grid="latlon", patches=False, random_uv=0.02),
    "field_forcing": dict(Nx=48, Ny=48, topo=("periodic", "periodic"), patches=True, field_forcing=True, random_uv=0.03),
    "ice_strength_nocoriolis": dict(Nx=32, Ny=32, topo=("periodic", "periodic"), pressure="ice_strength", coriolis=None,
                                    top=None, ue=0.1, patches=False),
    "ragged": dict(Nx=67, Ny=5, H=3, topo=("periodic", "periodic"), patches=False, random_uv=0.05),
    # several 56- / 60-column strips and several row chunks per wave tile: seams of the fused kernels
    "periodic_seams": dict(Nx=150, Ny=100, topo=("periodic", "periodic"), patches=True, random_uv=0.05),
    "periodic_halo6": dict(Nx=70, Ny=37, H=6, topo=("periodic", "periodic"), patches=True, random_uv=0.05),
    "bounded_seams": dict(Nx=141, Ny=90, topo=("bounded", "bounded"), patches=True, random_uv=0.05),
    # immersed land (SURVEY.md 8d config 5 style: discs covering ~30 %); only the two-sub-steps-per-launch kernel takes masks
    "masked_periodic": dict(Nx=130, Ny=84, topo=("periodic", "periodic"), patches=True, random_uv=0.05, land=0.3),
    "masked_channel": dict(Nx=96, Ny=120, topo=("periodic", "bounded"), patches=True, random_uv=0.05, land=0.3),
    "masked_latlon": dict(Nx=72, Ny=64, topo=("bounded", "bounded"), grid="latlon", patches=True, random_uv=0.03, land=0.25),
    # array-valued forcing (the coupled-model case: wind stress arrays on top, ocean velocity arrays in the bottom drag)
    "forced_seams": dict(Nx=150, Ny=70, topo=("periodic", "periodic"), patches=True, field_forcing=True, random_uv=0.03),
    "coupled_channel": dict(Nx=100, Ny=90, topo=("periodic", "bounded"), patches=True, field_forcing=True, random_uv=0.03, land=0.3),
    "coupled_latlon": dict(Nx=64, Ny=72, topo=("bounded", "bounded"), grid="latlon", patches=True, field_forcing=True, random_uv=0.03, land=0.2),
    # StressBalanceFreeDrift for marginal ice (two-sub-steps kernel, FORCE variant; the reference's own tripolar test
    # combines it with stress / ocean-velocity arrays and an immersed grid, test/distributed_tests_utils.jl:190-212)
    "free_drift": dict(Nx=64, Ny=48, topo=("periodic", "periodic"), patches=True, random_uv=0.05, ue=0.05, ve=-0.02, top=(0.03, -0.02),
                       free_drift=True),
    "free_drift_coupled": dict(Nx=60, Ny=44, topo=("periodic", "bounded"), patches=True, random_uv=0.03, field_forcing=True,
                               free_drift=True),
    "free_drift_omip": dict(Nx=120, Ny=84, topo=("periodic", "bounded"), patches=True, random_uv=0.03, field_forcing=True,
                            free_drift=True, land=0.25),
    # BetaPlane: f = f0 + beta * y per row (test/test_time_stepping.jl:35); per-row coefficient instantiation of the
    # FAST kernels on a uniform grid (halo rows of a periodic y side carry the wrapped row's f)
    "beta_bounded": dict(Nx=100, Ny=90, topo=("bounded", "bounded"), patches=True, random_uv=0.05, beta=2e-10),
    "beta_channel": dict(Nx=130, Ny=64, topo=("periodic", "bounded"), patches=True, random_uv=0.03, beta=-1.5e-10),
    "beta_latlon": dict(Nx=48, Ny=56, topo=("bounded", "bounded"), grid="latlon", patches=True, random_uv=0.03, beta=1e-6),
    "beta_periodic": dict(Nx=64, Ny=48, topo=("periodic", "periodic"), patches=True, random_uv=0.05, beta=2e-10),
    # orthogonal curvilinear grids (twelve 2-D metric arrays, CSI_METRIC_FULL): reference-order kernels in both modes
    "curvilinear_periodic": dict(Nx=64, Ny=48, topo=("periodic", "periodic"), patches=True, random_uv=0.05, curvilinear=0.05),
    "curvilinear_bounded": dict(Nx=40, Ny=56, topo=("bounded", "bounded"), grid="latlon", patches=True, random_uv=0.05, curvilinear=0.04),
    "curvilinear_masked": dict(Nx=72, Ny=60, topo=("periodic", "bounded"), patches=True, random_uv=0.03, curvilinear=0.05, land=0.25),
    # no-slip walls: ValueBoundaryCondition(0) on the tangential velocity (examples/ice_advected_on_coastline.jl:96-99)
    "noslip_channel": dict(Nx=64, Ny=40, topo=("periodic", "bounded"), patches=True, random_uv=0.05, noslip=True),
    "noslip_bounded": dict(Nx=40, Ny=48, topo=("bounded", "bounded"), grid="latlon", patches=True, random_uv=0.05, noslip=True),
    "noslip_coastline": dict(Nx=72, Ny=48, topo=("periodic", "bounded"), patches=False, random_uv=0.03, noslip=True, land=0.2,
                             field_forcing=True),
    "beta_masked": dict(Nx=96, Ny=80, topo=("periodic", "bounded"), patches=True, random_uv=0.03, beta=2e-10, land=0.25),
    # model.forcing.u / .v given as arrays (user_forcing of sum_of_forcing_u / _v, elasto_visco_plastic_rheology.jl:391-401)
    "user_forcing": dict(Nx=72, Ny=56, topo=("periodic", "periodic"), patches=True, random_uv=0.05, user_forcing=True),
    "user_forcing_latlon": dict(Nx=56, Ny=48, topo=("bounded", "bounded"), grid="latlon", patches=True, random_uv=0.03, user_forcing=True, land=0.2),
    # immersed FluxBoundaryCondition numbers on u and v (ice_stress_divergence.jl:65-123)
    "immersed_flux_bc": dict(Nx=80, Ny=64, topo=("periodic", "bounded"), patches=True, random_uv=0.03, land=0.3,
                             immersed_bc=((0.02, -0.01, 0.015, 0.005), (-0.01, 0.02, 0.01, -0.015))),
    # wind drag: a SemiImplicitStress on TOP (sea_ice_external_stress.jl:162-202), air velocities as numbers / as arrays
    "wind_drag_numbers": dict(Nx=64, Ny=48, topo=("periodic", "bounded"), patches=True, random_uv=0.05, wind_drag="numbers"),
    "wind_drag_arrays": dict(Nx=72, Ny=56, topo=("periodic", "periodic"), patches=True, random_uv=0.05, wind_drag="arrays"),
    "wind_drag_arrays_coupled": dict(Nx=64, Ny=48, topo=("periodic", "bounded"), patches=True, random_uv=0.05, wind_drag="arrays",
                                     field_forcing=True, land=0.2),
    # an explicit bottom stress given as arrays (any (u, v) NamedTuple works in either slot: sea_ice_external_stress.jl:54-61)
    "bottom_stress_arrays": dict(Nx=64, Ny=48, topo=("periodic", "bounded"), patches=True, random_uv=0.05, bottom="arrays", land=0.2),
    # TripolarGrid-like grids: north fold filled by the Zipper boundary condition (u, v change sign; sea_ice_model.jl:57-64)
    "folded_uniform": dict(Nx=64, Ny=48, topo=("periodic", "folded"), patches=True, random_uv=0.05),
    # ... and the reference's own tripolar test configuration (test/distributed_tests_utils.jl:190-212): curvilinear metrics,
    # immersed land, wind-stress / ocean-velocity arrays, StressBalanceFreeDrift
    "folded_tripolar": dict(Nx=60, Ny=44, topo=("periodic", "folded"), patches=True, random_uv=0.03, curvilinear=0.04, land=0.2,
                            field_forcing=True, free_drift=True),
    # per-point Coriolis parameter (2 Omega sin(latitude) of a curvilinear grid): PointwiseCoriolis / csi_coriolis_points_set
    "coriolis_points_curvilinear": dict(Nx=64, Ny=48, topo=("periodic", "bounded"), patches=True, random_uv=0.05, curvilinear=0.05, coriolis_points=True),
    "coriolis_points_tripolar": dict(Nx=60, Ny=44, topo=("periodic", "folded"), patches=True, random_uv=0.03, curvilinear=0.04, land=0.2,
                                     coriolis_points=True),
    "immersed_flux_bc_curvilinear": dict(Nx=64, Ny=48, topo=("periodic", "periodic"), patches=True, random_uv=0.03, land=0.25, curvilinear=0.05,
                                         immersed_bc=((0.02, -0.01, 0.015, 0.005), (-0.01, 0.02, 0.01, -0.015)), user_forcing=True),
}
MASKED = {"curvilinear_periodic", "curvilinear_bounded", "curvilinear_masked", "coriolis_points_curvilinear", "noslip_coastline", "masked_periodic", "masked_channel", "masked_latlon", "field_forcing", "forced_seams", "coupled_channel", "coupled_latlon",
          "beta_masked", "free_drift", "free_drift_coupled", "free_drift_omip",
          # round 3: model.forcing arrays and immersed flux boundary conditions (the EXTRA instantiations of the pair kernel)
          "user_forcing", "user_forcing_latlon", "immersed_flux_bc", "immersed_flux_bc_curvilinear",
          # ... and array-valued wind drag (a SemiImplicitStress on top)
          "wind_drag_arrays", "wind_drag_arrays_coupled", "bottom_stress_arrays"}      # configurations only the pair kernel fuses
THREE_KERNEL_ONLY = {"coriolis_points_tripolar", "folded_uniform", "folded_tripolar"}   # the north fold: never fused at level 1; level 2: three kernels on the rows next to the fold only


def ulp_diff(a, b):
    """largest distance in units in the last place (same-sign finite doubles: difference of the bit patterns)"""
    ia = np.ascontiguousarray(a).view(np.int64)
    ib = np.ascontiguousarray(b).view(np.int64)
    return int(np.abs(ia - ib).max())


DIAG = ("alpha", "zeta_c", "zeta_f", "Delta")


def cmp_region(c, k, a):
    """The part of a parent array every path defines.
    * sigma12 (Face, Face) beyond a wall is never filled nor read: the reference's kernels leave by-products of their
      -H+2 : N+H-1 range there, the two-sub-steps-per-launch kernel leaves them alone -> interior (wall corners included).
    * diagnostics (alpha, zeta, Delta; written on the last sub-step, never read): the reference computes them on
      -H+2 : N+H-1; the two-sub-steps-per-launch kernel writes the interior plus all H periodic images and nothing
      beyond walls -> periodic directions without the outermost layer, bounded directions interior only."""
    Hx, Hy = c.get("Hx", c["H"]), c.get("Hy", c["H"])                              # (make_case takes H as a number or as (Hx, Hy))
    if k == "s12" and ("bounded" in c["topo"] or "folded" in c["topo"]):
        return a[Hy:a.shape[0] - Hy, Hx:a.shape[1] - Hx]
    if k in DIAG:
        cut = [H if t in ("bounded", "folded") else 1 for t, H in zip(c["topo"], (Hx, Hy))]          # (x, y)
        return a[cut[1]:a.shape[0] - cut[1], cut[0]:a.shape[1] - cut[0]]
    return a


def gpu_fields(model):
    model.synchronize()
    return {k: f(model).numpy() for k, f in EVP_FIELDS.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_strict_bitwise_vs_oracle(name, oracle_lib):
    c = cases.make_case(substeps=7, **CASES[name])
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode="strict")
    # state after set! / update_state! must already be identical (halo fill + masks)
    for k in ("u", "v"):
        assert np.array_equal(EVP_FIELDS[k](m).numpy(), p.f[k]), f"{k} after update_state!"
    assert np.array_equal(m.ice_thickness.numpy(), p.f["h"])
    assert np.array_equal(m.ice_concentration.numpy(), p.f["aice"])
    # initialize_rheology!: P uses exp() -> compare in ulps, then continue from the oracle's P
    p.initialize_rheology()
    m.ctx.call("csi_evp_initialize")
    g = gpu_fields(m)
    assert ulp_diff(g["P"], p.f["P"]) <= 4
    assert np.array_equal(g["un"][:, :p.f["un"].shape[1]], p.f["un"]) and np.array_equal(g["vn"], p.f["vn"])
    m.copy_to_field(m.dynamics.auxiliaries.fields.P, p.f["P"])
    # the sub-cycle proper, bit for bit
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    p.subcycle(c["dt"], 1, c["substeps"])
    p.L.ora_finalize_rheology(p.ptr)
    m.ctx.call("csi_evp_subcycle", c["dt"], c["substeps"], 1)
    m.ctx.call("csi_evp_finalize")
    g = gpu_fields(m)
    for k in ("u", "v", "s11", "s22", "s12", "alpha", "zeta_c", "zeta_f", "Delta"):
        assert np.all(np.isfinite(g[k])), k
        assert np.array_equal(g[k], p.f[k]), f"{name}: {k} differs, max abs diff {np.abs(g[k] - p.f[k]).max():.3e}"


# The operand combinations of the strict velocity steps that no case of CASES reaches (there the bottom stress is a SemiImplicitStress
# or a pair of arrays, and a SemiImplicitStress on top always has an air velocity): case keywords, the keywords of the momentum
# equation that replace the case's, and the same stress set on the oracle
STRICT_STRESS_KINDS = {
    "bottom_nothing": (dict(bottom=None), {}, None),
    "bottom_numbers": (dict(bottom=None), dict(bottom_momentum_stress=(0.004, -0.003)), ("bottom", 1, dict(tau=(0.004, -0.003)))),
    "top_semi_at_rest": (dict(top=None), dict(top_momentum_stress=csi.SemiImplicitStress(rho_e=1.3, Cd=1.2e-3)),
                         ("top", 3, dict(rho_e=1.3, Cd=1.2e-3))),
}


@pytest.mark.parametrize("substeps", [3, 4])
@pytest.mark.parametrize("name", list(STRICT_STRESS_KINDS))
def test_strict_bitwise_vs_oracle_remaining_stress_kinds(name, substeps, oracle_lib):
    kw, override, ora = STRICT_STRESS_KINDS[name]
    c = cases.make_case(Nx=12, Ny=10, H=3, substeps=substeps, random_uv=0.05, **kw)
    p = cases.oracle_problem(c)
    if ora is not None:
        p.set_stress(ora[0], ora[1], **ora[2])
    orig = csi.SeaIceMomentumEquation
    csi.SeaIceMomentumEquation = lambda g, **k: orig(g, **dict(k, **override))
    try:
        m = cases.csi_model(c, mode="strict")
    finally:
        csi.SeaIceMomentumEquation = orig
    p.initialize_rheology()
    m.ctx.call("csi_evp_initialize")
    m.copy_to_field(m.dynamics.auxiliaries.fields.P, p.f["P"])      # (P uses exp(): continue from the oracle's, as above)
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    p.subcycle(c["dt"], 1, substeps)
    m.ctx.call("csi_evp_subcycle", c["dt"], substeps, 1)
    g = gpu_fields(m)
    for k in ("u", "v"):                                            # whole parents
        assert np.all(np.isfinite(g[k])) and np.abs(g[k]).max() > 0, k
        assert np.array_equal(g[k], p.f[k]), f"{name}: {k} differs, max abs diff {np.abs(g[k] - p.f[k]).max():.3e}"


FAST_TOL_VEL, FAST_TOL_SIG = 1e-12, 1e-11
_TOL_BRANCH = {}       # case -> {field: "stated" | "10x sensitivity"}: which bound each full-cycle comparison needed


def oracle_self_sensitivity(c, fields=("u", "v", "s11", "s22", "s12")):
    """Conditioning of the EVP iteration on this input: oracle(inputs) vs oracle(inputs * (1 + 1e-15 N(0,1)))."""
    p = cases.oracle_problem(c)
    p.time_step_momentum(c["dt"])
    rng = np.random.default_rng(11)
    c2 = dict(c)
    for k in ("u", "v", "h"):
        c2[k] = c[k] * (1 + 1e-15 * rng.standard_normal(c[k].shape))
    p2 = cases.oracle_problem(c2)
    p2.time_step_momentum(c["dt"])
    return p, {k: np.abs(p2.f[k] - p.f[k]).max() for k in fields}


@pytest.mark.parametrize("name", list(CASES))
def test_fast_vs_oracle_full_cycle(name, oracle_lib):
    """time_step_momentum! with the default 120 sub-steps: FAST kernels against the oracle."""
    c = cases.make_case(substeps=120, **CASES[name])
    p, sens = oracle_self_sensitivity(c)
    m = cases.csi_model(c, mode="fast")
    csi.time_step_momentum(m, c["dt"])
    g = gpu_fields(m)
    vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max())
    smax = max(np.abs(p.f["s11"]).max(), np.abs(p.f["s22"]).max(), np.abs(p.f["s12"]).max())
    well_conditioned = max(sens["u"], sens["v"]) <= 1e-13 * vmax
    branch = {}
    for k in ("u", "v"):
        assert np.all(np.isfinite(g[k]))
        d = np.abs(g[k] - p.f[k]).max()
        assert d <= max(FAST_TOL_VEL * vmax, 10 * sens[k]), (k, d, vmax, sens[k])
        branch[k] = "stated" if d <= FAST_TOL_VEL * vmax else "10x sensitivity"
    for k in ("s11", "s22", "s12"):
        d = np.abs(cmp_region(c, k, g[k]) - cmp_region(c, k, p.f[k])).max()
        assert d <= max(FAST_TOL_SIG * smax, 10 * sens[k]), (k, d, smax, sens[k])
        branch[k] = "stated" if d <= FAST_TOL_SIG * smax else "10x sensitivity"
    _TOL_BRANCH[name] = branch
    # masks / threshold decisions: zero velocity cells (no ice, peripheral nodes) are bit-identical sets
    assert np.array_equal(g["u"] == 0.0, p.f["u"] == 0.0)
    assert np.array_equal(g["v"] == 0.0, p.f["v"] == 0.0)
    if well_conditioned:
        # diagnostics of the last sub-step, where every path defines them (cmp_region)
        ga, pa = cmp_region(c, "alpha", g["alpha"]), cmp_region(c, "alpha", p.f["alpha"])
        # alpha clamp decisions agree (alpha- / alpha+ plateaus are the same cells)
        amin, amax = (c.get("evp", {}).get(k, default) for k, default in (("alpha_min", 50.0), ("alpha_max", 300.0)))     # the case's clamp bounds
        for bound in (amin, amax):
            assert np.array_equal(ga == bound, pa == bound)
        assert np.abs(ga - pa).max() <= 1e-11 * amax
        for k in ("zeta_c", "zeta_f", "Delta"):
            scale = np.abs(p.f[k]).max()
            assert np.abs(cmp_region(c, k, g[k]) - cmp_region(c, k, p.f[k])).max() <= 1e-10 * scale, k


@pytest.mark.parametrize("name", ["periodic_full_ice", "ice_strength_nocoriolis", "latlon_channel", "periodic_patches", "masked_latlon", "curvilinear_bounded"])
def test_fast_two_substeps_from_every_state_of_the_oracle_cycle(name, oracle_lib):
    """What makes the sensitivity branch of the full-cycle test above harmless (round 5): the FAST pair kernel is
    restarted from the ORACLE's state every two sub-steps of the whole 120-sub-step cycle -- u, v, sigma, P, u^n, v^n copied parent for
    parent, halos included -- and advanced by two sub-steps beside it: 60 comparisons per case, each on the TIGHT bound (1e-13 max|u| on
    u, v; 1e-10 max|sigma| on sigma; zero-velocity sets identical).  So the kernel's own error is rounding-level at every state the
    cycle passes through -- the rigid pack where the iteration is chaotic (the first two cases: Delta = Delta_min, gamma > alpha+)
    included; a whole-cycle difference beyond the stated tolerance there is the ITERATION amplifying 1e-16, not the kernel."""
    import torch
    c = cases.make_case(substeps=120, **CASES[name])
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode="fast")
    p.initialize_rheology()
    m.ctx.call("csi_evp_initialize")
    m.synchronize()
    worst = {"u": 0.0, "v": 0.0, "sig": 0.0}
    for s in range(1, 120, 2):
        for k in ("u", "v", "s11", "s22", "s12", "P", "un", "vn"):
            EVP_FIELDS[k](m).data.copy_(torch.from_numpy(np.ascontiguousarray(p.f[k])))
        torch.cuda.synchronize()
        p.subcycle(c["dt"], s, s + 1)
        m.ctx.call("csi_evp_subcycle", float(c["dt"]), 2, s)
        g = gpu_fields(m)
        assert m.ctx.last_path()["level"] == 2, "the two sub-steps did not run through the pair kernel"
        vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max(), 1e-30)
        smax = max(np.abs(p.f["s11"]).max(), np.abs(p.f["s22"]).max(), np.abs(p.f["s12"]).max(), 1e-30)
        for k in ("u", "v"):
            d = np.abs(g[k] - p.f[k]).max()
            assert np.all(np.isfinite(g[k])) and d <= 1e-13 * vmax, (name, "sub-steps", s, s + 1, k, d, vmax)
            assert np.array_equal(g[k] == 0.0, p.f[k] == 0.0), (name, s, k, "zero set")
            worst[k] = max(worst[k], d / vmax)
        for k in ("s11", "s22", "s12"):
            # (owned cells / corners: without finalize_rheology! the oracle's halo layers of sigma are whatever its kernels computed
            #  there -- nothing in the outermost one --, the pair kernel's are images of the interior)
            d = np.abs(EVP_FIELDS[k](m).interior_numpy() - p.interior(k)).max()
            assert d <= 1e-10 * smax, (name, "sub-steps", s, s + 1, k, d, smax)
            worst["sig"] = max(worst["sig"], d / smax)
    print(name, "worst two-sub-step differences along the cycle (relative):", worst)


def test_fast_vs_oracle_tolerance_branch_report():
    """How many of the full-cycle comparisons above needed the loose bound (10 x the oracle's own sensitivity) instead of
    the stated tolerance: printed and written to gpurun_out/fast_tolerance_branches.json.  The rigid-pack cases (a fully
    compact, uniformly moving pack: Delta = Delta_min, gamma > alpha+) are the ones expected there; they are checked tight
    after 1-2 sub-steps below."""
    import json, os
    if not _TOL_BRANCH:
        pytest.skip("the full-cycle tests did not run in this session")
    loose = {n: [k for k, b in br.items() if b != "stated"] for n, br in _TOL_BRANCH.items()}
    loose = {n: v for n, v in loose.items() if v}
    report = {"cases": len(_TOL_BRANCH), "cases_with_a_loose_field": len(loose), "loose": loose}
    print("[fast-vs-oracle]", json.dumps(report))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        json.dump(report, open(os.path.join(out, "fast_tolerance_branches.json"), "w"), indent=1)
    # the seeded inputs of most cases are well conditioned: at least half of them must pass on the stated tolerance alone
    assert len(loose) <= len(_TOL_BRANCH) // 2, report


@pytest.mark.parametrize("name", ["periodic_full_ice", "ice_strength_nocoriolis", "periodic_patches", "latlon_bounded"])
@pytest.mark.parametrize("k", [1, 2])
def test_fast_few_substeps_tight(name, k, oracle_lib):
    """Before the iteration's own chaos can act (1-2 sub-steps) FAST equals the oracle to rounding on every case,
    including the rigid-pack ones."""
    c = cases.make_case(substeps=k, **CASES[name])
    p = cases.oracle_problem(c)
    p.time_step_momentum(c["dt"])
    m = cases.csi_model(c, mode="fast")
    csi.time_step_momentum(m, c["dt"])
    g = gpu_fields(m)
    vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max())
    smax = max(np.abs(p.f["s11"]).max(), np.abs(p.f["s22"]).max(), np.abs(p.f["s12"]).max())
    for f in ("u", "v"):
        assert np.abs(g[f] - p.f[f]).max() <= 1e-13 * vmax
    for f in ("s11", "s22", "s12"):
        assert np.abs(cmp_region(c, f, g[f]) - cmp_region(c, f, p.f[f])).max() <= 1e-10 * smax


def test_strict_full_time_step_momentum_matches_oracle(oracle_lib):
    """Whole time_step_momentum! in STRICT mode, device exp() included: equal to rounding of P."""
    c = cases.make_case(substeps=20, **CASES["periodic_patches"])
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode="strict")
    p.time_step_momentum(c["dt"])
    csi.time_step_momentum(m, c["dt"])
    g = gpu_fields(m)
    vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max())
    assert np.abs(g["u"] - p.f["u"]).max() <= 1e-12 * vmax
    assert np.abs(g["v"] - p.f["v"]).max() <= 1e-12 * vmax


def test_drag_bound_reference_property():
    """test/test_time_stepping.jl:56-80 through the product path (RK3 default timestepper)."""
    g = csi.RectilinearGrid((8, 8), x=(0, 10_000), y=(0, 10_000), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
    uo = 0.1
    dyn = csi.SeaIceMomentumEquation(g, bottom_momentum_stress=csi.SemiImplicitStress(ue=uo),
                                     rheology=csi.ElastoViscoPlasticRheology(), solver=csi.SplitExplicitSolver(substeps=10))
    for mode in ("strict", "fast"):
        model = csi.SeaIceModel(g, dynamics=dyn, mode=mode)
        csi.set_(model, h=1, ℵ=1, u=0, v=0)
        for _ in range(20):
            csi.time_step(model, 60)
        model.synchronize()
        u = model.velocities.u.interior_numpy()
        assert np.all(np.isfinite(u))
        assert u.max() > 0
        assert u.max() <= uo


@pytest.mark.parametrize("N", [2048])
def test_full_size_properties(N):
    """BASELINE size (2048^2 f-plane, periodic): size-independent properties.
    (a) FAST == STRICT to the stated tolerance after 10 sub-steps;
    (b) translation invariance on the periodic uniform grid: shifting the inputs by (sx, sy)
        cells shifts the outputs by the same amount bit for bit (halo / wrap logic at full size);
    (c) everything finite, |u| bounded."""
    kw = dict(Nx=N, Ny=N, topo=("periodic", "periodic"), patches=True, random_uv=0.02, substeps=10)
    c = cases.make_case(**kw)
    out = {}
    for mode in ("strict", "fast"):
        m = cases.csi_model(c, mode=mode)
        csi.time_step_momentum(m, c["dt"])
        m.synchronize()
        out[mode] = {k: EVP_FIELDS[k](m).interior_numpy().copy() for k in ("u", "v", "s11", "s22", "s12")}
        del m
    vmax = max(np.abs(out["strict"]["u"]).max(), np.abs(out["strict"]["v"]).max())
    smax = np.abs(out["strict"]["s11"]).max()
    for k in ("u", "v"):
        assert np.all(np.isfinite(out["fast"][k]))
        assert np.abs(out["fast"][k] - out["strict"][k]).max() <= FAST_TOL_VEL * vmax
    for k in ("s11", "s22", "s12"):
        assert np.abs(out["fast"][k] - out["strict"][k]).max() <= FAST_TOL_SIG * smax
    assert vmax < 10.0
    sx, sy = 517, 1031
    c2 = dict(c)
    for k in ("h", "a", "u", "v"):
        c2[k] = np.roll(c[k], (sy, sx), axis=(0, 1))
    m = cases.csi_model(c2, mode="fast")
    csi.time_step_momentum(m, c["dt"])
    m.synchronize()
    for k in ("u", "v", "s11", "s22", "s12"):
        got = EVP_FIELDS[k](m).interior_numpy()
        assert np.array_equal(got, np.roll(out["fast"][k], (sy, sx), axis=(0, 1))), k


@pytest.mark.parametrize("k", [1, 2, 0])
@pytest.mark.parametrize("fc", [(True, True), (True, False), (False, True)], ids=["xy", "x", "y"])
@pytest.mark.parametrize("mode", ["strict", "fast", "fused"])
def test_rccl_self_exchange_bitwise(mode, fc, k):
    """The multi-GPU path on one GPU: a periodic domain whose tile edges are CONNECTED to itself, so every halo
    comes through pack -> ncclSend/ncclRecv (to self) -> unpack and the ring recomputation of SURVEY.md A.5.
    Owned cells must equal the plain periodic run bit for bit (same kernels, same arithmetic)."""
    # "fast": field-valued forcing -> three-kernel path; "fused": numeric forcing -> fused sub-step kernel on the tile
    fused = mode == "fused"
    c = cases.make_case(Nx=96, Ny=64, substeps=13, topo=("periodic", "periodic"), patches=True, random_uv=0.05,
                        field_forcing=(mode == "fast"))
    mode = "fast" if fused else mode
    ref = cases.csi_model(c, mode=mode)
    ref.set_fusion(False)
    csi.time_step_momentum(ref, c["dt"])
    til = cases.csi_model(c, mode=mode, tile=(1, 1, 0, fc))
    til.set_halo_transport("rccl")
    til.set_exchange_interval(k)        # k sub-steps per exchange of width 2k (0: automatic = 2 with halo 4)
    csi.time_step_momentum(til, c["dt"])
    ref.synchronize(); til.synchronize()
    # numeric forcing: fused kernels (pairs inside an even exchange batch); array-valued forcing: only the
    # two-sub-steps-per-launch kernel takes it, so k = 1 runs the three kernels
    level = til.ctx.last_path()["level"]
    if mode == "strict":
        assert level == 0
    else:
        assert level == ((2 if k != 1 else 1) if fused else (2 if k != 1 else 0))
    assert til.ctx.launches_per_substep() == (1 if level else (3 if mode == "fast" else 4)) + (3 if k == 1 else 0)
    for k in ("u", "v", "s11", "s22", "s12", "alpha"):
        a, b = EVP_FIELDS[k](ref).interior_numpy(), EVP_FIELDS[k](til).interior_numpy()
        assert np.array_equal(a, b), (k, np.abs(a - b).max())
    # and the exchanged halos (width 2) carry the neighbour's owned values
    u_ref, u_til = ref.velocities.u.numpy(), til.velocities.u.numpy()
    H = c["g"].Hx
    assert np.array_equal(u_ref[H - 2:-(H - 2), H - 2:-(H - 2)], u_til[H - 2:-(H - 2), H - 2:-(H - 2)])


@pytest.mark.parametrize("nsub", [12, 15])
@pytest.mark.parametrize("k", [4, 2, 3, 0])
@pytest.mark.parametrize("fc", [(True, True), (True, False), (False, True)], ids=["xy", "x", "y"])
def test_pair_kernel_on_tiles_halo8(fc, k, nsub):
    """Two sub-steps per launch on a self-connected tile with halo 8: exchange of width 2k every k sub-steps, the
    pairs sit at batch positions (0,1), (2,3); k = 3 is odd, so the library must fall back to one sub-step per
    launch.  Mixed sides ("x": connected in x, periodic in y) combine exchange and halo images.  Owned cells equal
    the untiled three-kernel run bit for bit."""
    c = cases.make_case(Nx=120, Ny=72, H=8, substeps=nsub, topo=("periodic", "periodic"), patches=True, random_uv=0.05)
    ref = cases.csi_model(c, mode="fast")
    ref.set_fusion(0)
    csi.time_step_momentum(ref, c["dt"])
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, fc))
    til.set_halo_transport("rccl")
    til.set_exchange_interval(k)
    csi.time_step_momentum(til, c["dt"])
    ref.synchronize(); til.synchronize()
    path = til.ctx.last_path()
    kk = k or 4                     # automatic: min(halo / 2, 8) = 4 with halo 8
    assert path["exchange_interval"] == kk and path["level"] == (2 if kk % 2 == 0 else 1), path
    for f in ("u", "v", "s11", "s22", "s12", "alpha", "zeta_c", "zeta_f", "Delta"):
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])


@pytest.mark.parametrize("k", [1, 2])
def test_user_forcing_arrays_on_tiles_bitwise(k):
    """model.forcing.u / .v as arrays on a self-connected tile: inside an exchange batch the velocity kernels read the forcing
    on ranges that extend into the halo, so its halos beyond connected sides must come through the exchange (they held zeros:
    ADVICE round 2).  Owned cells equal the untiled run bit for bit."""
    c = cases.make_case(Nx=96, Ny=64, substeps=10, topo=("periodic", "periodic"), patches=True, random_uv=0.05, user_forcing=True)
    ref = cases.csi_model(c, mode="fast")
    ref.set_fusion(0)
    csi.time_step_momentum(ref, c["dt"])
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, (True, True)))
    til.set_exchange_interval(k)
    csi.time_step_momentum(til, c["dt"])
    ref.synchronize(); til.synchronize()
    assert til.ctx.last_path()["exchange_interval"] == k
    for f in ("u", "v", "s11", "s22", "s12", "alpha"):
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])


@pytest.mark.parametrize("k", [4, 2])
def test_pair_kernel_on_channel_tile(k):
    """A tile with two kinds of edges: x connected (to itself), y walls.  Exchange in x, mirror images and in-register
    wall conditions in y; owned cells equal the untiled three-kernel run bit for bit."""
    c = cases.make_case(Nx=120, Ny=72, H=8, substeps=14, topo=("periodic", "bounded"), patches=True, random_uv=0.05)
    ref = cases.csi_model(c, mode="fast")
    ref.set_fusion(0)
    csi.time_step_momentum(ref, c["dt"])
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, (True, False)))
    til.set_exchange_interval(k)
    csi.time_step_momentum(til, c["dt"])
    ref.synchronize(); til.synchronize()
    path = til.ctx.last_path()
    assert path["exchange_interval"] == k and path["level"] == 2, path
    for f in ("u", "v", "s11", "s22", "s12", "alpha", "zeta_c", "zeta_f", "Delta"):
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])


def test_pair_kernel_on_tiles_halo16_auto_interval():
    """bench.py's tile configuration: halo 16, automatic exchange interval (8): four pairs per batch with shrinking
    valid widths 16/14, 12/10, 8/6, 4/2; 20 sub-steps = 2 full batches + half a batch."""
    c = cases.make_case(Nx=130, Ny=96, H=16, substeps=20, topo=("periodic", "periodic"), patches=True, random_uv=0.05)
    ref = cases.csi_model(c, mode="fast")
    ref.set_fusion(0)
    csi.time_step_momentum(ref, c["dt"])
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, (True, True)))
    til.set_halo_transport("rccl")
    csi.time_step_momentum(til, c["dt"])
    ref.synchronize(); til.synchronize()
    path = til.ctx.last_path()
    assert path["exchange_interval"] == 8 and path["level"] == 2 and path["exchanges"] == 3, path
    for f in ("u", "v", "s11", "s22", "s12", "alpha", "zeta_c", "zeta_f", "Delta"):
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])


@pytest.mark.parametrize("topo", [("periodic", "periodic"), ("periodic", "bounded")])
def test_pair_kernel_on_tiles_halo32_interval16(topo):
    """The widest batch: halo 32, automatic exchange interval 16 (eight pairs per batch, valid widths 32 .. 2);
    40 sub-steps = 2 full batches + half a batch; with walls in y and an immersed mask too."""
    c = cases.make_case(Nx=150, Ny=128, H=32, substeps=40, topo=topo, patches=True, random_uv=0.05,
                        land=0.2 if topo[1] == "bounded" else 0.0)
    ref = cases.csi_model(c, mode="fast")
    ref.set_fusion(0)
    csi.time_step_momentum(ref, c["dt"])
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, (True, topo[1] == "periodic")))
    til.set_halo_transport("rccl")
    csi.time_step_momentum(til, c["dt"])
    ref.synchronize(); til.synchronize()
    path = til.ctx.last_path()
    assert path["exchange_interval"] == 16 and path["level"] == 2 and path["exchanges"] == 3, path
    for f in ("u", "v", "s11", "s22", "s12", "alpha"):
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])


PEER_CASES = {
    # (make_case keywords, which periodic directions are connected to the tile itself)
    "periodic_xy": (dict(Nx=300, Ny=200, topo=("periodic", "periodic")), (True, True)),
    "periodic_x": (dict(Nx=300, Ny=200, topo=("periodic", "periodic")), (True, False)),
    "periodic_y": (dict(Nx=130, Ny=96, topo=("periodic", "periodic")), (False, True)),
    "small_halo6": (dict(Nx=128, Ny=48, H=6, topo=("periodic", "periodic")), (True, True)),
    "channel_land": (dict(Nx=300, Ny=200, topo=("periodic", "bounded"), land=0.2), (True, False)),
    "channel_noslip": (dict(Nx=180, Ny=120, topo=("periodic", "bounded"), noslip=True), (True, False)),
    "latlon_channel": (dict(Nx=150, Ny=128, topo=("periodic", "bounded"), grid="latlon"), (True, False)),
    "coupled_arrays": (dict(Nx=200, Ny=150, topo=("periodic", "periodic"), field_forcing=True), (True, True)),
    "free_drift_land": (dict(Nx=160, Ny=120, topo=("periodic", "bounded"), field_forcing=True, free_drift=True, land=0.25), (True, False)),
    "curvilinear": (dict(Nx=136, Ny=96, topo=("periodic", "bounded"), curvilinear=0.04), (True, False)),
    "beta_periodic_x": (dict(Nx=140, Ny=100, topo=("periodic", "bounded"), beta=2e-10), (True, False)),
    "wind_drag_arrays": (dict(Nx=160, Ny=96, topo=("periodic", "periodic"), wind_drag="arrays", field_forcing=True), (True, True)),
}


@pytest.mark.parametrize("nsub", [1, 2, 7, 12, 120])
@pytest.mark.parametrize("name", sorted(PEER_CASES))
def test_peer_halo_transport_self_connected_bitwise(name, nsub):
    """csi_set_halo_transport(PEER), the default on tiles: a connected side behaves like a periodic one whose halo lives in the
    neighbour's arrays -- the owners' stores write the images there, per-tile flags order the launches (evp_fused2.hip).  Here
    the neighbour is the tile itself (one GPU): same kernels, same flag protocol, every slot index exercised.  The whole parent
    arrays -- halos included -- of u, v, sigma equal the untiled run bit for bit, and so do the interiors of alpha, zeta, Delta
    against the three-kernel path; one RCCL exchange per sub-cycle remains.  An odd count ends with one launch of the same
    kernel in its single-sub-step mode (the untiled run's trailing launch may be another kernel, which leaves other by-products
    in never-read halo layers: interiors are compared then)."""
    kw, fc = PEER_CASES[name]
    c = cases.make_case(substeps=nsub, patches=True, random_uv=0.05, **kw)
    three = cases.csi_model(c, mode="fast")
    three.set_fusion(0)
    csi.time_step_momentum(three, c["dt"])
    ref = cases.csi_model(c, mode="fast")
    csi.time_step_momentum(ref, c["dt"])
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, fc))
    csi.time_step_momentum(til, c["dt"])
    csi.time_step_momentum(til, c["dt"])       # a second sub-cycle: the launch numbers carry on
    csi.time_step_momentum(ref, c["dt"])
    csi.time_step_momentum(three, c["dt"])
    three.synchronize(); ref.synchronize(); til.synchronize()
    path = til.ctx.last_path()
    assert til.ctx.halo_transport() == "peer" and path["exchanges"] == 1, path
    assert til.ctx.last_launches() == ((nsub + 1) // 2, nsub)
    assert path["level"] == (2 if nsub >= 2 else 1)
    assert nsub < 2 or ref.ctx.last_path()["level"] == 2      # (one sub-step with masks / array forcing, untiled: three kernels)
    for f in ("u", "v", "s11", "s22", "s12"):
        get = (lambda m: EVP_FIELDS[f](m).numpy()) if nsub % 2 == 0 else (lambda m: EVP_FIELDS[f](m).interior_numpy())
        a, b = get(ref), get(til)
        assert np.array_equal(a, b), (f, "parents incl. halos", np.abs(a - b).max(), np.argwhere(a != b)[:5])
    for f in ("u", "v", "s11", "s22", "s12", "alpha", "zeta_c", "zeta_f", "Delta"):
        a, b = EVP_FIELDS[f](three).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])


@pytest.mark.parametrize("tier", [1, 2])
@pytest.mark.parametrize("name", ["periodic_xy", "channel_land", "coupled_arrays"])
def test_peer_protocol_tiers_bitwise(name, tier):
    """csi_set_peer_tier: the run-time ladder of the peer transport's memory ordering (1: + a system-scope acquire fence once the
    flags have been seen; 2: + a system-scope release fence before the flags are published).  Every tier gives the untiled run's
    answer bit for bit -- the tiers differ in what they assume of the memory system between two devices, not in the result."""
    kw, fc = PEER_CASES[name]
    c = cases.make_case(substeps=13, patches=True, random_uv=0.05, **kw)
    ref = cases.csi_model(c, mode="fast")
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, fc))
    assert til.ctx.peer_tier() == 0
    til.set_peer_tier(tier)
    for _ in range(2):
        csi.time_step_momentum(ref, c["dt"])
        csi.time_step_momentum(til, c["dt"])
    ref.synchronize(); til.synchronize()
    assert til.ctx.halo_transport() == "peer" and til.ctx.peer_tier() == tier
    for f in ("u", "v", "s11", "s22", "s12"):
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (f, tier, np.abs(a - b).max())
    with pytest.raises(csi.CsiError):
        til.set_peer_tier(3)


def test_peer_abort_is_sticky_until_rearmed():
    """A wait of the flag protocol that gave up (simulated: csi_debug_peer_abort leaves the pinned error word the way the kernel's
    time-out does) makes EVERY later entry point fail with CSI_ERR_COMM -- not only the next one: the flags cannot recover by
    themselves -- until the caller re-arms the transport (csi_set_halo_transport, on all ranks); the next sub-cycle
    then runs the collective set-up again and the tile reproduces the untiled run bit for bit."""
    kw, fc = PEER_CASES["periodic_xy"]
    c = cases.make_case(substeps=12, patches=True, random_uv=0.05, **kw)
    ref = cases.csi_model(c, mode="fast")
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, fc))
    csi.time_step_momentum(ref, c["dt"]); csi.time_step_momentum(til, c["dt"])
    til.synchronize()
    assert til.ctx.halo_transport() == "peer"
    til.ctx.call("csi_debug_peer_abort")
    for _ in range(3):                                    # sticky: every call, not only the first
        with pytest.raises(csi.CsiError) as e:
            csi.time_step_momentum(til, c["dt"])
        assert "peer halo transport" in str(e.value)
    with pytest.raises(csi.CsiError):
        til.synchronize()
    with pytest.raises(csi.CsiError):
        til.ctx.validate_all()
    til.set_halo_transport("peer")                        # re-armed (on a real node: by every rank)
    csi.time_step_momentum(ref, c["dt"]); csi.time_step_momentum(til, c["dt"])
    ref.synchronize(); til.synchronize()
    assert til.ctx.halo_transport() == "peer"
    for f in ("u", "v", "s11", "s22", "s12"):
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), (f, np.abs(a - b).max())
    til.ctx.call("csi_debug_peer_abort")                  # ... and the message exchange is the other way out
    with pytest.raises(csi.CsiError):
        csi.time_step_momentum(til, c["dt"])
    til.set_halo_transport("rccl")
    csi.time_step_momentum(ref, c["dt"]); csi.time_step_momentum(til, c["dt"])
    ref.synchronize(); til.synchronize()
    assert til.ctx.halo_transport() == "rccl"
    for f in ("u", "v", "s11", "s22", "s12"):
        assert np.array_equal(EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()), f


def test_peer_abort_throws_before_output_is_read():
    """a step that ended on an aborted sub-cycle must not hand its fields to an output writer or a checkpointer.
    time_step (its once-per-step collective check) and prognostic_state (the checkpoint path) both raise; nothing is returned."""
    kw, fc = PEER_CASES["periodic_xy"]
    c = cases.make_case(substeps=12, patches=True, random_uv=0.05, **kw)
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, fc), timestepper="ForwardEuler")
    csi.time_step(til, c["dt"])
    assert til.ctx.halo_transport() == "peer"
    til.ctx.call("csi_debug_peer_abort")
    with pytest.raises(csi.CsiError):
        csi.prognostic_state(til)
    it = til.clock.iteration
    with pytest.raises(csi.CsiError):
        csi.time_step(til, c["dt"])
    assert til.clock.iteration == it                      # the failed step did not count
    til.set_halo_transport("peer")
    csi.time_step(til, c["dt"])
    assert til.clock.iteration == it + 1 and "u" in csi.prognostic_state(til)


def test_peer_halo_transport_falls_back_and_can_be_switched_off():
    """Explicit exchange intervals run the RCCL exchange; csi_set_halo_transport(RCCL) switches the peer transport off; odd
    sub-step counts stay on it; all bit-identical."""
    c = cases.make_case(Nx=136, Ny=72, H=8, substeps=13, topo=("periodic", "periodic"), patches=True, random_uv=0.05)
    ref = cases.csi_model(c, mode="fast")
    ref.set_fusion(0)
    csi.time_step_momentum(ref, c["dt"])
    ref.synchronize()
    want = {f: EVP_FIELDS[f](ref).interior_numpy().copy() for f in ("u", "v", "s11", "s22", "s12")}
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, (True, True)))
    csi.time_step_momentum(til, c["dt"])                      # 13 sub-steps: odd
    til.synchronize()
    assert til.ctx.halo_transport() == "peer"
    for f in want:
        assert np.array_equal(want[f], EVP_FIELDS[f](til).interior_numpy()), f
    c2 = dict(c, substeps=12)
    ref2 = cases.csi_model(c2, mode="fast"); ref2.set_fusion(0)
    csi.time_step_momentum(ref2, c2["dt"]); ref2.synchronize()
    for setup, expect in ((lambda m: None, "peer"), (lambda m: m.set_halo_transport("rccl"), "rccl"), (lambda m: m.set_exchange_interval(2), "rccl")):
        til = cases.csi_model(c2, mode="fast", tile=(1, 1, 0, (True, True)))
        setup(til)
        csi.time_step_momentum(til, c2["dt"])
        til.synchronize()
        assert til.ctx.halo_transport() == expect
        for f in want:
            assert np.array_equal(EVP_FIELDS[f](ref2).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()), (expect, f)


EXTRA_CASES = ["folded_uniform", "folded_tripolar", "coriolis_points_tripolar", "user_forcing", "user_forcing_latlon", "immersed_flux_bc", "immersed_flux_bc_curvilinear"]
FUSED_CASES = EXTRA_CASES + ["periodic_patches", "periodic_full_ice", "bounded", "channel", "latlon_bounded", "latlon_channel",
               "ice_strength_nocoriolis", "ragged", "periodic_seams", "periodic_halo6", "bounded_seams",
               "beta_bounded", "beta_channel", "beta_latlon", "beta_periodic", "noslip_channel", "noslip_bounded", "wind_drag_numbers",
               ] + sorted(MASKED)
PAIR_CASES = {"periodic_patches", "periodic_full_ice", "ice_strength_nocoriolis", "periodic_seams", "periodic_halo6",
              "bounded", "channel", "latlon_bounded", "latlon_channel", "bounded_seams",
              "beta_bounded", "beta_channel", "beta_latlon", "beta_periodic", "noslip_channel", "noslip_bounded", "wind_drag_numbers"} | MASKED


@pytest.mark.parametrize("nsub", [1, 2, 7, 120])
@pytest.mark.parametrize("name", FUSED_CASES)
def test_fused_kernels_bitwise_equal_three_kernel_path(name, nsub):
    """csrc/evp_fused.hip (one launch per sub-step, per-wave ring recomputation, double-buffered u, v, sigma) and
    csrc/evp_fused2.hip (two sub-steps per launch, the first one's results kept in registers) must reproduce the
    three-kernel FAST path bit for bit: same arithmetic (evp_fast_math.h), different schedule.  Level 1 is
    compared on every field, halos included.  Level 2 leaves the halo cells of the diagnostics (alpha, zeta,
    Delta: written on the last sub-step only, never read) to the second sub-step's range, so those are compared
    on the interior; so is sigma12 next to walls (its cells beyond a wall are never filled nor read; the
    three-kernel path leaves by-products of its -H+2 : N+H-1 range there).  Odd sub-step counts exercise the
    trailing single sub-step and the ping-pong copy-back."""
    c = cases.make_case(substeps=nsub, **CASES[name])
    out, level = {}, {}
    for fusion in (0, 1, 2):
        m = cases.csi_model(c, mode="fast")
        m.set_fusion(fusion)
        csi.time_step_momentum(m, c["dt"])
        m.synchronize()
        level[fusion] = m.ctx.last_path()["level"]
        assert m.ctx.launches_per_substep() == (1 if level[fusion] else 3)
        diag = (lambda f: f.numpy()) if fusion < 2 else (lambda f: f.interior_numpy())
        walls = "bounded" in CASES[name]["topo"] or "folded" in CASES[name]["topo"]      # (a RightFolded y has a wall in the south)
        out[fusion] = {k: EVP_FIELDS[k](m).numpy().copy() for k in ("u", "v", "s11", "s22") + (() if walls else ("s12",))}
        out[fusion].update({k: (EVP_FIELDS[k](m).numpy().copy(), EVP_FIELDS[k](m).interior_numpy().copy())
                            for k in ("alpha", "zeta_c", "zeta_f", "Delta") + (("s12",) if walls else ())})
    single = 0 if (name in MASKED or name in THREE_KERNEL_ONLY) else 1   # the one-sub-step kernel takes neither masks nor array-valued forcing
    assert level[0] == 0 and level[1] == single
    # (round 3: a north fold runs the pair kernel below a band of three-kernel rows next to the fold, csi_abi.hip FoldBand)
    assert level[2] == (2 if ((name in PAIR_CASES or name in THREE_KERNEL_ONLY) and nsub >= 2) else single), level
    if level[2] == 2 and name not in THREE_KERNEL_ONLY:
        launches, substeps = m.ctx.last_launches()
        assert substeps == nsub and launches == (nsub + 1) // 2        # (round 3: the odd trailing sub-step of masked / array-forced configurations is ONE launch too)
    for fusion in (1, 2):
        for k in out[0]:
            a, b = out[0][k], out[fusion][k]
            if isinstance(a, tuple):
                a, b = (a[1], b[1]) if level[fusion] == 2 else (a[0], b[0])
            assert np.all(np.isfinite(b)), k
            assert np.array_equal(a, b), (name, nsub, fusion, k, np.abs(a - b).max(), np.argwhere(a != b)[:5])


@pytest.mark.parametrize("k", [1, 2])
def test_masked_tile_self_exchange_bitwise(k):
    """Immersed mask + tile edges: the tile's mask (halo included) is sliced from the global one; owned cells equal
    the untiled masked three-kernel run bit for bit (k = 1: three-kernel path on the tile; k = 2: two sub-steps per
    launch with the mask)."""
    c = cases.make_case(Nx=64, Ny=48, substeps=10, topo=("periodic", "periodic"), patches=True, random_uv=0.03, land=0.3)
    ref = cases.csi_model(c, mode="fast")
    ref.set_fusion(0)
    csi.time_step_momentum(ref, c["dt"])
    til = cases.csi_model(c, mode="fast", tile=(1, 1, 0, True))
    til.set_exchange_interval(k)
    csi.time_step_momentum(til, c["dt"])
    ref.synchronize(); til.synchronize()
    assert til.ctx.last_path()["level"] == (2 if k == 2 else 0)
    for f in ("u", "v", "s11", "s22", "s12"):
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](til).interior_numpy()
        assert np.array_equal(a, b), f


def fuzz_config(seed):
    """(make_case keywords, sub-step count) of one fuzz seed (also drawn from by tests/test_gpu_pair_ufirst.py, on seeds of its own)"""
    rng = np.random.default_rng(1000 + seed)
    topo = (("periodic", "bounded")[rng.integers(2)], ("periodic", "bounded")[rng.integers(2)])
    H = int(rng.integers(4, 9))
    Nx = int(rng.integers(2 * H, 200)); Ny = int(rng.integers(2 * H, 90))
    kw = dict(Nx=Nx, Ny=Ny, H=H, topo=topo, patches=bool(rng.integers(2)), random_uv=0.04,
              grid=("rectilinear", "latlon")[rng.integers(2)] if topo[1] == "bounded" else "rectilinear",
              field_forcing=bool(rng.integers(2)), land=(0.0, 0.25)[rng.integers(2)],
              coriolis=(1e-4, None)[rng.integers(2)], pressure=("replacement", "ice_strength")[rng.integers(2)])
    if "bounded" in topo and rng.integers(3) == 0:
        kw["noslip"] = True
    if rng.integers(4) == 0:
        kw["free_drift"] = True
        if not kw["field_forcing"]:
            kw.update(ue=0.05, ve=-0.02, top=(0.03, -0.02))
    if kw["coriolis"] is not None and topo[1] == "bounded" and rng.integers(3) == 0:
        kw["beta"] = 2e-10 if kw["grid"] == "rectilinear" else 1e-6
    nsub = int(rng.integers(2, 12))
    if seed >= 20000:            # (round 3; earlier seeds keep their configurations) model.forcing arrays, immersed flux boundary conditions
        if rng.integers(4) == 0:
            kw["user_forcing"] = True
        if kw["land"] and rng.integers(4) == 0:
            kw["immersed_bc"] = ((0.02, -0.01, 0.015, 0.005), (-0.01, 0.02, 0.01, -0.015))
        if kw.get("user_forcing") or kw.get("immersed_bc"):
            kw.pop("free_drift", None)
    if seed >= 40000:            # (later in round 3) wind drag (a SemiImplicitStress on top) and explicit bottom-stress arrays
        r = rng.integers(6)
        if r < 2:
            kw["wind_drag"] = ("numbers", "arrays")[r]
            kw.pop("free_drift", None)          # (StressBalanceFreeDrift takes exactly one SemiImplicitStress)
        elif r == 2 and not kw["field_forcing"]:
            kw["bottom"] = "arrays"
            kw.pop("free_drift", None)
    return kw, nsub


def fuzz_unfused(kw):
    """no instantiation of the two-sub-steps kernel takes both families of arrays: such a configuration runs the three kernels"""
    return bool((kw.get("wind_drag") == "arrays" or kw.get("bottom") == "arrays") and (kw.get("free_drift") or kw.get("user_forcing") or kw.get("immersed_bc")))


@pytest.mark.parametrize("seed", range(24))
def test_fused_paths_fuzz_bitwise(seed):
    """Randomised geometry / topology / halo / sub-step count / forcing / mask: the fused paths (whatever the library
    picks at level 2) equal the three-kernel path bit for bit on u, v, sigma (interior of sigma12 next to walls)."""
    kw, nsub = fuzz_config(seed)
    c = cases.make_case(substeps=nsub, **kw)
    out = {}
    lvl = {}
    for fusion in (0, 2):
        m = cases.csi_model(c, mode="fast")
        m.set_fusion(fusion)
        csi.time_step_momentum(m, c["dt"])
        m.synchronize()
        out[fusion] = {k: cmp_region(c, k, EVP_FIELDS[k](m).numpy()).copy() for k in ("u", "v", "s11", "s22", "s12")}
        out[fusion]["alpha"] = EVP_FIELDS["alpha"](m).interior_numpy().copy()
        lvl[fusion] = m.ctx.last_path()["level"]
    assert (lvl[2] == 0) if fuzz_unfused(kw) else (lvl[2] == 2), (kw, nsub, lvl)   # (no instantiation with both families of arrays)
    for fusion in (2,):
        for k in out[0]:
            a, b = out[0][k], out[fusion][k]
            assert np.all(np.isfinite(b)), (k, kw)
            assert np.array_equal(a, b), (seed, fusion, kw, nsub, k, np.abs(a - b).max(), np.argwhere(a != b)[:4])


FOLD_BAND_CASES = {
    "uniform": dict(Nx=64, Ny=48),
    "uniform_halo7_ragged": dict(Nx=117, Ny=61, H=7),
    "one_chunk_below_the_band": dict(Nx=200, Ny=24),
    "tripolar_coupled": dict(Nx=120, Ny=70, curvilinear=0.04, land=0.2, field_forcing=True, free_drift=True),
    "tripolar_coriolis_points": dict(Nx=90, Ny=64, H=5, curvilinear=0.04, land=0.25, coriolis_points=True),
    "tripolar_user_forcing": dict(Nx=72, Ny=56, curvilinear=0.04, land=0.2, user_forcing=True,
                                  immersed_bc=((0.02, -0.01, 0.015, 0.005), (-0.01, 0.02, 0.01, -0.015))),
    "coupled_arrays": dict(Nx=128, Ny=80, field_forcing=True),
    "masked_noslip": dict(Nx=100, Ny=52, land=0.3, noslip=True),
}


@pytest.mark.parametrize("nsub", [2, 5, 120])
@pytest.mark.parametrize("name", sorted(FOLD_BAND_CASES))
def test_north_fold_band_bitwise(name, nsub):
    """A north fold (TripolarGrid: RightFolded y) at fusion level 2: rows 1 .. Ny - Hy - 4 through the two-sub-steps kernel, the rows
    next to the fold through the three kernels (which read and store fold images like the reference's), csi_abi.hip FoldBand.
    Everything -- the parents of u, v, sigma where anything reads them, the diagnostics' interiors -- equals the three-kernel run
    of the whole grid bit for bit, for two sub-cycles in a row."""
    kw = dict(topo=("periodic", "folded"), patches=True, random_uv=0.04)
    kw.update(FOLD_BAND_CASES[name])
    c = cases.make_case(substeps=nsub, **kw)
    ref = cases.csi_model(c, mode="fast"); ref.set_fusion(0)
    new = cases.csi_model(c, mode="fast")
    for _ in range(2):
        csi.time_step_momentum(ref, c["dt"]); csi.time_step_momentum(new, c["dt"])
    ref.synchronize(); new.synchronize()
    assert ref.ctx.last_path()["level"] == 0 and new.ctx.last_path()["level"] == 2
    for f in ("u", "v", "s11", "s22", "s12"):
        a, b = cmp_region(c, f, EVP_FIELDS[f](ref).numpy()), cmp_region(c, f, EVP_FIELDS[f](new).numpy())
        assert np.all(np.isfinite(b)), f
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])
    for f in ("alpha", "zeta_c", "zeta_f", "Delta"):
        a, b = EVP_FIELDS[f](ref).interior_numpy(), EVP_FIELDS[f](new).interior_numpy()
        assert np.array_equal(a, b), (f, np.abs(a - b).max(), np.argwhere(a != b)[:5])


@pytest.mark.parametrize("topo", [("periodic", "periodic"), ("bounded", "bounded"), ("periodic", "bounded")])
@pytest.mark.parametrize("Nx,Ny,H", [(8, 8, 4), (9, 7, 3), (5, 5, 4), (4, 9, 4), (3, 3, 2), (64, 8, 4), (8, 64, 4), (57, 9, 4), (113, 10, 5)])
def test_degenerate_grid_sizes_every_path(Nx, Ny, H, topo, oracle_lib):
    """Grids of a few cells, N = H, N = 2H, one strip / one chunk, ragged widths: STRICT bit for bit and FAST (three kernels,
    one sub-step per launch, two sub-steps per launch -- each falls back where its geometry needs more cells) against the
    oracle.  (scripts/tiny_grids.py also checks that halo < 2 and N < H fail loudly.)"""
    c = cases.make_case(Nx=Nx, Ny=Ny, H=H, topo=topo, substeps=6, patches=False, random_uv=0.02)
    p = cases.oracle_problem(c)
    p.time_step_momentum(c["dt"])
    vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max())
    for mode, fusion in (("strict", 0), ("fast", 0), ("fast", 1), ("fast", 2)):
        m = cases.csi_model(c, mode=mode)
        m.set_fusion(fusion)
        csi.time_step_momentum(m, c["dt"])
        g = gpu_fields(m)
        for k in ("u", "v"):
            assert np.all(np.isfinite(g[k]))
            d = np.abs(g[k] - p.f[k]).max()
            assert (d == 0.0) if mode == "strict" else (d <= 1e-11 * vmax), (mode, fusion, k, d, vmax)


def test_invalid_grids_fail_loudly():
    for (Nx, Ny, H, topo) in [(2, 2, 1, ("periodic", "periodic")), (1, 6, 2, ("bounded", "bounded")), (6, 1, 2, ("periodic", "bounded"))]:
        c = cases.make_case(Nx=Nx, Ny=Ny, H=H, topo=topo, substeps=2, patches=False)
        with pytest.raises(csi.CsiError):
            m = cases.csi_model(c, mode="fast")
            csi.time_step_momentum(m, c["dt"])
