"""Unequal halo widths (Hx != Hy) against the oracle and across the kernel families.

Every other GPU test builds its grids with halo = (H, H), so an Hx / Hy swap in an origin, an image test, a ring offset or a launch
geometry is invisible to them.  Here the same comparisons run with halos (5, 3) and (3, 5) -- (6, 4) and (4, 6) where WENO7 needs four
layers in both directions -- on grids of about 40 x 28 and 28 x 40 cells, so that a transposed stride cannot cancel out:

  * csi_time_step_momentum in STRICT against oracle.Problem(Nx, Ny, Hx, Hy, ...), BIT FOR BIT on whole parents of u, v, sigma, alpha,
    zeta, Delta: periodic, walls, a masked channel, a latitude-longitude grid (per-row metrics), a curvilinear grid with the north fold.
    The ice is compact (aice = 1 on every wet cell, 0 on land), so the ice strength P = P* h exp(-C (1 - aice)) needs exp() at 0 only
    and the device's libm and glibc cannot differ in it: the whole entry point is comparable bit for bit, P included.
  * FAST within the stated 1e-12 of max|u| of STRICT with equal zero-velocity sets, and FAST at fusion levels 0, 1, 2 bit-identical to
    each other on the regions every path defines (tests/test_gpu_evp.py cmp_region, which takes the halo pair), with the kernel family csi_last_path reports
    asserted for every run.  These cases have patches of open water and thin ice (both sides run on the device).
  * one SplitRungeKutta3 step with WENO7 and one ForwardEuler step with slab thermodynamics in STRICT against the oracle, bit for bit
    on h, aice, u, v.
"""
import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import oracle as O
from test_gpu_evp import DIAG, cmp_region, gpu_fields
from test_gpu_free_drift import model_of

pytestmark = pytest.mark.gpu

HALOS = [(5, 3), (3, 5)]
WENO7_HALOS = [(6, 4), (4, 6)]
GRIDS = {
    "periodic": dict(Nx=40, Ny=28, topo=("periodic", "periodic")),
    "walls": dict(Nx=28, Ny=40, topo=("bounded", "bounded")),
    "masked_channel": dict(Nx=40, Ny=28, topo=("periodic", "bounded"), land=0.25),
    "latlon": dict(Nx=28, Ny=40, topo=("bounded", "bounded"), grid="latlon"),
    "curvilinear_fold": dict(Nx=40, Ny=28, topo=("periodic", "folded"), curvilinear=0.04),
}
SUBSTEPS = 5
_TOPO_ID = {"periodic": csi._lib.PERIODIC, "bounded": csi._lib.BOUNDED, "folded": csi._lib.RIGHT_FOLDED}


def record_path(test, case, what):
    """One line per case: the kernel family csi_last_path / csi_last_advection reported, printed (pytest -s shows the lines;
    profiles/r24_halo_coverage.md keeps the table made from them)."""
    print(f"[halo-paths] {test} | {case} | {what}")


def hid(h):
    return f"H{h[0]}x{h[1]}"


def expected_level(c, mode, fusion, n):
    """The kernel family csi_last_path must report (0: three kernels, 1: one sub-step per launch, 2: two sub-steps per launch) for a
    sub-cycle of n sub-steps: the rule of csi_launch.hip do_subcycle over the keywords of a case, with csi_plan_pair for the sizes."""
    if mode == "strict" or fusion == 0:
        return 0
    g = c["g"]
    pair = fusion == 2 and n >= 2 and csi._lib.plan_pair(g.Nx, g.Ny, g.Hx, g.Hy, _TOPO_ID[c["topo"][0]], _TOPO_ID[c["topo"][1]]) is not None
    if c["topo"][1] == "folded":
        # the band: the pair kernel below row M = Ny - Hy - 4 (csi_fold.hip fold_band_supported), three kernels next to the fold
        M = g.Ny - g.Hy - 4
        band = fusion == 2 and n >= 2 and min(g.Hx, g.Hy) >= 4 and M >= 2 * g.Hy + 8 and g.Nx >= 2 * g.Hx
        return 2 if band else 0
    array_forcing = c.get("field_forcing") or c.get("wind_drag") == "arrays" or c.get("bottom") == "arrays" or c.get("free_drift") or c.get("user_forcing")
    if c.get("mask") is not None or array_forcing or c["g"].metrics()["kind"] == "full":
        return 2 if pair else 0                           # configurations only the two-sub-steps kernel fuses
    return 2 if pair else 1


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def first_difference(a, b):
    w = np.argwhere(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64))
    return (len(w), tuple(w[0]), float(a[tuple(w[0])]), float(b[tuple(w[0])])) if len(w) else None


@pytest.mark.parametrize("halo", HALOS, ids=hid)
@pytest.mark.parametrize("name", list(GRIDS))
def test_strict_time_step_momentum_bitwise_vs_oracle(name, halo, oracle_lib):
    c = cases.make_case(H=halo, substeps=SUBSTEPS, patches=False, random_uv=0.03, **GRIDS[name])
    assert (c["g"].Hx, c["g"].Hy) == halo
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode="strict")
    for k, f in (("u", m.velocities.u), ("v", m.velocities.v), ("h", m.ice_thickness), ("aice", m.ice_concentration)):
        assert bits_equal(f.numpy(), p.f[k]), (k, "after update_state!", first_difference(f.numpy(), p.f[k]))
    p.time_step_momentum(c["dt"])
    csi.time_step_momentum(m, c["dt"])
    g = gpu_fields(m)
    assert m.ctx.last_path()["level"] == 0
    record_path("strict vs oracle", f"{name} {hid(halo)}", "level 0 (STRICT: four launches per sub-step)")
    assert bits_equal(g["P"], p.f["P"]), ("P", first_difference(g["P"], p.f["P"]))          # (compact ice: exp() at 0 only)
    assert np.abs(p.f["u"]).max() > 0 and not bits_equal(p.interior("u"), c["u"])
    for k in ("u", "v", "s11", "s22", "s12", "alpha", "zeta_c", "zeta_f", "Delta"):
        assert np.all(np.isfinite(g[k])), k
        assert bits_equal(g[k], p.f[k]), (name, halo, k, first_difference(g[k], p.f[k]))


@pytest.mark.parametrize("n", [4, 5], ids=["even", "odd"])
@pytest.mark.parametrize("halo", HALOS + WENO7_HALOS, ids=hid)      # (H >= 4 in both directions: the two-sub-steps kernel applies)
@pytest.mark.parametrize("name", list(GRIDS))
def test_fast_paths_agree_and_stay_close_to_strict(name, halo, n):
    c = cases.make_case(H=halo, substeps=n, patches=True, random_uv=0.03, **GRIDS[name])
    strict = cases.csi_model(c, mode="strict")
    csi.time_step_momentum(strict, c["dt"])
    s = gpu_fields(strict)
    vmax = max(np.abs(s["u"]).max(), np.abs(s["v"]).max())
    out = {}
    for fusion in (0, 1, 2):
        m = cases.csi_model(c, mode="fast")
        m.set_fusion(fusion)
        csi.time_step_momentum(m, c["dt"])
        g = gpu_fields(m)
        level = m.ctx.last_path()["level"]
        record_path("fast paths", f"{name} {hid(halo)} n={n} fusion {fusion}", f"level {level}")
        assert level == expected_level(c, "fast", fusion, n), (fusion, level)
        for k in ("u", "v"):
            d = np.abs(g[k] - s[k]).max()
            assert np.all(np.isfinite(g[k])) and d <= 1e-12 * vmax, (fusion, k, d, vmax)
            assert np.array_equal(g[k] == 0.0, s[k] == 0.0), (fusion, k, "zero sets differ")
        # u, v, s11, s22 on whole parents; s12 and the diagnostics where every path defines them: cmp_region, which keeps the periodic
        # halo images of the diagnostics (all but the outermost layer) -- the cells where a swapped image store would show
        out[fusion] = {k: cmp_region(c, k, g[k]).copy() for k in ("u", "v", "s11", "s22", "s12") + DIAG}
    for fusion in (1, 2):
        for k in out[0]:
            assert bits_equal(out[0][k], out[fusion][k]), (name, halo, n, fusion, k, first_difference(out[0][k], out[fusion][k]))
    assert not bits_equal(out[0]["u"], s["u"])            # FAST ran its own arithmetic


STEPS = {"rk3_weno7": ("SplitRungeKutta3", WENO7_HALOS), "fe_slab": ("ForwardEuler", HALOS + WENO7_HALOS)}
STEP_GRIDS = {"periodic": dict(Nx=40, Ny=28, topo=("periodic", "periodic")), "walls": dict(Nx=28, Ny=40, topo=("bounded", "bounded")),
              "masked_channel": dict(Nx=40, Ny=28, topo=("periodic", "bounded"), land=0.25)}


@pytest.mark.parametrize("name", list(STEP_GRIDS))
@pytest.mark.parametrize("step,halo", [(s, h) for s, (_, hs) in STEPS.items() for h in hs], ids=lambda x: x if isinstance(x, str) else hid(x))
def test_strict_whole_step_bitwise_vs_oracle(step, halo, name, oracle_lib):
    """One RK3 step with WENO7 (four halo layers in both directions) and one FE step with the bare-ice slab (WENO5, three layers).
    Compact ice at the start: the FE step's one momentum step needs exp() at 0 only.  The later stages of an RK3 step see aice < 1
    where the ice diverged, and there exp() -- the one transcendental function of the whole step, device libm against glibc -- may
    differ in the last bit (with the default hardening C = 20: h and aice equal bit for bit and one to three velocity points are one
    unit in the last place apart, the same points at halo (6,4) and (4,6); tests/test_gpu_steps.py bounds whole steps at 1e-12 for this
    reason).  The RK3 case therefore runs with ice_compaction_hardening = 0, P = P* h exp(-0 (1 - aice)) = P* h on both sides:
    everything else of the step -- every index, every image, every sum -- is compared bit for bit."""
    stepper = STEPS[step][0]
    scheme, adv = (7, csi.WENO(order=7)) if step == "rk3_weno7" else (5, csi.WENO(order=5))
    c = cases.make_case(H=halo, substeps=SUBSTEPS, patches=False, random_uv=0.03, **STEP_GRIDS[name])
    p = cases.oracle_problem(c)
    kw, slab_o, rheology = {}, None, None
    if step == "rk3_weno7":
        p.s.C_star = 0.0
        rheology = csi.ElastoViscoPlasticRheology(ice_compaction_hardening=0.0)
    if step == "fe_slab":
        slab_o = O.make_slab(Tu=-5.0, top_flux_kind=0, Qu=100.0, Qb=10.0)
        kw["ice_thermodynamics"] = csi.SlabThermodynamics(top_temperature=-5.0, top_heat_flux=100.0, bottom_heat_flux=10.0)
    m = model_of(c, rheology=rheology, mode="strict", timestepper=stepper, advection=adv, **kw)
    if stepper == "ForwardEuler":
        p.time_step_fe(c["dt"], scheme, True, slab=slab_o)
    else:
        p.time_step_rk3(c["dt"], scheme, slab=slab_o)
    csi.time_step(m, c["dt"])
    m.synchronize()
    adv_path = m.ctx.last_advection()
    record_path("whole step", f"{step} {name} {hid(halo)}", f"level {m.ctx.last_path()['level']}, advection {adv_path}")
    assert m.ctx.last_path()["level"] == 0 and adv_path["stage_fused"] == 0
    assert not bits_equal(p.interior("h"), c["h"]) and not bits_equal(p.interior("u"), c["u"])
    for k, f in (("h", m.ice_thickness), ("aice", m.ice_concentration), ("u", m.velocities.u), ("v", m.velocities.v)):
        a = f.numpy()
        print(step, name, hid(halo), k, "differing cells:", first_difference(a, p.f[k]))
        assert np.all(np.isfinite(a)), k
        assert bits_equal(a, p.f[k]), (step, name, halo, k, first_difference(a, p.f[k]))



@pytest.mark.parametrize("name", list(STEP_GRIDS))
@pytest.mark.parametrize("halo", WENO7_HALOS, ids=hid)
def test_strict_rk3_step_with_default_hardening_vs_oracle(halo, name, oracle_lib):
    """The same RK3 step with the default ice_compaction_hardening, exp() in play in the later stages: the bound
    tests/test_gpu_steps.py sets for whole STRICT steps, 1e-12 of the field's maximum on u, v, h, aice, with equal zero sets."""
    c = cases.make_case(H=halo, substeps=SUBSTEPS, patches=False, random_uv=0.03, **STEP_GRIDS[name])
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode="strict", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7))
    p.time_step_rk3(c["dt"], 7)
    csi.time_step(m, c["dt"])
    m.synchronize()
    assert m.ctx.last_path()["level"] == 0 and m.ctx.last_advection()["stage_fused"] == 0
    vmax = max(np.abs(p.f["u"]).max(), np.abs(p.f["v"]).max())
    for k, f, scale in (("u", m.velocities.u, vmax), ("v", m.velocities.v, vmax), ("h", m.ice_thickness, np.abs(p.f["h"]).max()),
                        ("aice", m.ice_concentration, np.abs(p.f["aice"]).max())):
        a = f.numpy()
        d = np.abs(a - p.f[k]).max()
        print("rk3 default hardening", name, hid(halo), k, "max difference", d, "of", scale, "differing cells:", first_difference(a, p.f[k]))
        assert np.all(np.isfinite(a)) and d <= 1e-12 * scale, (name, halo, k, d, scale)
        assert np.array_equal(a == 0.0, p.f[k] == 0.0), (name, halo, k, "zero sets differ")
