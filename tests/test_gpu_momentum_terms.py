"""GPU tests of csi_momentum_terms_compute / csi_momentum_budget_compute (include/csi.h): the ten term fields, the interface stresses and
the five powers, bit for bit against the restatement (tests/momentum_terms_ref.py) in both modes -- at the block edges of the kernels, on
every topology and metric kind, with and without land, for every stress kind on each side, every Coriolis kind, user forcing, every
dynamics configuration, with NaN / 1e300 in every halo element the contract does not name; the errors by name; the state after real RK3
steps; the explicit solver's own tendency; tiles, a north fold and two processes; the output writer; and a model that never asks."""
import math
import multiprocessing as mp
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import derived_ref
import diagnostics_ref as dref
import momentum_terms_ref as ref
import oracle as O
import output_ref
from momentum_ref import Ref

pytestmark = pytest.mark.gpu
L = csi._lib
HERE = os.path.dirname(os.path.abspath(__file__))
NGPU = torch.cuda.device_count() if torch.cuda.is_available() else 0
SENTINEL = 7.25
NU = 1000.0
IBC = ((0.02, -0.03, 0.01, 0.04), (0.03, 0.01, -0.02, 0.02))
TOPOS = {"PxP": ("periodic", "periodic"), "PxB": ("periodic", "bounded"), "BxB": ("bounded", "bounded")}
# 37 x 29: narrower than a wave; 63 x 8: with a Bounded x the last face is the last lane of the only block column; 64 x 16: ... is alone in
# a one-column block; 65 x 5: a one-column (two with the face) last block, fewer rows than a block and a half; 130 x 33: three block columns
SHAPES = ((37, 29), (63, 8), (64, 16), (65, 5), (130, 33))


def model_with(case, as_dynamics=False, rheology=None, solver=None, override=None, **kw):
    """cases.csi_model with the dynamics' rheology / solver / stress keywords replaced, or with StressBalanceFreeDrift built on the
    case's stresses as the whole dynamics."""
    orig = csi.SeaIceMomentumEquation

    def dynamics(g, **k):
        k.update(override or {})
        if as_dynamics:
            return csi.StressBalanceFreeDrift(top_momentum_stress=k.get("top_momentum_stress"), bottom_momentum_stress=k.get("bottom_momentum_stress"))
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


def evp_fields(m):
    f = getattr(getattr(m.dynamics, "auxiliaries", None), "fields", None)
    return f if f is not None and hasattr(f, "s11") else None


def set_sigma(m, seed=5):
    """noise in the stored stresses, halos included"""
    f, rng = evp_fields(m), np.random.default_rng(seed)
    for k, amp in (("s11", 50.0), ("s22", 50.0), ("s12", 30.0)):
        fld = getattr(f, k)
        m.copy_to_field(fld, amp * rng.standard_normal((fld.nj, fld.ni)))


def input_fields(m, p):
    """(oracle array, model field) of everything the terms read"""
    out = [(p.f["u"], m.velocities.u), (p.f["v"], m.velocities.v), (p.f["h"], m.ice_thickness), (p.f["aice"], m.ice_concentration)]
    f = evp_fields(m)
    if f is not None:
        out += [(p.f[k], getattr(f, k)) for k in ("s11", "s22", "s12")]
    r = Ref(p)
    for side, st in (("TOP", p.s.top), ("BOT", p.s.bottom)):
        for comp, fo, vel_kind in (("U", st.fu, st.ue_kind), ("V", st.fv, st.ve_kind)):
            if st.kind == O.STRESS_FIELD or (st.kind == O.STRESS_SEMI_IMPLICIT and vel_kind == O.VEL_FIELD):
                out.append((r._arr(fo, comp.lower()), m._stress_fields[f"{side}_{comp}"]))
    if p.s.has_forcing:
        out += [(r._arr(p.s.forcing_u, "u"), m.forcing_fields.u), (r._arr(p.s.forcing_v, "v"), m.forcing_fields.v)]
    return out


def sync(m, p):
    """the oracle problem's arrays := the model's parents, halos included"""
    m.synchronize()
    for arr, fld in input_fields(m, p):
        arr[...] = fld.numpy()


def check_fields(m, t, what, modes=("strict", "fast"), raw=True):
    """all ten fields (one launch) and both interface stresses equal the restatement bit for bit in both modes; returns the restatement"""
    want = t.fields()
    for mode in modes:
        m.set_mode(mode)
        fields = m.compute_momentum_terms(*ref.TERMS)
        m.synchronize()
        for n, fld in zip(ref.FIELDS, fields):
            got = fld.interior_numpy()
            assert np.all(np.isfinite(got)), (what, n, mode)
            assert ref.same_bits(got, want[n]), (what, n, mode, np.argwhere(got != want[n])[:4].tolist())
    if raw:
        wraw = t.fields(raw=True)
        for side in ("top", "bottom"):
            tx, ty = m.interface_stress(side)
            m.synchronize()
            assert ref.same_bits(tx.interior_numpy(), wraw[f"{side}_x"]) and ref.same_bits(ty.interior_numpy(), wraw[f"{side}_y"]), (what, side)
    return want


def evp_pair(kw, sigma=True, **model_kw):
    c = cases.make_case(**kw)
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, **model_kw)
    if sigma:
        set_sigma(m)
    sync(m, p)
    return c, p, m


# ---- 1. shapes and topologies --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topo", list(TOPOS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_topologies(shape, topo, oracle_lib):
    c, p, m = evp_pair(dict(Nx=shape[0], Ny=shape[1], topo=TOPOS[topo], random_uv=0.03, user_forcing=True, wind_drag="numbers"))
    t = ref.TermsRef(p)
    for n in ref.FIELDS:
        m.momentum_term(n).fill_parent(SENTINEL)
    want = check_fields(m, t, (shape, topo), raw=False)
    g = c["g"]
    for n in ref.FIELDS:                                   # the interior and nothing else is written
        parent = m.momentum_term(n).numpy().copy()
        ny, nx = want[n].shape
        parent[g.Hy:g.Hy + ny, g.Hx:g.Hx + nx] = SENTINEL
        assert np.all(parent == SENTINEL), (n, "halo written")
    if TOPOS[topo][0] == "bounded":                        # wall faces, the last one included: peripheral nodes hold +0.0
        assert want["top_x"].shape == (shape[1], shape[0] + 1)
        for n in ref.FIELDS[::2]:
            assert np.all(want[n][:, 0] == 0.0) and np.all(want[n][:, -1] == 0.0)
    assert all(np.abs(want[n]).max() > 0 for n in ref.FIELDS)


# ---- 2. metrics and land -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("land", [False, True], ids=["open", "land"])
@pytest.mark.parametrize("metrics", ["uniform", "latlon", "curvilinear"])
def test_metrics_and_land(metrics, land, oracle_lib):
    kw = dict(Nx=37, Ny=29, topo=TOPOS["PxB"], random_uv=0.03, grid="rectilinear" if metrics == "uniform" else "latlon",
              curvilinear=0.1 if metrics == "curvilinear" else None)
    if land:
        kw.update(land=0.15, immersed_bc=IBC)
    c, p, m = evp_pair(kw)
    t = ref.TermsRef(p)
    want = check_fields(m, t, (metrics, land))
    if land:                                               # the immersed flux term is there, and faces next to land hold +0.0
        bare = cases.make_case(**dict(kw, immersed_bc=None))
        pb = cases.oracle_problem(bare)
        sync(m, pb)
        assert not ref.same_bits(ref.TermsRef(pb).fields()["internal_x"], want["internal_x"])
        wet = c["mask"]
        dry_u = ~(wet & np.roll(wet, 1, axis=1))
        assert dry_u.any() and all(np.all(want[n][dry_u] == 0.0) for n in ref.FIELDS[::2])


# ---- 3. stress kinds, each side ------------------------------------------------------------------------------------------------------------
STRESSES = {
    "nothing_nothing": (dict(top=None, bottom=None), None, None),
    "numbers_semi_zero": (dict(), None, None),
    "arrays_semi_arrays": (dict(field_forcing=True), None, None),
    "semi_numbers_arrays": (dict(wind_drag="numbers", bottom="arrays"), None, None),
    "numbers_semi_numbers": (dict(ue=0.05, ve=-0.02), None, None),
    "wind_arrays_ocean_arrays": (dict(field_forcing=True, wind_drag="arrays"), None, None),
    "nothing_numbers": (dict(top=None, bottom=None), dict(bottom_momentum_stress=(0.004, -0.003)), ("bottom", (0.004, -0.003))),
    "semi_zero_nothing": (dict(top=None, bottom=None), dict(top_momentum_stress=csi.SemiImplicitStress(rho_e=1.3, Cd=1.2e-3)),
                          ("top", None)),
}


@pytest.mark.parametrize("name", list(STRESSES))
def test_stress_kinds(name, oracle_lib):
    kw, override, ora = STRESSES[name]
    c = cases.make_case(Nx=37, Ny=29, topo=TOPOS["PxB"], random_uv=0.03, **kw)
    p = cases.oracle_problem(c)
    if ora is not None:
        side, tau = ora
        if tau is not None:
            p.set_stress(side, O.STRESS_CONST, tau=tau)
        else:
            p.set_stress(side, O.STRESS_SEMI_IMPLICIT, rho_e=1.3, Cd=1.2e-3)
    m = model_with(c, override=override)
    set_sigma(m)
    sync(m, p)
    t = ref.TermsRef(p)
    want = check_fields(m, t, name)
    for side, st in (("top", p.s.top), ("bottom", p.s.bottom)):
        some = np.abs(want[f"{side}_x"]).max() > 0
        assert some == (st.kind != O.STRESS_NONE), (name, side)


# ---- 4. Coriolis, 5. model.forcing arrays --------------------------------------------------------------------------------------------------
CORIOLIS = {"fplane": dict(), "betaplane_rows": dict(beta=2e-11, topo=TOPOS["BxB"]), "points": dict(curvilinear=0.15, coriolis_points=True),
            "none": dict(coriolis=None), "none_forcing": dict(coriolis=None, user_forcing=True), "fplane_forcing_latlon": dict(grid="latlon", user_forcing=True)}


@pytest.mark.parametrize("name", list(CORIOLIS))
def test_coriolis_kinds_and_user_forcing(name, oracle_lib):
    c, p, m = evp_pair(dict(dict(Nx=37, Ny=29, random_uv=0.03), **CORIOLIS[name]))
    want = check_fields(m, ref.TermsRef(p), name, raw=False)
    assert (np.abs(want["coriolis_x"]).max() > 0) == (not name.startswith("none"))
    assert (np.abs(want["forcing_y"]).max() > 0) == ("forcing" in name)
    if name.startswith("none"):                            # no Coriolis: +0.0, not -0.0
        assert not np.signbit(want["coriolis_x"]).any() and not np.signbit(want["coriolis_y"]).any()


# ---- 6. dynamics ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["evp_split", "evp_explicit", "viscous_split", "viscous_explicit", "free_drift"])
def test_dynamics_configurations(config, oracle_lib):
    c = cases.make_case(Nx=65, Ny=20, topo=TOPOS["BxB"], random_uv=0.03, land=0.12, immersed_bc=IBC, user_forcing=True, substeps=4)
    p = cases.oracle_problem(c)
    if config == "free_drift":
        p.set_coriolis(None)                               # StressBalanceFreeDrift carries no Coriolis term
        m = model_with(c, as_dynamics=True)
        assert isinstance(m.dynamics, csi.StressBalanceFreeDrift)
        t = ref.TermsRef(p, rheology=None, rho=m.sea_ice_density)
    else:
        viscous = config.startswith("viscous")
        m = model_with(c, rheology=csi.ViscousRheology(nu=NU) if viscous else None,
                       solver=csi.ExplicitSolver() if config.endswith("explicit") else csi.SplitExplicitSolver(substeps=4))
        if not viscous:
            set_sigma(m)
        t = ref.TermsRef(p, rheology="viscous" if viscous else "evp", nu=NU)
    sync(m, p)
    want = check_fields(m, t, config)
    assert (np.abs(want["internal_x"]).max() > 0) == (config != "free_drift")
    assert (np.abs(want["coriolis_y"]).max() > 0) == (config != "free_drift")
    b = m.momentum_budget()
    for k, v in t.budget().items():
        assert dref.same_bits(getattr(b, k), v), (config, k, getattr(b, k), v)


# ---- 7. the halo contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beyond", [np.nan, 1e300], ids=["nan", "1e300"])
def test_halo_contract(beyond, oracle_lib):
    """White noise in every input, one ring around each field's own interior included; NaN in every halo element the contract does not
    name -- and, in the second run, 1e300 in the layer just beyond the ring, which a select or a comparison would let through where NaN
    stands out.  Fields and powers equal the restatement fed the same parents, and are finite."""
    c = cases.make_case(Nx=37, Ny=29, topo=TOPOS["PxB"], grid="latlon", random_uv=0.03, land=0.15, immersed_bc=IBC, field_forcing=True,
                        wind_drag="arrays", user_forcing=True)
    p = cases.oracle_problem(c)
    m = cases.csi_model(c)
    g, rng = c["g"], np.random.default_rng(31)
    for arr, fld in input_fields(m, p):
        nx, ny = g.interior_size(fld.LX, fld.LY)
        a = np.abs(arr).max() * rng.standard_normal(arr.shape) if np.abs(arr).max() > 0 else 40.0 * rng.standard_normal(arr.shape)
        if fld in (m.ice_thickness, m.ice_concentration):
            a = np.abs(a)
        poisoned = np.full(arr.shape, np.nan)
        poisoned[g.Hy - 2:g.Hy + ny + 2, g.Hx - 2:g.Hx + nx + 2] = beyond
        ring = (slice(g.Hy - 1, g.Hy + ny + 1), slice(g.Hx - 1, g.Hx + nx + 1))
        poisoned[ring] = a[ring]
        m.copy_to_field(fld, poisoned)
    sync(m, p)
    t = ref.TermsRef(p)
    want = check_fields(m, t, ("halo", beyond))
    assert all(np.abs(want[n]).max() > 0 for n in ref.FIELDS)
    b = m.momentum_budget()
    for k, v in t.budget().items():
        assert math.isfinite(v) and dref.same_bits(getattr(b, k), v), (k, getattr(b, k), v)


# ---- 8. mask bits, 9. zero mass ------------------------------------------------------------------------------------------------------------
def test_mask_bits_and_zero_mass(oracle_lib):
    c, p, m = evp_pair(dict(Nx=65, Ny=20, topo=TOPOS["PxB"], random_uv=0.03, user_forcing=True, patches=True))
    t = ref.TermsRef(p)
    want = check_fields(m, t, "all ten", raw=False)
    # cells without ice: m_i = 0 at the faces between two of them -> every slot +0.0 there, and elsewhere not all zero
    ice = (c["h"] * c["a"]) > 0
    no_mass_u = ~(ice | np.roll(ice, 1, axis=1))
    assert no_mass_u.sum() > 10
    for n in ref.FIELDS[::2]:
        assert np.all(want[n][no_mass_u] == 0.0) and not np.signbit(want[n][no_mass_u]).any() and np.abs(want[n][~no_mass_u]).max() > 0
    fields = {n: m.momentum_term(n) for n in ref.FIELDS}
    for term in ref.TERMS:                                 # each bit alone: its two slots and nothing else
        for fld in fields.values():
            fld.fill_parent(SENTINEL)
        got = m.compute_momentum_terms(term)
        m.synchronize()
        assert [f.name for f in got] == [f"{term}_x", f"{term}_y"]
        for n, fld in fields.items():
            if n.startswith(term):
                assert ref.same_bits(fld.interior_numpy(), want[n]), (term, n)
            else:
                assert np.all(fld.numpy() == SENTINEL), (n, "written by a call for", term)
    one, = m.compute_momentum_terms("internal_y")          # a component's name selects the term: both slots are filled
    m.synchronize()
    assert one is fields["internal_y"] and ref.same_bits(fields["internal_x"].interior_numpy(), want["internal_x"])
    assert m.ctx.momentum_terms_stats() == (2 + 5 + 1, 0)


# ---- 10. errors by name --------------------------------------------------------------------------------------------------------------------
def test_errors_by_name():
    c = cases.make_case(Nx=37, Ny=29, random_uv=0.03)
    m = cases.csi_model(c)
    with pytest.raises(csi.CsiError, match="top_x") as e:          # the slot is not bound
        m.ctx.momentum_terms_compute(L.MTERM_TOP)
    assert e.value.code == -2
    m.momentum_term("top_x")
    with pytest.raises(csi.CsiError, match="top_y") as e:          # a bit selects both components
        m.ctx.momentum_terms_compute(L.MTERM_TOP)
    assert e.value.code == -2
    m.momentum_term("top_y")
    m.ctx.momentum_terms_compute(L.MTERM_TOP)
    m.ctx.momentum_terms_compute(L.MTERM_TOP | L.MTERM_RAW_STRESS)
    for mask in (0, 64, -1, L.MTERM_RAW_STRESS):
        with pytest.raises(csi.CsiError, match="mask") as e:
            m.ctx.momentum_terms_compute(mask)
        assert e.value.code == -1
    for what in (0, 8, -1):
        with pytest.raises(csi.CsiError, match="what") as e:
            m.ctx.momentum_budget_compute(what)
        assert e.value.code == -1
    with pytest.raises(ValueError, match="coriolis_x, coriolis_y"):
        m.compute_momentum_terms("inertia")
    # the internal term of an EVP model names the stress field it misses; the other terms and groups do not need it
    m.ctx.call("csi_field_bind", L.F["S12"], None, 0, 0, 0)
    for call in (lambda: m.compute_momentum_terms("internal"), lambda: m.momentum_budget(), lambda: m.momentum_budget("internal")):
        with pytest.raises(csi.CsiError, match="sigma12") as e:
            call()
        assert e.value.code == -2
    m.compute_momentum_terms("top", "bottom", "coriolis", "forcing")
    b = m.momentum_budget(("external", "body"))
    assert b.internal is None and b.residual is None and math.isfinite(b.bottom) and b.forcing == 0.0
    # u, v, h, aice by name
    for slot, name in (("A", "aice"), ("H", "h"), ("V", "v")):
        m.ctx.call("csi_field_bind", L.F[slot], None, 0, 0, 0)
        for call in (lambda: m.ctx.momentum_terms_compute(L.MTERM_TOP), lambda: m.ctx.momentum_budget_compute(L.MBUDGET_BODY)):
            with pytest.raises(csi.CsiError, match=rf"needs field {name} ") as e:
                call()
            assert e.value.code == -2
    # a free-drift-dynamics model has no rheology: the internal term is +0.0 and needs no stress field, h and aice are still needed
    d = model_with(c, as_dynamics=True)
    ix, iy = d.compute_momentum_terms("internal")
    d.synchronize()
    assert np.all(ix.numpy() == 0.0) and np.all(iy.numpy() == 0.0) and d.momentum_budget("internal").internal == 0.0
    d.ctx.call("csi_field_bind", L.F["H"], None, 0, 0, 0)
    with pytest.raises(csi.CsiError, match="needs field h "):
        d.compute_momentum_terms("internal")
    # a model without dynamics binds u, v, h, aice: the terms of a state without stresses, the term fields listed once allocated
    n = csi.SeaIceModel(c["g"], dynamics=None, advection=None, timestepper="ForwardEuler")
    assert "bottom_x" not in csi.bound_fields(n)
    n.compute_momentum_terms("bottom")
    assert csi.bound_fields(n)["bottom_x"][1] == "M_BOTTOM_X" and csi.bound_fields(n)["bottom_y"][0].location == (csi.Center, csi.Face)


# ---- 11. the state after real steps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("config", ["bounded_latlon_land", "periodic_uniform_forcing"])
def test_after_three_rk3_steps(config, mode, oracle_lib):
    """The halo elements the entry points read are the ones the step entry points leave valid: fields and powers of the stepped state
    against the restatement fed the DOWNLOADED parents, halos included."""
    kw = {"bounded_latlon_land": dict(topo=TOPOS["BxB"], grid="latlon", land=0.2, immersed_bc=IBC, field_forcing=True),
          "periodic_uniform_forcing": dict(topo=TOPOS["PxP"], user_forcing=True, wind_drag="arrays")}[config]
    c = cases.make_case(Nx=65, Ny=33, random_uv=0.02, substeps=12, **kw)
    p = cases.oracle_problem(c)
    m = cases.csi_model(c, mode=mode, timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    for _ in range(3):
        csi.time_step(m, c["dt"])
    sync(m, p)
    t = ref.TermsRef(p)
    want = check_fields(m, t, config, modes=(mode,))
    assert np.abs(want["internal_x"]).max() > 0 and np.abs(want["bottom_y"]).max() > 0
    b = m.momentum_budget()
    sums = t.budget()
    for k, v in sums.items():
        assert dref.same_bits(getattr(b, k), v), (config, k, getattr(b, k), v)
    assert b.bottom < 0.0 and b.residual == math.fsum(sums.values())


# ---- 12. the explicit solver's own tendency ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rheo", ["viscous", "evp"])
@pytest.mark.parametrize("topo", ["PxP", "BxB"])
def test_explicit_solver_tendency_is_the_sum_of_the_fields(topo, rheo):
    """An ExplicitSolver model without implicit stresses: m_i G from csi_compute_momentum_tendencies against the sum of the GPU's own
    five fields, within 32 * 2^-53 * sum |F_k| / m_i (tests/test_momentum_terms_ref.py states where the bound comes from).  EVP: u^n = u,
    so that the pseudo-time term of sum_of_forcing_*, which is not one of the five, is (u^n - u) / dt / alpha = 0."""
    c = cases.make_case(Nx=65, Ny=20, topo=TOPOS[topo], random_uv=0.03, bottom="arrays", user_forcing=True)
    m = model_with(c, rheology=csi.ViscousRheology(nu=NU) if rheo == "viscous" else None, solver=csi.ExplicitSolver(), mode="strict")
    if rheo == "evp":
        set_sigma(m)
        f = evp_fields(m)
        m.copy_to_field(f.un, m.velocities.u.numpy())
        m.copy_to_field(f.vn, m.velocities.v.numpy())
    csi.compute_momentum_tendencies(m, 60.0)
    fields = dict(zip(ref.FIELDS, m.compute_momentum_terms(*ref.TERMS)))
    m.synchronize()
    g, rho = c["g"], m.sea_ice_density
    mass = m.ice_thickness.numpy() * rho * m.ice_concentration.numpy()
    inner = lambda a, di=0, dj=0: a[g.Hy + dj:g.Hy + dj + g.Ny, g.Hx + di:g.Hx + di + g.Nx]
    for comp, G, mi in (("x", m.timestepper.Gn.u, (inner(mass, -1, 0) + inner(mass)) / 2), ("y", m.timestepper.Gn.v, (inner(mass, 0, -1) + inner(mass)) / 2)):
        F = [fields[f"{t}_{comp}"].interior_numpy()[:g.Ny, :g.Nx] for t in ref.TERMS]
        Gi = inner(G.numpy())
        ok = mi > 0
        if topo == "BxB":                                  # the wall faces are peripheral nodes: the fields hold +0.0, G what the stencil gives
            ok[:, 0] &= comp != "x"
            ok[0, :] &= comp != "y"
        total, mag = sum(F), sum(np.abs(x) for x in F)
        err = np.abs(total[ok] / mi[ok] - Gi[ok])
        bound = 32 * 2.0 ** -53 * mag[ok] / mi[ok]
        print(topo, rheo, comp, "worst error / bound", float((err / bound).max()), "points", int(ok.sum()))
        assert ok.sum() > 500 and np.abs(Gi[ok]).max() > 0 and np.all(err <= bound)
        assert np.all(total[~(mi > 0)] == 0.0)


# ---- 13. the budget ------------------------------------------------------------------------------------------------------------------------
# (16385 x 4: 257 x 1 records, more than the finishing block has 256 threads -- thread 0 adds records 0 and 256; a thin grid because the
#  restatement walks the points in Python: 65 540 points are a few seconds, the 17 x 16 blocks of a square grid would be most of a minute)
@pytest.mark.parametrize("shape", [(64, 64), (65, 65), (130, 65), (16385, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_budget_at_the_record_layout_edges(shape, oracle_lib):
    """Uniform doubly periodic f-plane, uniform h and aice, random u and v, a wind stress and an ocean at rest: the five powers equal
    the restatement bit for bit in both modes and on repeated calls; the Coriolis power vanishes within (2 n + 8) 2^-53 sum |summand|;
    the drag takes energy out; one group alone leaves the other members NaN in the C struct, None in the record."""
    c = cases.make_case(Nx=shape[0], Ny=shape[1], random_uv=0.1, patches=False, noise=0.0, user_forcing=True)
    c["h"][...] = 1.25
    c["a"][...] = 0.75
    p = cases.oracle_problem(c)
    m = cases.csi_model(c)
    set_sigma(m)
    sync(m, p)
    t = ref.TermsRef(p)
    f = t.fields(extent=False)
    sums = t.budget(f)
    for mode in ("strict", "fast", "strict"):
        m.set_mode(mode)
        b = m.momentum_budget()
        for k, v in sums.items():
            assert dref.same_bits(getattr(b, k), v), (shape, mode, k, getattr(b, k), v)
    az = float(p.s.dx * p.s.dy)
    px, py = (p.interior("u") * f["coriolis_x"]) * az, (p.interior("v") * f["coriolis_y"]) * az
    bound = (2 * px.size + 8) * 2.0 ** -53 * math.fsum(np.abs(px).ravel().tolist() + np.abs(py).ravel().tolist())
    print(shape, "coriolis power", b.coriolis, "bound", bound, "top", b.top, "bottom", b.bottom, "internal", b.internal, "forcing", b.forcing)
    assert abs(b.coriolis) <= bound and b.bottom < 0.0 and b.top != 0.0 and b.internal != 0.0 and b.forcing != 0.0
    assert b.residual == math.fsum(sums.values()) and b.what == ("external", "body", "internal")
    raw = m.ctx.momentum_budget_compute(L.MBUDGET_EXTERNAL)
    assert raw.what == 1 and dref.same_bits(raw.top, sums["top"]) and dref.same_bits(raw.bottom, sums["bottom"])
    assert all(math.isnan(getattr(raw, k)) for k in ("coriolis", "internal", "forcing"))
    one = m.momentum_budget("internal")
    assert dref.same_bits(one.internal, sums["internal"]) and one.top is None and one.coriolis is None and one.residual is None
    body = m.momentum_budget("body")
    assert dref.same_bits(body.coriolis, sums["coriolis"]) and dref.same_bits(body.forcing, sums["forcing"]) and body.internal is None
    assert m.ctx.momentum_terms_stats() == (0, 6)          # no field was asked for: no slot is bound
    assert m._momentum_term_fields == {}


# ---- 14. tiles, a north fold, two processes ------------------------------------------------------------------------------------------------
TILES = {"2x1_bounded_x": (2, 1, dict(Nx=128, Ny=64, topo=("bounded", "periodic"), user_forcing=True)),
         "2x2_channel_land": (2, 2, dict(Nx=128, Ny=96, topo=("periodic", "bounded"), land=0.2, field_forcing=True)),
         "1x2_fold": (1, 2, dict(Nx=192, Ny=192, topo=("periodic", "folded")))}
STEP_KW = dict(timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))


def _run(m, c, steps=2):
    for _ in range(steps):
        csi.time_step(m, c["dt"])
    fields = m.compute_momentum_terms(*ref.TERMS)
    b = m.momentum_budget()
    m.synchronize()
    return {n: f.interior_numpy().copy() for n, f in zip(ref.FIELDS, fields)}, {k: getattr(b, k) for k in ref.TERMS}


def _power_summands(m, fields):
    """(u F_x) Az^fc + (v F_y) Az^cf of an untiled model's own fields, per cell and term (NumPy, the documented order)"""
    g = m.grid
    r = derived_ref.Ref(g, {"u": m.velocities.u.numpy(), "v": m.velocities.v.numpy()})
    u, v, azfc, azcf = r.at("u"), r.at("v"), r.metric("az", "f", "c"), r.metric("az", "c", "f")
    return {t: (u * fields[f"{t}_x"][:g.Ny, :g.Nx]) * azfc + (v * fields[f"{t}_y"][:g.Ny, :g.Nx]) * azcf for t in ref.TERMS}


def _check_tiles(parts, want, bw, summands, what):
    """parts: per rank (fields, budget, (i_off, j_off)).  Fields reassembled == untiled bit for bit; budget bits equal on all ranks and
    within twice the order-independent bound of the untiled sum (the same terms in another tree)."""
    for n in ref.FIELDS:
        got = np.full_like(want[n], np.nan)
        for fields, _, (i0, j0) in parts:
            a = fields[n]
            got[j0:j0 + a.shape[0], i0:i0 + a.shape[1]] = a
        assert ref.same_bits(got, want[n]), (what, n, np.argwhere(got != want[n])[:4].tolist())
    for k in ref.TERMS:
        vals = [b[k] for _, b, _ in parts]
        assert all(dref.same_bits(v, vals[0]) for v in vals), (what, k, vals)
        _, bound = dref.fsum_bound(summands[k])
        print(what, k, "tiled", vals[0], "untiled", bw[k], "difference", vals[0] - bw[k], "bound", 2 * bound)
        assert abs(vals[0] - bw[k]) <= 2 * bound, (what, k)


def _untiled(kw):
    c = cases.make_case(substeps=8, random_uv=0.02, **kw)
    whole = cases.csi_model(c, **STEP_KW)
    want, bw = _run(whole, c)
    summands = _power_summands(whole, want)
    for k in ref.TERMS:                                    # the untiled budget is the ordered sum of the untiled fields' summands
        assert dref.same_bits(bw[k], dref.ordered_sum(summands[k])), k
    return c, want, bw, summands


@pytest.mark.parametrize("name", list(TILES))
def test_tiles_of_one_process(name):
    from test_gpu_local_tiles import run_tile_threads
    Rx, Ry, kw = TILES[name]
    c, want, bw, summands = _untiled(kw)
    assert np.abs(want["internal_x"]).max() > 0

    def tile(rank, group):
        m = cases.csi_model(c, tile=(Rx, Ry, rank), local_group=group, **STEP_KW)
        fields, b = _run(m, c)
        g = m.grid
        return fields, b, (g.i_off, g.j_off)

    _check_tiles(run_tile_threads(Rx * Ry, tile), want, bw, summands, name)


def _host_rank(conn, shm, kw, Rx, Ry, rank):
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    try:
        import cases as cs
        c = cs.make_case(substeps=8, random_uv=0.02, **kw)
        m = cs.csi_model(c, tile=(Rx, Ry, rank), host_group=shm, **STEP_KW)      # (this module, imported anew by the spawned process)
        fields, b = _run(m, c)
        conn.send((fields, b, (m.grid.i_off, m.grid.j_off)))
    except Exception as e:      # noqa: BLE001  (reported to the parent, which fails the test)
        conn.send({"error": repr(e)})


def test_two_processes_on_one_gpu_over_the_host_channel_group():
    kw = dict(Nx=96, Ny=96, topo=("bounded", "bounded"), land=0.2, H=4)
    Rx, Ry = 1, 2
    c, want, bw, summands = _untiled(kw)
    shm = f"/csi-test-{uuid.uuid4().hex[:12]}"
    ctx = mp.get_context("spawn")
    procs, pipes = [], []
    for r in range(Rx * Ry):
        a, b = ctx.Pipe()
        pr = ctx.Process(target=_host_rank, args=(b, shm, kw, Rx, Ry, r))
        pr.start()
        procs.append(pr); pipes.append(a)
    got = []
    for r in range(Rx * Ry):
        assert pipes[r].poll(300), f"rank {r} did not answer"
        got.append(pipes[r].recv())
    for pr in procs:
        pr.join(timeout=60)
    for r, d in enumerate(got):
        assert not isinstance(d, dict), (r, d.get("error"))
    _check_tiles(got, want, bw, summands, "host-channel group 1x2")


@pytest.mark.skipif(NGPU < 2, reason="needs at least 2 GPUs (one rank per GPU)")
def test_two_devices_over_rccl(tmp_path):
    import json
    kw = dict(Nx=128, Ny=96, H=8, topo=("bounded", "periodic"), land=0.2)
    c, want, bw, summands = _untiled(kw)
    port = str(29500 + os.getpid() % 90)
    out = str(tmp_path / "terms")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "momentum_terms_rank_worker.py"), str(r), "2", port, "2", "1", out,
                               json.dumps(kw)], env=env) for r in range(2)]
    for pr in procs:
        assert pr.wait(timeout=600) == 0
    got = []
    for r in range(2):
        z = np.load(f"{out}.rank{r}.npz")
        got.append(({n: z[n] for n in ref.FIELDS}, {k: float(z["budget"][q]) for q, k in enumerate(ref.TERMS)}, tuple(int(x) for x in z["offsets"])))
    _check_tiles(got, want, bw, summands, "RCCL 2x1")


# ---- 15. the output writer -----------------------------------------------------------------------------------------------------------------
def test_writer_with_term_outputs(tmp_path, oracle_lib):
    """["h", "bottom_x", "bottom_y", "internal_x"], snapshots and time averages: the records equal the stand-in's arithmetic on the
    restatement's fields of a twin's downloaded states; one launch per accumulate and per record."""
    c = cases.make_case(Nx=40, Ny=24, topo=TOPOS["BxB"], grid="latlon", random_uv=0.02, substeps=8)
    dt, names = c["dt"], ["h", "bottom_x", "bottom_y", "internal_x"]
    mk = lambda: cases.csi_model(c, timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    twin, states = mk(), []
    p = cases.oracle_problem(c)

    def state():
        sync(twin, p)
        f = ref.TermsRef(p).fields()
        f["h"] = twin.ice_thickness.interior_numpy().copy()
        return f
    states.append(state())
    for _ in range(4):
        csi.time_step(twin, dt)
        states.append(state())
    m = mk()
    m.output_writers["snap"] = csi.OutputWriter(m, names, csi.IterationInterval(2), str(tmp_path / "snap"), dtype="f64")
    m.output_writers["avg"] = csi.OutputWriter(m, names, csi.AveragedTimeInterval(2 * dt), str(tmp_path / "avg"), dtype="f32")
    assert m.output_writers["snap"].momentum_terms == ("bottom_x", "bottom_y", "internal_x") and m.output_writers["snap"].derived == ()
    for _ in range(4):
        csi.time_step(m, dt)
    for w in m.output_writers.values():
        w.close()
    snap, avg = csi.load_output(str(tmp_path / "snap")), csi.load_output(str(tmp_path / "avg"))
    assert list(snap["iteration"]) == [0, 2, 4] and list(avg["time"]) == [2 * dt, 4 * dt]
    assert snap["bottom_x"].shape[1:] == (24, 41) and snap["bottom_y"].shape[1:] == (25, 40)
    for n in names:
        for r, it in enumerate((0, 2, 4)):
            assert output_ref.same_bits(snap[n][r], states[it][n]), ("snap", n, it)
        for r in range(2):
            want = output_ref.element(output_ref.averaged([states[2 * r + k][n] for k in (1, 2)], [dt] * 2), "f32")
            assert output_ref.same_bits(avg[n][r], want), ("avg", n, r)
    # snapshots: 3 records; averages: 4 accumulates + 2 records -- one launch each, for either writer
    assert m.ctx.momentum_terms_stats() == (3 + 6, 0) and m.ctx.derived_stats() == (0, 0)


# ---- 16. a model that never asks -----------------------------------------------------------------------------------------------------------
def test_a_model_that_never_asks_makes_none_of_the_new_calls(tmp_path, monkeypatch):
    c = cases.make_case(Nx=65, Ny=33, topo=TOPOS["BxB"], grid="latlon", random_uv=0.02)
    m = cases.csi_model(c, timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    called = []
    for name in ("momentum_terms_compute", "momentum_budget_compute"):
        monkeypatch.setattr(type(m.ctx), name, lambda self, *a, _n=name: called.append(_n))
    with csi.OutputWriter(m, ["h", "u", "sigma12", "shear"], csi.IterationInterval(1), str(tmp_path / "w")) as w:
        m.output_writers["w"] = w
        assert w.momentum_terms == ()
        for _ in range(2):
            csi.time_step(m, c["dt"])
        m.diagnostics()
        m.energy_budget()
    monkeypatch.undo()
    assert called == [] and m.ctx.momentum_terms_stats() == (0, 0)
    assert m._momentum_term_fields == {} and not any(n in csi.bound_fields(m) for n in csi.TERM_FIELD_NAMES)
