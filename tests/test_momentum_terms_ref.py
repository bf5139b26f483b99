"""CPU tests of the definition of the momentum balance terms, the interface stresses and their power (include/csi.h): the restatement
(tests/momentum_terms_ref.py) reassembled into the tendency of tests/momentum_ref.py, the Coriolis identity and its ability to fail, the
sign of the drag against an ocean at rest, the internal power against the energy budget's restatement, the sums against math.fsum, the
layout of csi_momentum_budget and the slots as gcc, ctypes and the Julia stub see them, and the front end on the stand-in recorder of
tests/output_ref.py."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
import derived_ref
import diagnostics_ref as dref
import momentum_terms_ref as ref
import output_ref
from momentum_ref import Ref

L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IBC = ((0.02, -0.03, 0.01, 0.04), (0.03, 0.01, -0.02, 0.02))
GRIDS = {"uniform": dict(grid="rectilinear"), "latlon": dict(grid="latlon"), "curvilinear": dict(grid="latlon", curvilinear=0.1)}


def problem(metrics, land, seed=7, **kw):
    """A small oracle problem with noise in u, v, sigma, u^n, alpha; land comes with immersed flux boundary conditions."""
    extra = dict(land=0.15, immersed_bc=IBC) if land else {}
    c = cases.make_case(Nx=14, Ny=11, topo=("periodic", "bounded"), random_uv=0.03, user_forcing=True, **GRIDS[metrics], **extra, **kw)
    p = cases.oracle_problem(c)
    rng = np.random.default_rng(seed)
    for k, s in (("s11", 50.0), ("s22", 50.0), ("s12", 30.0)):
        p.f[k][...] = s * rng.standard_normal(p.f[k].shape)
    p.f["alpha"][...] = 50.0 + 200.0 * rng.random(p.f["alpha"].shape)
    p.f["un"][...] = p.f["u"] + 0.01 * rng.standard_normal(p.f["u"].shape)
    p.f["vn"][...] = p.f["v"] + 0.01 * rng.standard_normal(p.f["v"].shape)
    return c, p


def points(p, comp):
    return [(i, j) for j in range(1, p.s.Ny + 1) for i in range(1, p.s.Nx + 1)]


# ---- 1. reassembly -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("viscous", [True, False], ids=["viscous", "evp"])
@pytest.mark.parametrize("land", [False, True], ids=["open", "land"])
@pytest.mark.parametrize("metrics", list(GRIDS))
def test_pieces_reassemble_into_the_tendency_bitwise(metrics, land, viscous, oracle_lib):
    """Stresses without an implicit part (a number on top, arrays below): the restatement's pieces, put together in the reference's
    order, ARE Ref.tendency, bit for bit; the EVP pseudo-time term of sum_of_forcing_* is added from u^n and alpha as the tendency does."""
    c, p = problem(metrics, land, bottom="arrays")
    r = Ref(p, nu=1000.0, viscous=viscous)
    t = ref.TermsRef(p, rheology="viscous" if viscous else "evp")
    u, v, f = p.f["u"], p.f["v"], p.f
    dt, seen = 60.0, 0
    for comp in ("u", "v"):
        for (i, j) in points(p, comp):
            G, mi, ai = r.tendency(comp, u, v, i, j, dt)
            q = t.pieces(comp, i, j)
            assert q["mi"] == mi and q["ai"] == ai
            if mi <= 0:
                continue
            extra = 0.0
            if not viscous:
                a0 = (i - 1, j) if comp == "u" else (i, j - 1)
                abar = (r.at(f["alpha"], *a0) + r.at(f["alpha"], i, j)) / 2
                own, n = (u, f["un"]) if comp == "u" else (v, f["vn"])
                extra = (r.at(n, i, j) - r.at(own, i, j)) / dt / abar
            got = ref.reassembled(q, extra_forcing=extra)
            assert np.float64(got).tobytes() == np.float64(G).tobytes(), (comp, i, j, got, G)
            seen += 1
    assert seen > 100


@pytest.mark.parametrize("stresses", ["explicit", "semi_implicit"])
@pytest.mark.parametrize("land", [False, True], ids=["open", "land"])
@pytest.mark.parametrize("metrics", list(GRIDS))
def test_slot_values_sum_to_the_tendency_within_the_rounding_bound(metrics, land, stresses, oracle_lib):
    """m_i G = the sum of the five slot values, to 32 * 2^-53 * sum |F_k| / m_i: fewer than sixteen roundings (two per term for the
    scaling by m_i or a_i and back, five additions, the division) each act on a quantity bounded by sum |F_k| / m_i; doubled for margin.
    With a SemiImplicitStress (wind drag from arrays on top, the ocean below) the slots hold TOTAL stresses: the explicit part the
    tendency takes is total + coef * u."""
    kw = dict(bottom="arrays") if stresses == "explicit" else dict(wind_drag="arrays")
    c, p = problem(metrics, land, **kw)
    p.f["un"][...] = p.f["u"]               # no pseudo-time term: it is not one of the five
    p.f["vn"][...] = p.f["v"]
    r = Ref(p, viscous=False)
    t = ref.TermsRef(p, rheology="evp")
    u, v = p.f["u"], p.f["v"]
    worst = 0.0
    for comp in ("u", "v"):
        for (i, j) in points(p, comp):
            F = t.point(comp, i, j)
            G, mi, ai = r.tendency(comp, u, v, i, j, 60.0)
            if mi <= 0 or r.peripheral(comp, i, j):
                assert all(x == 0.0 for x in F)
                continue
            own = r.at(u if comp == "u" else v, i, j)
            coef = (r.implicit_tau(p.s.top, comp, u, v, i, j), r.implicit_tau(p.s.bottom, comp, u, v, i, j))
            # TOP = -(a_i tau_top), BOTTOM = a_i tau_bottom with total stresses; the tendency's explicit parts add coef * u * a_i
            total = F[0] + (F[1] - ai * (coef[0] * own)) + (F[2] + ai * (coef[1] * own)) + F[3] + F[4]
            bound = 32 * 2.0 ** -53 * sum(abs(x) for x in F) / mi
            worst = max(worst, abs(total / mi - G) / bound)
            assert abs(total / mi - G) <= bound, (comp, i, j, total / mi, G, bound)
    print(metrics, land, stresses, "worst |sum F / m - G| / bound", worst)


# ---- 2. the Coriolis power ------------------------------------------------------------------------------------------------------------
def coriolis_case():
    c = cases.make_case(Nx=37, Ny=29, topo=("periodic", "periodic"), random_uv=0.1, patches=False, noise=0.0, top=None, bottom=None)
    p = cases.oracle_problem(c)
    p.interior("h")[...] = 1.25
    p.interior("aice")[...] = 0.75
    p.update_state()
    return p


def test_coriolis_power_vanishes_on_a_uniform_periodic_f_plane(oracle_lib):
    """sum u F_x Az + v F_y Az = 0 for F = m f (v-bar, -u-bar): every pair (u point, v point) enters both sums with weight 1/4.  Bound
    (2 n + 8) * 2^-53 * sum |summand|: n - 1 additions of the sum, n roundings shared by each summand's own products and averages (at
    most eight per summand, of relative size 2^-53), as stated in the issue.  A swapped sign in one component misses it by orders of
    magnitude."""
    p = coriolis_case()
    t = ref.TermsRef(p, rheology=None)
    f = t.fields(extent=False)
    assert np.abs(f["coriolis_x"]).max() > 0 and all(np.all(f[k] == 0.0) for k in f if not k.startswith("coriolis"))
    r, u, v = t.r, p.f["u"], p.f["v"]
    az = p.s.dx * p.s.dy
    ui, vi = p.interior("u"), p.interior("v")
    px, py = (ui * f["coriolis_x"]) * az, (vi * f["coriolis_y"]) * az
    n = px.size
    bound = (2 * n + 8) * 2.0 ** -53 * math.fsum(np.abs(px).ravel().tolist() + np.abs(py).ravel().tolist())
    got = t.budget(f)["coriolis"]
    assert dref.same_bits(got, dref.ordered_sum(px + py))
    wrong = dict(f, coriolis_y=-f["coriolis_y"])
    bad = t.budget(wrong)["coriolis"]
    print("coriolis power", got, "bound", bound, "with a swapped sign", bad)
    assert abs(got) <= bound
    assert abs(bad) > 1e6 * bound


# ---- 3. the drag against an ocean at rest -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metrics", list(GRIDS))
def test_bottom_drag_opposes_the_motion_when_the_ocean_is_at_rest(metrics, oracle_lib):
    c, p = problem(metrics, True)             # bottom: SemiImplicitStress with u_e = v_e = 0
    assert p.s.bottom.kind == 3 and p.s.bottom.ue_kind == 0 and p.s.bottom.ve_kind == 0
    t = ref.TermsRef(p)
    f = t.fields()
    ui, vi = p.interior("u"), p.interior("v")
    assert np.all(ui * f["bottom_x"] <= 0.0) and np.all(vi * f["bottom_y"] <= 0.0)
    assert (ui * f["bottom_x"]).min() < 0.0
    raw = t.fields(raw=True)                  # the interface stress itself: the same sign, without a_i
    assert np.all(ui * raw["bottom_x"] <= 0.0) and np.all(np.sign(raw["bottom_x"]) == np.sign(f["bottom_x"]))
    assert t.budget(f)["bottom"] < 0.0


# ---- 4. the internal power is the energy budget's internal_work -------------------------------------------------------------------------
@pytest.mark.parametrize("metrics", list(GRIDS))
def test_internal_power_equals_the_energy_budget_restatement(metrics, oracle_lib):
    """On unmasked grids with ice everywhere and u = 0 on the walls the summands are those of tests/derived_ref.py's internal_work, so
    the ordered sum lies within that test's bound of its math.fsum: (n - 1) 2^-53 sum |x_i|."""
    c = cases.make_case(Nx=37, Ny=29, topo=("periodic", "bounded"), random_uv=0.03, patches=False, **GRIDS[metrics])
    p = cases.oracle_problem(c)
    rng = np.random.default_rng(3)
    for k, s in (("s11", 50.0), ("s22", 50.0), ("s12", 30.0)):
        p.f[k][...] = s * rng.standard_normal(p.f[k].shape)
    t = ref.TermsRef(p)
    par = {"u": p.f["u"], "v": p.f["v"], "s11": p.f["s11"], "s22": p.f["s22"], "s12": p.f["s12"]}
    work = derived_ref.Ref(c["g"], par).terms(("internal_work",))["internal_work"]
    exact, bound = dref.fsum_bound(work)
    got = t.budget()["internal"]
    print(metrics, "internal power", got, "internal_work (fsum)", exact, "difference", got - exact, "bound", bound)
    assert abs(exact) > 0 and abs(got - exact) <= bound
    assert derived_ref.same_bits(t.power_terms()["internal"], work)


# ---- 5. the sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("land", [False, True], ids=["open", "land"])
def test_ordered_sums_within_the_worst_case_bound_of_fsum(land, oracle_lib):
    c, p = problem("curvilinear", land, wind_drag="arrays")
    t = ref.TermsRef(p)
    terms = t.power_terms()
    for name, x in terms.items():
        exact, bound = dref.fsum_bound(x)
        got = dref.ordered_sum(x)
        print(name, "ordered", got, "fsum", exact, "difference", got - exact, "bound", bound)
        assert np.abs(x).max() > 0 and abs(got - exact) <= bound, name


# ---- 6. layouts ---------------------------------------------------------------------------------------------------------------------------
MEMBERS = ["what", "reserved", "coriolis", "top", "bottom", "internal", "forcing"]


def _c_layout(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    exe = tmp_path / "momentum_terms_layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "momentum_terms_layout.c"), "-o", str(exe)])
    return {k: int(v) for k, v in (ln.split("=") for ln in subprocess.check_output([str(exe)]).decode().split())}


def test_c_compiler_layout_matches_ctypes(tmp_path):
    got = _c_layout(tmp_path)
    T = L.MomentumBudget
    assert [f[0] for f in T._fields_] == MEMBERS
    assert C.sizeof(T) == got["sizeof"] == 8 + 5 * 8
    for f in MEMBERS:
        assert getattr(T, f).offset == got["offset_" + f], f
    # every older id and count keeps its value; the term slots follow the derived ones: 48 .. 57, count 58, version 100
    assert got["CSI_VERSION"] == 100 and got["CSI_F_COUNT"] == len(L.FIELD_IDS) and got["CSI_F_COUNT_TOTAL"] == len(L.F) == 41
    assert got["CSI_F_COUNT_DERIVED"] == 48 == got["CSI_F_D_STRESS_POWER"] + 1 and got["sizeof_budget"] == C.sizeof(L.Budget) == 32
    assert L.MOMENTUM_TERM_FIELD_IDS == ["M_" + n.upper() for n in ref.FIELDS]
    for k, n in enumerate(ref.FIELDS):
        assert got["CSI_F_M_" + n.upper()] == L.F_MOMENTUM_TERMS["M_" + n.upper()] == L.slot_id("M_" + n.upper()) == 48 + k
    assert got["CSI_F_COUNT_BINDABLE"] == L.F_COUNT_BINDABLE == 58
    for k, n in enumerate(ref.TERMS):
        assert got["CSI_MTERM_" + n.upper()] == getattr(L, "MTERM_" + n.upper()) == 1 << k
    assert got["CSI_MTERM_ALL"] == L.MTERM_ALL == 31 and got["CSI_MTERM_RAW_STRESS"] == L.MTERM_RAW_STRESS == 32
    assert (got["CSI_MBUDGET_EXTERNAL"], got["CSI_MBUDGET_BODY"], got["CSI_MBUDGET_INTERNAL"], got["CSI_MBUDGET_ALL"]) == \
        (L.MBUDGET_EXTERNAL, L.MBUDGET_BODY, L.MBUDGET_INTERNAL, L.MBUDGET_ALL) == (1, 2, 4, 7)
    assert got["terms_result_bytes"] == got["budget_result_bytes"] == got["stats_result_bytes"] == 4


def test_c_compiler_layout_matches_julia_stub(tmp_path):
    got = _c_layout(tmp_path)
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    m = re.search(r"^struct\s+CsiMomentumBudget\b[^\n]*\n(.*?)\nend", stub, re.S | re.M)
    assert m, "struct CsiMomentumBudget is missing from the Julia stub"
    fields = re.findall(r"([A-Za-z_]\w*)::(\w+)", re.sub(r"#[^\n]*", "", m.group(1)))
    size_of = {"Cdouble": 8, "Float64": 8, "Int32": 4, "Cint": 4, "Int64": 8}
    off, offsets = 0, {}
    for name, t in fields:
        s = size_of[t]
        off = (off + s - 1) // s * s
        offsets[name] = off
        off += s
    assert list(offsets) == MEMBERS
    assert offsets == {f: got["offset_" + f] for f in MEMBERS} and (off + 7) // 8 * 8 == got["sizeof"]
    assert re.search(r"ccall\(\(:csi_momentum_budget_compute, libcsi\), Int32, \(Ptr\{Cvoid\}, Int32, Ptr\{CsiMomentumBudget\}\)", stub)
    assert re.search(r"ccall\(\(:csi_momentum_terms_compute, libcsi\), Int32, \(Ptr\{Cvoid\}, Int32\)", stub)
    assert re.search(r"function momentum_terms!\(model::HIPSeaIceModel, terms::Symbol\.\.\.", stub)
    assert re.search(r"function momentum_budget\(model::HIPSeaIceModel", stub)
    slots = dict(re.findall(r"(\w+)=(\d+)", re.search(r"const MOMENTUM_TERMS = \(([^)]*)\)", stub).group(1)))
    assert {k: int(v) for k, v in slots.items()} == {n: got["CSI_F_M_" + n.upper()] for n in csi.TERM_FIELD_NAMES}
    bits = dict(re.findall(r"(\w+)=(\d+)", re.search(r"const MOMENTUM_TERM_BITS = \(([^)]*)\)", stub).group(1)))
    assert {k: int(v) for k, v in bits.items()} == {n: got["CSI_MTERM_" + n.upper()] for n in csi.MOMENTUM_TERMS}


def test_library_exports_the_entry_points_and_the_header_states_the_contract():
    lib = L.load()
    for name, nargs in (("csi_momentum_terms_compute", 2), ("csi_momentum_budget_compute", 3), ("csi_momentum_terms_stats", 3)):
        assert len(getattr(lib, name).argtypes) == nargs and name in L.SYMBOLS
    text = open(os.path.join(ROOT, "include", "csi.h")).read()
    sec = text[text.index("momentum balance terms, interface stresses and their power"):text.index("int32_t csi_momentum_terms_stats")]
    for needle in ("HALO ELEMENTS READ", "ONE launch", "ONE RING", "SUMMATION ORDER", "COLLECTIVE", "rank order", "m_i <= 0", "peripheral",
                   "CSI_F_M_CORIOLIS_X = CSI_F_COUNT_DERIVED", "x_momentum_stress", "function of (Nx, Ny) alone", "NaN"):
        assert needle in sec, needle


# ---- 7. front end -------------------------------------------------------------------------------------------------------------------------
def test_front_end_names_and_argument_errors():
    from climaseaice_jl_amd import momentum_terms as M
    assert M.MOMENTUM_TERMS == ref.TERMS == csi.MOMENTUM_TERMS and M.TERM_FIELD_NAMES == ref.FIELDS == csi.TERM_FIELD_NAMES
    assert [M.slot_of(n) for n in M.TERM_FIELD_NAMES] == L.MOMENTUM_TERM_FIELD_IDS
    assert M.location_of("top_x") == (csi.Face, csi.Center) and M.location_of("internal_y") == (csi.Center, csi.Face)
    assert M.expand(("top", "forcing_y")) == ["top_x", "top_y", "forcing_y"]
    assert M.mask_of(("top",)) == 2 and M.mask_of(("top_x",)) == 2 and M.mask_of(M.MOMENTUM_TERMS) == 31
    assert M.mask_of(("bottom_y", "coriolis", "bottom_x")) == 1 | 4 and M.terms_of(5) == ("coriolis", "bottom")
    assert M.name_of_slot("M_INTERNAL_Y") == "internal_y" and M.name_of_slot("top_x") == "top_x" and M.name_of_slot("H") is None
    assert M.name_of_slot("top_u") is None                    # the wind stress array's slot is not a term field
    with pytest.raises(ValueError, match="coriolis_x, coriolis_y, top_x"):
        M.mask_of(("inertia",))
    with pytest.raises(ValueError, match="at least one"):
        M.mask_of(())
    assert [M._what_mask(w) for w in ("all", "external", "body", "internal", ("external", "internal"))] == [7, 1, 2, 4, 5]
    with pytest.raises(ValueError, match="'all', 'external', 'body' or 'internal'"):
        M._what_mask("kinetic")
    with pytest.raises(ValueError, match="'top' or 'bottom'"):
        M.interface_stress(None, "east")
    b = M.MomentumBudget(what=("body",), coriolis=0.0, forcing=1.0)
    assert b.top is None and b.residual is None
    with pytest.raises(Exception):
        b.forcing = 2.0                                           # immutable
    for name in ("momentum_term", "compute_momentum_terms", "interface_stress", "momentum_budget"):
        assert hasattr(csi.SeaIceModel, name), name

    class Ctx:                                                  # the record's members by group, the residual only with all five
        def momentum_budget_compute(self, mask):
            nan = math.nan
            return SimpleNamespace(coriolis=1.0 if mask & 2 else nan, forcing=0.5 if mask & 2 else nan, top=4.0 if mask & 1 else nan,
                                   bottom=-3.0 if mask & 1 else nan, internal=-2.0 if mask & 4 else nan)
    fake = SimpleNamespace(ctx=Ctx())
    b = M.momentum_budget(fake)
    assert b.what == ("external", "body", "internal") and b.residual == 0.5 and (b.top, b.bottom, b.internal) == (4.0, -3.0, -2.0)
    b = M.momentum_budget(fake, "external")
    assert b.what == ("external",) and b.coriolis is None and b.internal is None and b.residual is None and b.bottom == -3.0


class StandInModel:
    """What tests/output_ref.py RefRecorder needs (.grid, .fields) plus the two methods the writer's hook calls; compute_momentum_terms
    writes a value that depends on the clock, so a record shows WHEN it ran."""

    def __init__(self):
        self.grid = csi.RectilinearGrid((6, 4), x=(0, 6), y=(0, 4), topology=(csi.Periodic, csi.Bounded), halo=(2, 2))
        self.clock = SimpleNamespace(time=0.0, iteration=0)
        self.fields = {"h": csi.CenterField(self.grid, "cpu", "h")}
        self.fields["h"].data.fill_(1.5)
        self.calls = []

    def momentum_term(self, name):
        from climaseaice_jl_amd.momentum_terms import location_of
        if name not in self.fields:
            self.fields[name] = csi.Field(location_of(name), self.grid, "cpu", name)
        return self.fields[name]

    def compute_momentum_terms(self, *names):
        self.calls.append((self.clock.iteration, names))
        for k, n in enumerate(names):
            self.fields[n].data.fill_(10.0 * self.clock.iteration + k + 1)

    def step(self, writer, dt):
        self.clock.time += dt
        self.clock.iteration += 1
        writer.after_step(self, dt)


def test_writer_hook_on_the_stand_in_recorder(tmp_path):
    """Term field names in a writer's list: allocated at construction, computed immediately before every snapshot and every accumulate
    -- and never for a writer without them.  A _y field on a Bounded y direction has its extra face row in the record."""
    m = StandInModel()
    with csi.OutputWriter(m, ["h", "bottom_x", "bottom_y"], csi.IterationInterval(2), str(tmp_path / "snap"), dtype="f64",
                          recorder=output_ref.RefRecorder) as w:
        assert w.momentum_terms == ("bottom_x", "bottom_y") and w.derived == () and set(m.fields) == {"h", "bottom_x", "bottom_y"}
        w.begin(m)
        for _ in range(4):
            m.step(w, 10.0)
    assert m.calls == [(0, ("bottom_x", "bottom_y")), (2, ("bottom_x", "bottom_y")), (4, ("bottom_x", "bottom_y"))]
    got = csi.load_output(str(tmp_path / "snap"))
    assert list(got["iteration"]) == [0, 2, 4] and got["bottom_x"].shape[1:] == (4, 6) and got["bottom_y"].shape[1:] == (5, 6)
    for r, it in enumerate((0, 2, 4)):
        assert np.all(got["bottom_x"][r] == 10.0 * it + 1) and np.all(got["bottom_y"][r] == 10.0 * it + 2) and np.all(got["h"][r] == 1.5)
    m = StandInModel()
    with csi.OutputWriter(m, ["top_x", "h"], csi.AveragedTimeInterval(20.0), str(tmp_path / "avg"), dtype="f64",
                          recorder=output_ref.RefRecorder) as w:
        w.begin(m)
        for _ in range(4):
            m.step(w, 10.0)
    assert [it for it, _ in m.calls] == [1, 2, 2, 3, 4, 4] and all(n == ("top_x",) for _, n in m.calls)
    got = csi.load_output(str(tmp_path / "avg"))
    assert np.all(got["top_x"][0] == (11.0 * 10.0 + 21.0 * 10.0) / 20.0) and np.all(got["top_x"][1] == (31.0 * 10.0 + 41.0 * 10.0) / 20.0)
    m = StandInModel()
    with csi.OutputWriter(m, ["h"], csi.IterationInterval(1), str(tmp_path / "plain"), dtype="f64", recorder=output_ref.RefRecorder) as w:
        assert w.momentum_terms == ()
        w.begin(m)
        m.step(w, 10.0)
    assert m.calls == [] and set(m.fields) == {"h"}
    with pytest.raises(ValueError, match="'inertia_x'"):
        csi.OutputWriter(m, ["h", "inertia_x"], csi.IterationInterval(1), str(tmp_path / "bad"), recorder=output_ref.RefRecorder)
