"""CPU tests of the definition of the derived fields and the energy budget integrals (include/csi.h): the NumPy restatement
(tests/derived_ref.py) against the CPU oracle's strain rates and stress divergence bit for bit, its sums against math.fsum within the
order-independent worst-case bound, the reference's adjoint identity and its ability to fail, the layout of csi_budget as gcc, ctypes and
the Julia stub see it, and the output writer's hook on the stand-in recorder of tests/output_ref.py."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import climaseaice_jl_amd as csi
import derived_ref as ref
import diagnostics_ref as dref
import oracle as O
import output_ref

L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORA_NAME = {"u": "u", "v": "v", "s11": "s11", "s22": "s22", "s12": "s12", "P": "P", "h": "h", "a": "aice"}


def oracle_of(g, par, topo, mask):
    """An oracle problem on grid g whose parent arrays hold `par` as they are (no fill, no update_state!)."""
    code = tuple(O.PERIODIC if t == "periodic" else O.BOUNDED for t in topo)
    m = g.metrics()
    kw = dict(dx=m["dx"], dy=m["dy"]) if m["kind"] == "uniform" else (dict(full=m) if m["kind"] == "full" else dict(per_j=m))
    p = O.Problem(g.Nx, g.Ny, g.Hx, g.Hy, code, **kw)
    for k, name in ORA_NAME.items():
        assert p.f[name].shape == par[k].shape, (k, p.f[name].shape, par[k].shape)
        p.f[name][...] = par[k]
    if mask is not None:
        p.set_mask(mask)
    return p


def over_cells(p, fn):
    f = getattr(p.L, fn)
    return np.array([[f(p.ptr, i, j) for i in range(1, p.s.Nx + 1)] for j in range(1, p.s.Ny + 1)])


# ---- the restatement's operators are the oracle's, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("land", [False, True], ids=["open", "land"])
@pytest.mark.parametrize("metrics,topo", [("uniform", "periodic"), ("latlon", "bounded"), ("curvilinear", "channel"),
                                          ("curvilinear", "bounded"), ("latlon", "periodic"), ("uniform", "channel")])
def test_strain_rates_and_stress_divergence_equal_the_oracle_bitwise(metrics, topo, land, oracle_lib):
    """e11, e22, e12 and d_j sigma_1j, d_j sigma_2j of the restatement == ora_strain_* / ora_div_sigma_* at every interior point, on
    white noise whose halos are noise too, with the immersed conditionals of the divergence where there is land."""
    g = ref.grid_of(37, 29, ref.TOPOS[topo], metrics)
    par, wet = ref.white_noise(g, seed=5, land=land)
    mask = ref.mask_parent(g, wet)
    p = oracle_of(g, par, ref.TOPOS[topo], mask)
    r = ref.Ref(g, par, mask)
    for fn, got in (("ora_strain_xx", r.e11()), ("ora_strain_yy", r.e22()), ("ora_strain_xy", r.e12()),
                    ("ora_div_sigma_1", r.div_sigma_1()), ("ora_div_sigma_2", r.div_sigma_2()),
                    ("ora_old_div_sigma_1", r.old_div_sigma()[0]), ("ora_old_div_sigma_2", r.old_div_sigma()[1])):
        want = over_cells(p, fn)
        assert ref.same_bits(got, want), (fn, metrics, topo, land, np.abs(got - want).max())
    if land:                                 # the conditionals matter: without them the divergence differs next to land
        bare = ref.Ref(g, par, None)
        assert not ref.same_bits(bare.div_sigma_1(), r.div_sigma_1())


def test_fields_on_hand_worked_values():
    """Uniform grid, u = a x, v = b y: divergence a + b, shear |a - b|, no e12; speed at the centre; P == 0 gives +0.0."""
    g = csi.RectilinearGrid((6, 5), x=(0.0, 6.0), y=(0.0, 5.0), topology=(csi.Periodic, csi.Periodic), halo=(2, 2))
    a, b = 0.25, -0.5
    iu = np.arange(1 - 2, 6 + 2 + 1) - 1.0            # x of the u faces, i = 1 - H .. Nx + H
    jv = np.arange(1 - 2, 5 + 2 + 1) - 1.0
    par = {"u": np.broadcast_to(a * iu[None, :], (9, 10)).copy(), "v": np.broadcast_to(b * jv[:, None], (9, 10)).copy(),
           "s11": np.full((9, 10), 3.0), "s22": np.full((9, 10), 1.0), "s12": np.full((9, 10), 2.0), "P": np.full((9, 10), 4.0)}
    par["P"][2 + 1, 2 + 2] = 0.0
    f = ref.Ref(g, par).fields()
    assert np.all(f["divergence"] == a + b) and np.all(f["shear"] == abs(a - b))
    assert np.all(f["deformation"] == math.sqrt((a + b) ** 2 + (a - b) ** 2))
    uc, vc = a * (np.arange(6) + 0.5), b * (np.arange(5) + 0.5)
    assert np.array_equal(f["speed"], np.sqrt(uc[None, :] ** 2 + vc[:, None] ** 2))
    sI, sII = np.full((5, 6), 0.5), np.full((5, 6), math.sqrt(1.0 + 4.0) / 4.0)
    sI[1, 2] = sII[1, 2] = 0.0
    assert np.array_equal(f["sigma_I"], sI) and np.array_equal(f["sigma_II"], sII)
    assert not np.signbit(f["sigma_I"][1, 2]) and not np.signbit(f["sigma_II"][1, 2])
    assert np.all(f["stress_power"] == 3.0 * a + 1.0 * b)
    wet = np.ones((5, 6), dtype=bool)
    wet[3, 4] = False
    fm = ref.Ref(g, par, ref.mask_parent(g, wet)).fields()
    for n in ref.NAMES:
        assert fm[n][3, 4] == 0.0 and not np.signbit(fm[n][3, 4]) and np.array_equal(np.delete(fm[n].ravel(), 3 * 6 + 4), np.delete(f[n].ravel(), 3 * 6 + 4))


# ---- the sums --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 29), (130, 33), (65, 65)])
@pytest.mark.parametrize("metrics,topo,land", [("latlon", "bounded", True), ("curvilinear", "periodic", False), ("uniform", "channel", True)])
def test_ordered_sums_within_the_worst_case_bound_of_fsum(shape, metrics, topo, land):
    g = ref.grid_of(*shape, ref.TOPOS[topo], metrics)
    par, wet = ref.white_noise(g, seed=9, land=land)
    r = ref.Ref(g, par, ref.mask_parent(g, wet))
    for name, t in r.terms().items():
        exact, bound = dref.fsum_bound(t)
        got = dref.ordered_sum(t)
        print(name, shape, metrics, "ordered", got, "fsum", exact, "difference", got - exact, "bound", bound)
        assert abs(got - exact) <= bound, (name, got, exact, bound)
    assert r.budget()["kinetic_energy"] > 0.0


# the grids of the identity: unmasked, fields that vanish on and beyond the walls (the reference test's two-cell margin) or are periodic
IDENTITY = {"latlon_bounded_40": ((40, 40), "bounded", "latlon"), "rectilinear_periodic": ((37, 29), "periodic", "uniform"),
            "curvilinear_periodic": ((37, 29), "periodic", "distorted_rectilinear"), "latlon_channel": ((64, 33), "channel", "latlon")}


def identity_case(name, seed=21):
    shape, topo, metrics = IDENTITY[name]
    g = ref.grid_of(*shape, ref.TOPOS[topo], metrics)
    par, _ = ref.white_noise(g, seed=seed, margin=2, zero_P=False, unit=True)
    return g, par


@pytest.mark.parametrize("name", list(IDENTITY))
def test_energy_identity_on_unmasked_grids(name):
    """sum (u d_j sigma_1j Az^fc + v d_j sigma_2j Az^cf) = - sum sigma : eps Az to the reference's own bound, 1e-10
    (test/test_rheology_energy_budget.jl:117), with white-noise u, v, sigma."""
    g, par = identity_case(name)
    b = ref.Ref(g, par).budget(("internal_work", "stress_power"))
    imb = ref.imbalance(b["internal_work"], b["stress_power"])
    print(name, "W", b["internal_work"], "D", b["stress_power"], "imbalance", imb)
    assert abs(b["stress_power"]) > 0.0
    assert imb < 1e-10


def test_the_identity_can_fail(oracle_lib):
    """With the flux-form operator the reference keeps for contrast the lat-lon 40 x 40 case does NOT close: > 1e-3, as the reference
    asserts (:120).  The terms come from the oracle's ora_old_div_sigma_*."""
    g, par = identity_case("latlon_bounded_40")
    p = oracle_of(g, par, ref.TOPOS["bounded"], None)
    r = ref.Ref(g, par)
    d1, d2 = over_cells(p, "ora_old_div_sigma_1"), over_cells(p, "ora_old_div_sigma_2")
    W = dref.ordered_sum((r.at("u") * d1) * r.metric("az", "f", "c") + (r.at("v") * d2) * r.metric("az", "c", "f"))
    D = r.budget(("stress_power",))["stress_power"]
    good = r.budget(("internal_work",))["internal_work"]
    print("old operator: W", W, "D", D, "imbalance", ref.imbalance(W, D), "new", ref.imbalance(good, D))
    assert ref.imbalance(W, D) > 1e-3
    assert ref.same_bits(r.budget(("internal_work",), old=True)["internal_work"], W)


def test_a_dropped_or_doubled_cell_shows_in_the_sums():
    g, par = identity_case("rectilinear_periodic")
    r = ref.Ref(g, par)
    for name, t in r.terms(("internal_work", "stress_power")).items():
        _, bound = dref.fsum_bound(t)
        good = dref.ordered_sum(t)
        dropped = t.copy()
        j, i = np.unravel_index(np.argmax(np.abs(t)), t.shape)
        dropped[j, i] = 0.0
        assert abs(dref.ordered_sum(dropped) - good) > bound, name


# ---- ABI: header, ctypes mirror, Julia stub ------------------------------------------------------------------------------------------------
FIELDS = ["what", "reserved", "internal_work", "stress_power", "kinetic_energy"]


def _c_layout(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    exe = tmp_path / "budget_layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "budget_layout.c"), "-o", str(exe)])
    return {k: int(v) for k, v in (ln.split("=") for ln in subprocess.check_output([str(exe)]).decode().split())}


def test_c_compiler_layout_matches_ctypes(tmp_path):
    got = _c_layout(tmp_path)
    T = L.Budget
    assert [f[0] for f in T._fields_] == FIELDS
    assert C.sizeof(T) == got["sizeof"] == 8 + 3 * 8
    for f in FIELDS:
        assert getattr(T, f).offset == got["offset_" + f], f
    # every older id and count keeps its value; the derived slots follow CSI_F_FREE_DRIFT_V
    assert got["CSI_VERSION"] == 100 and got["CSI_F_COUNT"] == len(L.FIELD_IDS) and got["CSI_F_COUNT_TOTAL"] == len(L.F) == 41
    assert got["CSI_F_D_DIVERGENCE"] == got["CSI_F_FREE_DRIFT_V"] + 1 == got["CSI_F_COUNT_TOTAL"]
    names = ["DIVERGENCE", "SHEAR", "DEFORMATION", "SPEED", "SIGMA_I", "SIGMA_II", "STRESS_POWER"]
    assert L.DERIVED_FIELD_IDS == ["D_" + n for n in names]
    for k, n in enumerate(names):
        assert got["CSI_F_D_" + n] == L.F_DERIVED["D_" + n] == L.slot_id("D_" + n) == 41 + k
        assert got["CSI_DERIVED_" + n] == 1 << k
    assert got["CSI_F_COUNT_DERIVED"] == 48 and got["CSI_DERIVED_ALL"] == L.DERIVED_ALL == 127
    assert (got["CSI_BUDGET_STRESS"], got["CSI_BUDGET_KINETIC"], got["CSI_BUDGET_ALL"]) == (L.BUDGET_STRESS, L.BUDGET_KINETIC, L.BUDGET_ALL) == (1, 2, 3)
    assert got["sizeof_diagnostics"] == C.sizeof(L.Diagnostics)                  # csi_diagnostics is untouched
    assert got["derived_result_bytes"] == got["budget_result_bytes"] == got["stats_result_bytes"] == 4


def test_c_compiler_layout_matches_julia_stub(tmp_path):
    got = _c_layout(tmp_path)
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    m = re.search(r"^struct\s+CsiBudget\b[^\n]*\n(.*?)\nend", stub, re.S | re.M)
    assert m, "struct CsiBudget is missing from the Julia stub"
    fields = re.findall(r"([A-Za-z_]\w*)::(\w+)", re.sub(r"#[^\n]*", "", m.group(1)))
    size_of = {"Cdouble": 8, "Float64": 8, "Int32": 4, "Cint": 4, "Int64": 8}
    off, offsets = 0, {}
    for name, t in fields:
        s = size_of[t]
        off = (off + s - 1) // s * s
        offsets[name] = off
        off += s
    assert list(offsets) == FIELDS
    assert offsets == {f: got["offset_" + f] for f in FIELDS} and (off + 7) // 8 * 8 == got["sizeof"]
    assert re.search(r"ccall\(\(:csi_budget_compute, libcsi\), Int32, \(Ptr\{Cvoid\}, Int32, Ptr\{CsiBudget\}\)", stub)
    assert re.search(r"ccall\(\(:csi_derived_compute, libcsi\), Int32, \(Ptr\{Cvoid\}, Int32\)", stub)
    assert re.search(r"function derived!\(model::HIPSeaIceModel, names::Symbol\.\.\.\)", stub)
    assert re.search(r"function energy_budget\(model::HIPSeaIceModel", stub)
    slots = dict(re.findall(r"(\w+)=(\d+)", re.search(r"const DERIVED = \(([^)]*)\)", stub).group(1)))
    assert {k: int(v) for k, v in slots.items()} == {n: got["CSI_F_D_" + n.upper()] for n in csi.DERIVED_NAMES}


def test_library_exports_the_entry_points_and_the_header_states_the_contract():
    lib = L.load()
    for name, nargs in (("csi_derived_compute", 2), ("csi_budget_compute", 3), ("csi_derived_stats", 3)):
        assert len(getattr(lib, name).argtypes) == nargs and name in L.SYMBOLS
    text = open(os.path.join(ROOT, "include", "csi.h")).read()
    sec = text[text.index("derived fields and energy budget integrals"):text.index("int32_t csi_derived_stats")]
    for needle in ("HALO ELEMENTS READ", "ONE launch", "SUMMATION ORDER", "COLLECTIVE", "rank order", "Where P == 0 both are +0.0",
                   "CSI_F_D_DIVERGENCE = CSI_F_COUNT_TOTAL", "do_finalize"):
        assert needle in sec, needle


# ---- front end ----------------------------------------------------------------------------------------------------------------------------
def test_front_end_names_and_argument_errors():
    from climaseaice_jl_amd import derived as D
    assert D.DERIVED_NAMES == ref.NAMES == csi.DERIVED_NAMES
    assert [D.slot_of(n) for n in D.DERIVED_NAMES] == L.DERIVED_FIELD_IDS
    assert D.mask_of(("shear",)) == 2 and D.mask_of(D.DERIVED_NAMES) == 127 and D.mask_of(("speed", "sigma_II", "speed")) == 8 | 32
    assert D.name_of_slot("D_SIGMA_I") == "sigma_I" and D.name_of_slot("shear") == "shear" and D.name_of_slot("H") is None
    with pytest.raises(ValueError, match="divergence, shear"):
        D.mask_of(("vorticity",))
    with pytest.raises(ValueError, match="at least one"):
        D.mask_of(())
    assert (D._what_mask("all"), D._what_mask("stress"), D._what_mask("kinetic"), D._what_mask(("stress", "kinetic"))) == (3, 1, 2, 3)
    with pytest.raises(ValueError, match="'all', 'stress' or 'kinetic'"):
        D._what_mask("external")
    assert D.imbalance(2.0, -2.0) == 0.0 and D.imbalance(3.0, -1.0) == 2.0 / 3.0 and math.isnan(D.imbalance(0.0, 0.0))
    b = D.EnergyBudget(what=("stress",), internal_work=1.0, stress_power=-1.0, imbalance=0.0)
    with pytest.raises(Exception):
        b.internal_work = 2.0                                                    # immutable
    for name in ("derived_field", "compute_derived", "energy_budget"):
        assert hasattr(csi.SeaIceModel, name), name


class StandInModel:
    """What tests/output_ref.py RefRecorder needs (.grid, .fields) plus the two methods the writer's hook calls; compute_derived writes
    a value that depends on the clock, so a record shows WHEN it ran."""

    def __init__(self):
        self.grid = csi.RectilinearGrid((6, 4), x=(0, 6), y=(0, 4), topology=(csi.Periodic, csi.Bounded), halo=(2, 2))
        self.clock = SimpleNamespace(time=0.0, iteration=0)
        self.fields = {"h": csi.CenterField(self.grid, "cpu", "h")}
        self.fields["h"].data.fill_(1.5)
        self.calls = []

    def derived_field(self, name):
        if name not in self.fields:
            self.fields[name] = csi.CenterField(self.grid, "cpu", name)
        return self.fields[name]

    def compute_derived(self, *names):
        self.calls.append((self.clock.iteration, names))
        for k, n in enumerate(names):
            self.fields[n].data.fill_(10.0 * self.clock.iteration + k + 1)

    def step(self, writer, dt):
        self.clock.time += dt
        self.clock.iteration += 1
        writer.after_step(self, dt)


def test_writer_hook_on_the_stand_in_recorder(tmp_path):
    """Derived names in a writer's list: allocated at construction, computed immediately before every snapshot and every accumulate --
    and never for a writer without them."""
    m = StandInModel()
    with csi.OutputWriter(m, ["h", "shear", "divergence"], csi.IterationInterval(2), str(tmp_path / "snap"), dtype="f64",
                          recorder=output_ref.RefRecorder) as w:
        assert w.derived == ("shear", "divergence") and set(m.fields) == {"h", "shear", "divergence"}
        w.begin(m)
        for _ in range(4):
            m.step(w, 10.0)
    assert m.calls == [(0, ("shear", "divergence")), (2, ("shear", "divergence")), (4, ("shear", "divergence"))]
    got = csi.load_output(str(tmp_path / "snap"))
    assert list(got["iteration"]) == [0, 2, 4]
    for r, it in enumerate((0, 2, 4)):
        assert np.all(got["shear"][r] == 10.0 * it + 1) and np.all(got["divergence"][r] == 10.0 * it + 2) and np.all(got["h"][r] == 1.5)
    m = StandInModel()
    with csi.OutputWriter(m, ["shear", "h"], csi.AveragedTimeInterval(20.0), str(tmp_path / "avg"), dtype="f64",
                          recorder=output_ref.RefRecorder) as w:
        w.begin(m)
        for _ in range(4):
            m.step(w, 10.0)
    # steps 1 .. 4: an accumulate each; a record (one more computation) at the end of steps 2 and 4
    assert [it for it, _ in m.calls] == [1, 2, 2, 3, 4, 4] and all(n == ("shear",) for _, n in m.calls)
    got = csi.load_output(str(tmp_path / "avg"))
    assert np.all(got["shear"][0] == (11.0 * 10.0 + 21.0 * 10.0) / 20.0) and np.all(got["shear"][1] == (31.0 * 10.0 + 41.0 * 10.0) / 20.0)
    m = StandInModel()
    with csi.OutputWriter(m, ["h"], csi.IterationInterval(1), str(tmp_path / "plain"), dtype="f64", recorder=output_ref.RefRecorder) as w:
        assert w.derived == ()
        w.begin(m)
        m.step(w, 10.0)
    assert m.calls == [] and set(m.fields) == {"h"}
    with pytest.raises(ValueError, match="'vorticity'"):
        csi.OutputWriter(m, ["h", "vorticity"], csi.IterationInterval(1), str(tmp_path / "bad"), recorder=output_ref.RefRecorder)
