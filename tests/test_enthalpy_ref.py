"""CPU tests of the enthalpy-method column model's definition (include/csi.h, "enthalpy-method column model"): properties of the NumPy
restatement (tests/enthalpy_ref.py), that the mistakes the header warns of are visible, the choosing rule of the library against
tests/enthalpy_layouts.py, the layouts as gcc, ctypes and the Julia stub see them, and the front end's argument errors.  Nothing here
needs a GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import climaseaice_jl_amd as csi
import enthalpy_layouts as lay
import enthalpy_ref as ref
import time_series_ref as tsr

L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stretched_faces(Nz=12):
    k = np.arange(Nz + 1)
    return -2.0 + 2.0 * (k / Nz) ** 1.7


# ---- properties of the restatement --------------------------------------------------------------------------------------------------

def test_uniform_temperature_with_no_flux_sides_stays_bit_identical():
    for zf in (ref.uniform_faces(-1.0, 0.0, 20), stretched_faces()):
        for T0 in (1.1, -3.25):
            m = ref.Model(3, 2, zf)
            m.set_T(T0)
            m.update_state()
            H0, T = m.H.copy(), m.T.copy()
            m.time_steps(10.0, 50)
            assert np.array_equal(m.H, H0) and np.array_equal(m.T, T)
            assert np.all(m.phi[1:-1] == (1.0 if T0 < 0 else 0.0))


def test_enthalpy_is_conserved_with_uniform_kappa_and_no_flux_sides():
    """sum H dzc changes only by rounding: the interior fluxes cancel in pairs and the boundary fluxes are exactly zero.  Bound: every
    step adds one rounding of each of the Nz terms' updates, |dH| <= eps * max|H|, so n steps move the sum by at most
    n * Nz * eps * max|H dzc| (plus the summation's own Nz * eps * sum|H dzc|, taken on both ends)."""
    rng = np.random.default_rng(5)
    zf = stretched_faces(16)
    m = ref.Model(2, 2, zf, kappa_ice=1e-5, kappa_water=1e-5)
    m.set_T(rng.uniform(-4.0, 2.0, (16, 2, 2)))
    m.update_state()
    assert np.all(m.kappa == 1e-5) and 0 < m.phi[1:-1].sum() < m.phi[1:-1].size
    total = lambda: (m.H[1:-1] * m.dzc[:, None, None]).sum(axis=0)      # noqa: E731
    s0, n = total(), 400
    dt = 0.1 * m.dzc.min() ** 2 / 1e-5
    m.time_steps(dt, n)
    scale = np.abs(m.H[1:-1] * m.dzc[:, None, None]).max()
    bound = (n + 2) * m.Nz * np.finfo(float).eps * scale
    print("conservation: max |d sum| =", np.abs(total() - s0).max(), "bound", bound)
    assert np.abs(total() - s0).max() <= bound
    assert np.all(np.isfinite(m.T)) and np.ptp(m.T[1:-1], axis=0).max() < 6.0      # (it did diffuse: the profile's range shrank)


def test_a_fresh_model_first_bare_step_changes_nothing():
    zf = ref.uniform_faces(-1.0, 0.0, 8)
    m = ref.Model(1, 1, zf, bottom=1.0, top=-5.0)
    m.set_T(np.linspace(1.0, -2.0, 8))
    assert np.all(m.kappa == 0.0) and np.all(m.phi == 0.0)
    H0 = m.H.copy()
    m.time_step(5.0)                       # kappa = 0: G = 0; update_state runs behind it and fills kappa
    assert np.array_equal(m.H, H0) and m.time == 5.0
    assert np.any(m.kappa != 0.0)
    m2 = ref.Model(1, 1, zf, bottom=1.0, top=-5.0)
    m2.set_T(np.linspace(1.0, -2.0, 8))
    m2.update_state()
    m2.time_step(5.0)
    assert not np.array_equal(m2.H, H0)


def test_set_T_uses_the_porosity_held_now_and_set_H_fills_the_halos():
    zf = ref.uniform_faces(-1.0, 0.0, 4)
    m = ref.Model(1, 1, zf, bottom=0.5, top=-2.0)
    m.set_T(-1.0)
    assert np.all(m.H[1:-1] == m.c * -1.0)              # phi = 0 for a fresh model: no latent term
    m.update_state()
    assert np.all(m.phi[1:-1] == 1.0)
    m.set_T(-1.0)
    assert np.all(m.H[1:-1] == m.c * -1.0 + m.L * 1.0)
    m.set_H(np.array([4.0, 2.0, -2.0, -4.0]))
    assert m.T[0, 0, 0] == 2.0 * 0.5 - m.T[1, 0, 0] and m.T[-1, 0, 0] == 2.0 * -2.0 - m.T[-2, 0, 0]
    assert np.all(m.phi[1:-1] == 1.0)                   # untouched by set


def test_example_freezes_the_top_cell_at_step_two_and_keeps_both_phases():
    """Steps counted from 0, as the clock's iteration counts them when a step starts: steps 0 and 1 leave the top cell at 0.516 and
    0.0165 degrees, step 2 takes it to -0.412.  From then on the column holds both phases."""
    m, dt = ref.example_model(720)
    frozen_top = []
    for s in range(720):
        assert m.iteration == s
        m.time_step(dt)
        frozen_top.append(bool(m.phi[-2, 0, 0] == 1.0))
        if s >= 2:
            assert 0 < m.phi[1:-1].sum() < m.Nz, s
    assert frozen_top[:2] == [False, False] and all(frozen_top[2:])
    # frozen cells take kappa_water: the reference's assignment
    assert m.kappa[-2, 0, 0] == 1e-6 and m.kappa[1, 0, 0] == 1e-5


# ---- a mistake shows ----------------------------------------------------------------------------------------------------------------------

def test_mistakes_are_visible():
    """The three mistakes the header's wording guards against, each against the restatement: the distances are printed and must be
    far above rounding (1e-9 of the temperatures' scale would already be 1e7 ulp)."""
    good, dt = ref.example_model(720)
    good.time_steps(dt, 720)
    late, _ = ref.example_model(720, mistake="late_boundary")
    late.time_steps(dt, 720)
    d_late = np.abs(late.T[1:-1] - good.T[1:-1]).max()
    swap, _ = ref.example_model(720, mistake="swap_kappa")
    swap.time_steps(dt, 720)
    d_swap = np.abs(swap.T[1:-1] - good.T[1:-1]).max()
    zf = stretched_faces(12)
    step = 0.1 * np.diff(zf).min() ** 2 / 1e-5
    a, b = ref.Model(1, 1, zf, bottom=1.1, top=-5.0), ref.Model(1, 1, zf, bottom=1.1, top=-5.0, mistake="dzc_for_dzf")
    for m in (a, b):
        m.set_T(1.1)
        m.update_state()
        m.time_steps(step, 720)
    d_dz = np.abs(a.T[1:-1] - b.T[1:-1]).max()
    print(f"late boundary: {d_late:.3e}   swapped kappa: {d_swap:.3e}   dzc for dzf on a stretched grid: {d_dz:.3e}")
    # one step late shifts the top temperature by dt * |dTt/dt| <= 25 s * 3.7e-4 K/s = 9e-3 K, and the top cell follows its boundary
    # with a factor below one: between 1e-3 and 1e-2.  Measured: 1.83e-3 over the interior, 2.60e-3 with T's halo levels
    d_late_all = np.abs(late.T - good.T).max()
    print(f"late boundary, halo levels included: {d_late_all:.3e}")
    assert 1e-3 < d_late < 1e-2 and 2.5e-3 < d_late_all < 2.7e-3
    assert d_swap > 1e-3 and d_dz > 1e-3


def test_thickness_equals_the_examples_binary_search_on_monotone_profiles():
    rng = np.random.default_rng(11)
    zf = stretched_faces(14)
    m = ref.Model(5, 4, zf)
    prof = np.sort(rng.uniform(-6.0, 1.5, (14, 4, 5)), axis=0)[::-1]
    prof[0] = np.maximum(prof[0], 0.2)          # liquid at the bottom, frozen at the top: the search's precondition
    prof[-1] = np.minimum(prof[-1], -0.5)
    m.set_T(prof)
    h = m.ice_thickness(-0.1)
    for j in range(4):
        for i in range(5):
            assert h[j, i] == ref.example_thickness_binary_search(prof[:, j, i], m.zc, m.dzf, np.float64(-0.1))
    assert np.all((h > 0) & (h < 2.0))
    # total: wholly frozen, wholly liquid
    m.set_T(-3.0)
    assert np.all(m.ice_thickness() == 2.0)
    m.set_T(0.5)
    assert np.all(m.ice_thickness() == 0.0)


# ---- the choosing rule ------------------------------------------------------------------------------------------------------------------

def test_plan_matches_the_python_rule():
    for forced in (0, 1, 2):
        for Nz in range(1, 201):
            try:
                want = lay.plan(Nz, forced)
            except lay.Unsupported:
                with pytest.raises(csi.CsiError) as e:
                    L.enthalpy_plan(Nz, forced)
                assert e.value.code == -4
                continue
            assert L.enthalpy_plan(Nz, forced) == want, (Nz, forced)
    assert lay.LARGEST_ON_CHIP_NZ == 79 and lay.LARGEST_FORCED_NZ == 159
    assert L.enthalpy_plan(20)["waves_per_cu"] == 7 and L.enthalpy_plan(20)["lds_bytes"] == 21504
    assert L.enthalpy_plan(79)["form"] == L.ENTH_ON_CHIP and L.enthalpy_plan(80)["form"] == L.ENTH_PER_STEP
    for bad in ((0, 0), (-3, 0), (5, 3), (5, -1)):
        with pytest.raises(csi.CsiError) as e:
            L.enthalpy_plan(*bad)
        assert e.value.code == -1
    assert (lay.PER_STEP, lay.ON_CHIP, lay.MAX_SUBSTEPS, lay.MIN_WAVES_PER_CU, lay.LDS_PER_CU) == \
        (L.ENTH_PER_STEP, L.ENTH_ON_CHIP, L.ENTH_MAX_SUBSTEPS, L.ENTH_MIN_WAVES_PER_CU, L.ENTH_LDS_PER_CU)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------

def _c_layout(tmp_path):
    exe = str(tmp_path / "enthalpy_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "enthalpy_layout.c"), "-o", exe])
    return json.loads(subprocess.check_output([exe]).decode())


def test_c_layout_matches_ctypes(tmp_path):
    got = _c_layout(tmp_path)
    assert got["sizeof_params"] == C.sizeof(L.EnthalpyParams) == 64 and got["sizeof_launch"] == C.sizeof(L.EnthalpyLaunch) == 16
    for T, cname in ((L.EnthalpyParams, "csi_enthalpy_params"), (L.EnthalpyLaunch, "csi_enthalpy_launch")):
        for name, _ in T._fields_:
            assert got[f"{cname}.{name}"] == getattr(T, name).offset, name
    assert [got["CSI_ENTH_" + n] for n in ("H", "T", "PHI", "KAPPA")] == [L.ENTH_H, L.ENTH_T, L.ENTH_PHI, L.ENTH_KAPPA]
    assert [got["CSI_ENTH_" + n] for n in ("T_BOTTOM", "T_TOP", "H_BOTTOM", "H_TOP")] == [L.ENTH_T_BOTTOM, L.ENTH_T_TOP, L.ENTH_H_BOTTOM, L.ENTH_H_TOP]
    assert [got["CSI_ENTH_BC_" + n] for n in ("NONE", "NUMBER", "ARRAY", "SERIES_SCALAR", "SERIES_PLANE", "FLUX", "GRADIENT")] == list(range(7)) == \
        [L.ENTH_BC_NONE, L.ENTH_BC_NUMBER, L.ENTH_BC_ARRAY, L.ENTH_BC_SERIES_SCALAR, L.ENTH_BC_SERIES_PLANE, L.ENTH_BC_FLUX, L.ENTH_BC_GRADIENT]
    assert (got["CSI_ENTH_PER_STEP"], got["CSI_ENTH_ON_CHIP"], got["CSI_ENTH_MAX_SUBSTEPS"], got["CSI_ENTH_MIN_WAVES_PER_CU"],
            got["CSI_ENTH_LDS_PER_CU"]) == (L.ENTH_PER_STEP, L.ENTH_ON_CHIP, L.ENTH_MAX_SUBSTEPS, L.ENTH_MIN_WAVES_PER_CU, L.ENTH_LDS_PER_CU)
    # no older id, count or version moved
    assert got["CSI_F_COUNT_SHORTWAVE"] == L.F_COUNT_SHORTWAVE == 72 and got["CSI_VERSION"] == 100
    lib = L.load()
    for name, nargs in (("csi_enthalpy_plan", 6), ("csi_enthalpy_create", 3), ("csi_enthalpy_destroy", 1), ("csi_enthalpy_bind", 3),
                        ("csi_enthalpy_boundary_set", 6), ("csi_enthalpy_set", 3), ("csi_enthalpy_update_state", 2),
                        ("csi_enthalpy_time_step", 5), ("csi_enthalpy_last_launch", 2), ("csi_enthalpy_ice_thickness", 3)):
        assert len(getattr(lib, name).argtypes) == nargs and name in L.SYMBOLS


def test_c_layout_matches_julia_stub(tmp_path):
    got = _c_layout(tmp_path)
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    for const, prefix in (("ENTHALPY", "CSI_ENTH_"), ("ENTHALPY_SIDE", "CSI_ENTH_"), ("ENTHALPY_BC", "CSI_ENTH_BC_")):
        m = re.search(r"^const %s = \((.*?)\)" % const, stub, re.S | re.M)
        assert m, const
        vals = {k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)", m.group(1))}
        assert vals and vals == {k: got[prefix + k] for k in vals}, const
    for name in ("CSI_ENTH_PER_STEP", "CSI_ENTH_ON_CHIP", "CSI_ENTH_MAX_SUBSTEPS"):
        m = re.search(r"^const %s = (\d+)" % name, stub, re.M)
        assert m and int(m.group(1)) == got[name], name
    size_of = {"Cdouble": 8, "Float64": 8, "Int32": 4, "Cint": 4, "Ptr": 8}
    for jname, cname, T, size in (("CsiEnthalpyParams", "csi_enthalpy_params", L.EnthalpyParams, "sizeof_params"),
                                  ("CsiEnthalpyLaunch", "csi_enthalpy_launch", L.EnthalpyLaunch, "sizeof_launch")):
        m = re.search(r"^struct\s+" + jname + r"\b[^\n]*\n(.*?)\nend", stub, re.S | re.M)
        assert m, jname
        fields = re.findall(r"([A-Za-z_]\w*)::(\w+)", re.sub(r"#[^\n]*", "", m.group(1)))
        off, offsets = 0, {}
        for name, t in fields:
            s = size_of[t]
            off = (off + s - 1) // s * s
            offsets[name] = off
            off += s
        assert offsets == {n: got[f"{cname}.{n}"] for n, _ in T._fields_}, jname
        assert (off + 7) // 8 * 8 == got[size] or off == got[size], jname
    for fn in ("csi_enthalpy_plan", "csi_enthalpy_create", "csi_enthalpy_destroy", "csi_enthalpy_bind", "csi_enthalpy_boundary_set",
               "csi_enthalpy_set", "csi_enthalpy_update_state", "csi_enthalpy_time_step", "csi_enthalpy_last_launch",
               "csi_enthalpy_ice_thickness"):
        assert re.search(r"ccall\(\(:%s, " % fn, stub), fn
    assert "function attach_enthalpy" in stub and "this stub passes Numbers only" in stub


def test_header_is_the_definition():
    text = open(os.path.join(ROOT, "include", "csi.h"), encoding="utf-8").read()
    for words in ("flux[k] = ((kappa[k] + kappa[k - 1]) / 2) * ((T[k] - T[k - 1]) / dzf[k])", "G[k]    = (flux[k + 1] - flux[k]) / dzc[k]",
                  "dzf[1] = dzc[1] and dzf[Nz + 1] = dzc[Nz]", "T[0] = 2 * Tb - T[1]", "Frozen cells (phi = 1) take kappa_WATER",
                  "update_state at the time the\n *                  step STARTED from", "(2 Nz + 2) * 512", "CSI_ENTH_MIN_WAVES_PER_CU = 2",
                  "this definition is OURS", "STATUS: RECALLED", "psi_2 * frac + psi_1 * (1 - frac)"):
        assert words in text, words


# ---- front end ----------------------------------------------------------------------------------------------------------------------------

def test_column_grid():
    g = csi.ColumnGrid(20, z=(-1, 0), topology=(csi.Flat, csi.Flat, csi.Bounded))
    assert (g.Nx, g.Ny, g.Nz) == (1, 1, 20) and np.array_equal(g.z_faces, ref.uniform_faces(-1.0, 0.0, 20))
    assert g.z_faces[0] == -1.0 and g.z_faces[-1] == 0.0 and g.interior_size() == (1, 1)
    g = csi.ColumnGrid((5, 3, 4), z=[-2.0, -1.0, -0.5, -0.2, 0.0])
    assert (g.Nx, g.Ny, g.Nz) == (5, 3, 4) and g.minimum_zspacing() == pytest.approx(0.2)
    for kw, err in ((dict(size=4, z=(0, -1)), ValueError), (dict(size=4, z=[0, 1, 2]), ValueError), (dict(size=(4, 4), z=(0, 1)), ValueError),
                    (dict(size=0, z=(0, 1)), ValueError), (dict(size=4, z=(0, 1), topology=(csi.Flat, csi.Flat, csi.Periodic)), NotImplementedError)):
        with pytest.raises(err, match="ColumnGrid"):
            csi.ColumnGrid(**kw)


def test_value_boundary_condition_keeps_arrays_and_series_and_old_consumers_refuse_them():
    assert csi.ValueBoundaryCondition(3).value == 3.0 and isinstance(csi.ValueBoundaryCondition(3).value, float)
    a = np.zeros((2, 3))
    assert csi.ValueBoundaryCondition(a).value is a
    g = csi.ColumnGrid((3, 2, 4), z=(-1, 0))
    s = csi.ColumnTimeSeries(g, [0.0, 1.0], [1.0, 2.0])
    assert csi.ValueBoundaryCondition(s).value is s and s.scalar
    assert not csi.ColumnTimeSeries(g, [0.0, 1.0], np.zeros((2, 2, 3))).scalar
    f = csi.FieldBoundaryConditions(top=csi.ValueBoundaryCondition(1.0))
    assert f.top.value == 1.0 and f.bottom is None and f.north is None


@pytest.mark.parametrize("make, err, words", [
    (lambda g: dict(grid=csi.RectilinearGrid((8, 8), x=(0, 1), y=(0, 1))), TypeError, "grid is a ColumnGrid"),
    (lambda g: dict(closure=object()), NotImplementedError, "closure is a MolecularDiffusivity"),
    (lambda g: dict(boundary_conditions=dict(H=csi.FieldBoundaryConditions(top=csi.ValueBoundaryCondition(0.0)))), NotImplementedError,
     "a boundary condition on H is not supported"),
    (lambda g: dict(boundary_conditions=dict(T=csi.FieldBoundaryConditions(top=csi.FluxBoundaryCondition(1.0)))), NotImplementedError,
     "flux and gradient conditions are not supported"),
    (lambda g: dict(boundary_conditions=dict(T=csi.FieldBoundaryConditions(bottom=csi.ValueBoundaryCondition(np.zeros((4, 4)))))), ValueError,
     r"bottom temperature array has shape \(4, 4\)"),
    (lambda g: dict(boundary_conditions=dict(T=csi.FieldBoundaryConditions(top=csi.ValueBoundaryCondition(lambda x, y, t: 0.0)))),
     NotImplementedError, "function-valued top temperature"),
    (lambda g: dict(boundary_conditions=dict(T=csi.FieldBoundaryConditions(top=csi.ValueBoundaryCondition(
        csi.ColumnTimeSeries(csi.ColumnGrid((7, 2, 4), z=(-1, 0)), [0.0, 1.0], [0.0, 1.0]))))), ValueError, "made for another grid"),
    (lambda g: dict(boundary_conditions=dict(u=csi.FieldBoundaryConditions())), ValueError, "unknown fields"),
])
def test_model_refusals_by_name_before_a_device_is_touched(make, err, words):
    g = csi.ColumnGrid((3, 2, 4), z=(-1, 0))
    kw = dict(grid=g)
    kw.update(make(g))
    with pytest.raises(err, match=words):
        csi.EnthalpyMethodSeaIceModel(**kw)


def test_series_refusals_by_name():
    g = csi.ColumnGrid((3, 2, 4), z=(-1, 0))
    with pytest.raises(NotImplementedError, match="host-resident backend"):
        csi.ColumnTimeSeries(g, [0.0, 1.0], [0.0, 1.0], backend=csi.InMemory(2))
    with pytest.raises(ValueError, match=r"\(Nt,\) = \(2,\) or \(Nt, Ny, Nx\)"):
        csi.ColumnTimeSeries(g, [0.0, 1.0], np.zeros((2, 3)))
    with pytest.raises(ValueError, match="strictly increasing"):
        csi.ColumnTimeSeries(g, [1.0, 1.0], [0.0, 1.0])
    s = csi.ColumnTimeSeries(g, [0.0, 10.0, 20.0], [1.0, 2.0, 4.0], time_indexing=csi.Clamp())
    assert s.plan(15.0) == tsr.plan(s.times, tsr.CLAMP, 0.0, 15.0)


def test_an_output_writer_over_column_fields_is_refused_by_name(tmp_path):
    m = object.__new__(csi.EnthalpyMethodSeaIceModel)          # (no device is touched: the refusal comes first)
    with pytest.raises(NotImplementedError, match="output writer over the column fields"):
        csi.OutputWriter(m, ["T"], csi.IterationInterval(1), str(tmp_path))


def test_velocity_conditions_of_the_sea_ice_model_still_take_numbers_only():
    import inspect
    src = inspect.getsource(csi.SeaIceModel)
    assert "ValueBoundaryCondition(number); an array or a FieldTimeSeries" in src
