"""CPU tests of the device diagnostics' definition: the NumPy restatement (tests/diagnostics_ref.py) against math.fsum within the
order-independent worst-case bound, on the inputs the GPU tests use; the restatement's ability to fail; new_time_step at each clamp;
the layout of csi_diagnostics as gcc, ctypes and the Julia stub see it; argument errors of the Python front end."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import climaseaice_jl_amd as csi
import diagnostics_cases as dc
import diagnostics_ref as ref

L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _terms(c):
    _, _, az = ref.metrics_of(c["g"])
    return ref.tracer_terms(c["h"], c["a"], c["hs"], az, c["mask"], dc.THRESHOLD)[1]


@pytest.mark.parametrize("grid", ["narrow", "many", "more_records_than_threads"])
@pytest.mark.parametrize("config", ["bb_latlon_land_snow", "pp_curvilinear_snow", "bb_uniform_land"])
def test_ordered_sums_within_the_worst_case_bound_of_fsum(grid, config):
    """Each sum of the restatement lies within (n - 1) 2^-53 sum |x_i| of math.fsum: the bound of recursive summation in ANY order."""
    topo, metrics, land, snow = dc.CONFIGS[config]
    c = dc.make(*dc.GRIDS[grid], topo=topo, metrics=metrics, land=land, snow=snow)
    for name, t in _terms(c).items():
        exact, bound = ref.fsum_bound(t)
        got = ref.ordered_sum(t)
        print(name, grid, config, "ordered", got, "fsum", exact, "difference", got - exact, "bound", bound)
        assert abs(got - exact) <= bound, (name, got, exact, bound)
        assert exact > 0.0 or (name == "snow_volume" and not snow)


def test_ordered_sum_is_the_documented_tree_on_integers():
    """Exact data: any order gives the same integers, and a cell counted twice or not at all shows."""
    rng = np.random.default_rng(0)
    for ny, nx in ((29, 37), (16, 64), (33, 130), (260, 1030), (64, 64), (65, 130), (65, 65), (1030, 1030)):
        t = rng.integers(0, 1000, (ny, nx)).astype(np.float64)
        assert ref.ordered_sum(t) == float(t.sum())
    # the order itself, where it matters: 1e16 + 1 + 1 (a thread's rows 0, 4, 8 of one column) loses both ones; in another order it keeps them
    t = np.zeros((16, 64))
    t[0, 0], t[4, 0], t[8, 0] = 1e16, 1.0, 1.0
    assert ref.ordered_sum(t) == 1e16
    t[4, 0] = t[8, 0] = 0.0
    t[1, 0] = t[1, 1] = 1.0                         # row 1 is wave 1's: the ones meet in its butterfly before the waves are added
    assert ref.ordered_sum(t) == 1e16 + 2.0


@pytest.mark.parametrize("grid", ["narrow", "many"])
def test_the_restatement_can_fail(grid):
    """Dropping one interior cell or including one halo column moves a sum by more than the bound on the inputs the GPU tests use."""
    Nx, Ny = dc.GRIDS[grid]
    c = dc.make(Nx, Ny, topo=("periodic", "periodic"), metrics="latlon", snow=True)
    for name, t in _terms(c).items():
        _, bound = ref.fsum_bound(t)
        good = ref.ordered_sum(t)
        dropped = t.copy()
        j, i = np.argwhere(t > 0)[-1]
        dropped[j, i] = 0.0
        assert abs(ref.ordered_sum(dropped) - good) > bound, name
        halo = np.concatenate([t, t[:, :1]], axis=1)         # the periodic image of column 1 as column Nx + 1
        assert abs(ref.ordered_sum(halo) - good) > bound, name


def test_the_timescale_restatement_sees_the_wrong_metric():
    """dx^fc swapped for another dx moves the timescale by more than n 2^-53 relative.  On a REGULAR latitude-longitude grid dx^fc and
    dx^cc are the same numbers (dx varies with the row only), so there the swap that can show is dx^fc for dx^cf (Face rows); dx^fc for
    dx^cc is checked on the distorted curvilinear form of the same grid, where the two differ."""
    Nx, Ny = dc.GRIDS["narrow"]
    n = Nx * Ny
    c = dc.make(Nx, Ny, metrics="latlon")
    g = c["g"]
    dxfc, dycf, _ = ref.metrics_of(g)
    good = ref.velocity_group(c["u"], c["v"], dxfc, dycf)["advection_timescale"]
    dxcf = np.asarray(g.metrics()["dxf"])[g.Hy:g.Hy + Ny, None] * np.ones((Ny, Nx))
    bad = ref.velocity_group(c["u"], c["v"], dxcf, dycf)["advection_timescale"]
    assert abs(bad - good) > n * 2.0 ** -53 * good
    c = dc.make(Nx, Ny, metrics="curvilinear")
    g = c["g"]
    dxfc, dycf, _ = ref.metrics_of(g)
    good = ref.velocity_group(c["u"], c["v"], dxfc, dycf)["advection_timescale"]
    dxcc = g.metrics()["dxcc"][g.Hy:g.Hy + Ny, g.Hx:g.Hx + Nx]
    bad = ref.velocity_group(c["u"], c["v"], dxcc, dycf)["advection_timescale"]
    assert abs(bad - good) > n * 2.0 ** -53 * good


def test_timescale_definition_on_hand_worked_values():
    u = np.array([[0.0, -2.0], [1.0, 0.5]])
    v = np.array([[0.0, 1.0], [-4.0, 0.0]])
    dx, dy = np.full((2, 2), 4.0), np.full((2, 2), 8.0)
    r = ref.velocity_group(u, v, dx, dy)
    assert r["inv_timescale_max"] == 0.75 and r["advection_timescale"] == 1.0 / 0.75       # cell (1, 0): 1 / 4 + 4 / 8
    assert (r["max_abs_u"], r["max_abs_v"]) == (2.0, 4.0)
    assert ref.velocity_group(0 * u, 0 * v, dx, dy)["advection_timescale"] == math.inf      # ice at rest
    u[0, 0] = math.inf
    r = ref.velocity_group(u, v, dx, dy)
    assert r["advection_timescale"] == 0.0 and r["nonfinite_u"] == 1 and r["nan_u"] == 0
    v[1, 1] = math.nan
    r = ref.velocity_group(u, v, dx, dy)
    assert math.isnan(r["advection_timescale"]) and r["nonfinite_v"] == 1 and r["nan_v"] == 1 and r["max_abs_v"] == 4.0


def test_new_time_step_at_each_clamp():
    W = csi.TimeStepWizard
    w = W()
    assert (w.cfl, w.max_change, w.min_change, w.max_dt, w.min_dt) == (0.2, 1.1, 0.5, math.inf, 0.0)
    assert csi.new_time_step(100.0, 525.0, w) == 0.2 * 525.0                 # cfl * timescale = 105, inside [50, 110]
    assert csi.new_time_step(100.0, 1000.0, w) == 1.1 * 100.0                # 200 -> max_change * old_dt
    assert csi.new_time_step(100.0, 100.0, w) == 0.5 * 100.0                 # 20 -> min_change * old_dt
    assert csi.new_time_step(100.0, 525.0, W(max_dt=90.0)) == 90.0           # 105 -> max_dt
    assert csi.new_time_step(100.0, 100.0, W(min_dt=60.0)) == 60.0           # 50 -> min_dt
    assert csi.new_time_step(100.0, math.inf, w) == 1.1 * 100.0              # ice at rest: grow by max_change
    assert csi.new_time_step(100.0, math.inf, W(max_dt=105.0)) == 105.0
    assert csi.new_time_step(100.0, 0.0, w) == 50.0                          # an infinite velocity: shrink by min_change
    assert math.isnan(csi.new_time_step(100.0, math.nan, w))
    assert csi.new_time_step(100.0, 525.0, W(cfl=0.1, max_change=2.0, min_change=0.1)) == 0.1 * 525.0
    with pytest.raises(Exception):
        w.cfl = 0.3                                                           # immutable


# ---- ABI: header, ctypes mirror, Julia stub ------------------------------------------------------------------------------------------
FIELDS = ["what", "has_snow", "advection_timescale", "inv_timescale_max", "max_abs_u", "max_abs_v", "nonfinite_u", "nonfinite_v", "nan_u",
          "nan_v", "ice_volume", "ice_area", "ice_extent", "snow_volume", "active_area", "min_h", "max_h", "min_aice", "max_aice", "max_hs",
          "nonfinite_h", "nonfinite_aice", "nonfinite_hs", "active_cells", "extent_threshold"]


def _c_layout(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    exe = tmp_path / "diagnostics_layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "diagnostics_layout.c"), "-o", str(exe)])
    return {k: int(v) for k, v in (ln.split("=") for ln in subprocess.check_output([str(exe)]).decode().split())}


def test_c_compiler_layout_matches_ctypes(tmp_path):
    got = _c_layout(tmp_path)
    T = L.Diagnostics
    assert [f[0] for f in T._fields_] == FIELDS
    assert C.sizeof(T) == got["sizeof"] == 8 + 23 * 8
    for f in FIELDS:
        assert getattr(T, f).offset == got["offset_" + f], f
    assert (got["CSI_DIAG_VELOCITY"], got["CSI_DIAG_TRACERS"], got["CSI_DIAG_ALL"]) == (L.DIAG_VELOCITY, L.DIAG_TRACERS, L.DIAG_ALL) == (1, 2, 3)
    assert got["CSI_VERSION"] == 100 and got["CSI_F_COUNT_TOTAL"] == len(L.F)         # no slot was added
    assert got["compute_result_bytes"] == 4


def test_c_compiler_layout_matches_julia_stub(tmp_path):
    """struct CsiDiagnostics of julia/ClimaSeaIceHIP.jl (never executed here), laid out by C's rules, against gcc's; the ccall and the
    two methods built on it."""
    got = _c_layout(tmp_path)
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    m = re.search(r"^struct\s+CsiDiagnostics\b[^\n]*\n(.*?)\nend", stub, re.S | re.M)
    assert m, "struct CsiDiagnostics is missing from the Julia stub"
    body = re.sub(r"#[^\n]*", "", m.group(1))
    fields = re.findall(r"([A-Za-z_]\w*)::(\w+)", body)
    size_of = {"Cdouble": 8, "Float64": 8, "Int32": 4, "Cint": 4, "Int64": 8}
    off, offsets = 0, {}
    for name, t in fields:
        s = size_of[t]
        off = (off + s - 1) // s * s
        offsets[name] = off
        off += s
    assert list(offsets) == FIELDS
    assert offsets == {f: got["offset_" + f] for f in FIELDS} and (off + 7) // 8 * 8 == got["sizeof"]
    assert re.search(r"ccall\(\(:csi_diagnostics_compute, libcsi\), Int32, \(Ptr\{Cvoid\}, Int32, Cdouble, Ptr\{CsiDiagnostics\}\)", stub)
    assert re.search(r"Oceananigans\.Advection\.cell_advection_timescale\(model::HIPSeaIceModel\)", stub)
    assert re.search(r"function diagnostics\(model::HIPSeaIceModel", stub)


def test_library_exports_the_entry_point_and_the_header_defines_the_order():
    lib = L.load()
    assert lib.csi_diagnostics_compute.argtypes is not None and "csi_diagnostics_compute" in L.SYMBOLS
    text = open(os.path.join(ROOT, "include", "csi.h")).read()
    sec = text[text.index("device diagnostics: advection timescale"):text.index("int32_t csi_diagnostics_compute")]
    for needle in ("RECALLED", "SUMMATION ORDER", "32, 16, 8, 4, 2, 1", "COLLECTIVE", "rank order", "t + 256"):
        assert needle in sec, needle
    survey = open(os.path.join(ROOT, "SURVEY.md"), encoding="utf-8").read()
    assert "cell_advection_timescale" in survey[survey.index("## Appendix B"):survey.index("## Appendix C")]


# ---- argument errors of the front end, by name (the ABI's own, which need a context: tests/test_gpu_diagnostics.py) ---------------------
def test_front_end_argument_errors():
    from climaseaice_jl_amd import diagnostics as D
    assert (D._what_mask("all"), D._what_mask("velocity"), D._what_mask("tracers"), D._what_mask(("velocity", "tracers"))) == (3, 1, 2, 3)
    with pytest.raises(ValueError, match="'all', 'velocity' or 'tracers'"):
        D._what_mask("momentum")
    with pytest.raises(ValueError, match="'all', 'velocity' or 'tracers'"):
        D._what_mask(("velocity", "snow"))
    for name in ("Diagnostics", "TimeStepWizard", "new_time_step", "cell_advection_timescale", "assert_finite"):
        assert hasattr(csi, name), name
    assert hasattr(csi.SeaIceModel, "diagnostics")
