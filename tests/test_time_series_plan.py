"""csi_time_series_plan (pure host function of libcsi_hip.so, no GPU) against the NumPy restatement of include/csi.h's statement
(tests/time_series_ref.py): indices equal and the weight BIT-equal, for the three indexing kinds; the properties the statement implies;
the layout of csi_time_series as gcc, ctypes and the Julia stub see it."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import climaseaice_jl_amd as csi
import time_series_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = csi._lib
KINDS = {"clamp": L.TIME_CLAMP, "cyclical": L.TIME_CYCLICAL, "linear": L.TIME_LINEAR}
NONUNIFORM = np.array([3.0, 10.0, 11.0, 40.0, 41.5])
UNIFORM = np.arange(10) * 10800.0
SERIES = {"nonuniform": NONUNIFORM, "uniform": UNIFORM, "two": np.array([-2.5, 0.75]),
          "thirds": np.array([0.1, 0.2, 0.30000000000000004, 0.7, 1.1, 1.3])}


def probe_times(times, period):
    """every node, points between the nodes (midpoints and uneven fractions), before and after the ends; for a cyclical series also
    the gap, exactly one / two periods later and negative times"""
    t = list(times)
    for a, b in zip(times[:-1], times[1:]):
        t += [0.5 * (a + b), a + 0.1 * (b - a), a + (b - a) / 3.0, np.nextafter(a, b), np.nextafter(b, a)]
    span, step = times[-1] - times[0], times[-1] - times[-2]
    t += [times[0] - 0.25 * step, times[0] - 7.0 * span, times[-1] + 0.25 * step, times[-1] + 0.5 * step, times[-1] + 3.3 * span]
    if period:
        gap = period - span
        t += [times[-1] + 0.5 * gap, times[-1] + 0.999 * gap, times[0] + period, times[0] + 2 * period, times[2 % len(times)] + period,
              0.5 * (times[0] + times[1]) + period, times[0] - 0.3 * period, -1.7 * period, times[-1] - 3 * period, 0.0, -0.0]
    return [float(x) for x in t]


@pytest.mark.parametrize("name", list(SERIES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_plan_equals_the_restatement_bit_for_bit(kind, name):
    times = SERIES[name]
    periods = [0.0]
    if kind == "cyclical":
        span = times[-1] - times[0]
        periods += [span * 1.25, span + 1e-3 * (times[-1] - times[-2]), 2.0 * span + 1.0]
    n = 0
    for period in periods:
        P = period if period else (ref.inferred_period(times) if kind == "cyclical" else 0.0)
        for t in probe_times(times, P):
            want = ref.plan(times, KINDS[kind], period, t)
            got = L.time_series_plan(times, KINDS[kind], period, t)
            assert got[:2] == want[:2], (kind, name, period, t, got, want)
            assert np.float64(got[2]).tobytes() == np.float64(want[2]).tobytes(), (kind, name, period, t, got, want)
            n += 1
    assert n >= 12


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_node_returns_its_own_slice(kind):
    for times in SERIES.values():
        for n, t in enumerate(times):
            n1, n2, w = L.time_series_plan(times, KINDS[kind], 0.0, float(t))
            assert (n1 == n2 == n) or (n1 == n and w == 0.0) or (n2 == n and w == 1.0), (kind, n, (n1, n2, w))


def test_clamp_holds_the_end_slices_and_linear_extrapolates():
    t = NONUNIFORM
    assert L.time_series_plan(t, L.TIME_CLAMP, 0.0, -100.0) == (0, 0, 0.0)
    assert L.time_series_plan(t, L.TIME_CLAMP, 0.0, 1e9) == (4, 4, 0.0)
    n1, n2, w = L.time_series_plan(t, L.TIME_LINEAR, 0.0, -4.0)
    assert (n1, n2) == (0, 1) and w == (-4.0 - 3.0) / (10.0 - 3.0) and w < 0
    n1, n2, w = L.time_series_plan(t, L.TIME_LINEAR, 0.0, 44.5)
    assert (n1, n2) == (3, 4) and w == (44.5 - 40.0) / (41.5 - 40.0) and w > 1
    # inside, the two kinds agree
    for x in (3.0, 5.0, 10.5, 39.0, 41.5):
        assert L.time_series_plan(t, L.TIME_LINEAR, 0.0, x) == L.time_series_plan(t, L.TIME_CLAMP, 0.0, x)


def test_cyclical_period_gap_and_wrap():
    t = NONUNIFORM
    assert ref.inferred_period(t) == (41.5 - 3.0) + 1.5 == 40.0
    # the gap behind the last node: slices (nt - 1, 0), the weight measured across the gap
    assert L.time_series_plan(t, L.TIME_CYCLICAL, 0.0, 42.25) == (4, 0, 0.5)
    assert L.time_series_plan(t, L.TIME_CYCLICAL, 50.0, 41.5 + 5.75) == (4, 0, 0.5)
    # one period later the indices are the same (these times are exactly representable, so is the weight)
    for x in (3.0, 4.0, 10.0, 10.5, 25.5, 40.0, 41.5, 42.25, -6.0, -37.0):
        for period in (0.0, 64.0):
            P = period or 40.0
            a, b = L.time_series_plan(t, L.TIME_CYCLICAL, period, x), L.time_series_plan(t, L.TIME_CYCLICAL, period, x + P)
            assert a == b, (x, period, a, b)
    assert L.time_series_plan(t, L.TIME_CYCLICAL, 0.0, 3.0 - 40.0) == (0, 0, 0.0)
    assert L.time_series_plan(t, L.TIME_CYCLICAL, 0.0, -30.0)[:2] == (1, 1)          # 10 - 40


def test_invalid_input_is_refused():
    bad = [([5.0], L.TIME_CLAMP, 0.0, 5.0), ([1.0, 1.0, 2.0], L.TIME_LINEAR, 0.0, 1.5), ([1.0, 3.0, 2.0], L.TIME_CLAMP, 0.0, 1.5),
           ([0.0, 1.0, 2.0], L.TIME_CYCLICAL, 2.0, 0.5), ([0.0, 1.0, 2.0], L.TIME_CYCLICAL, 1.5, 0.5), ([0.0, 1.0], 7, 0.0, 0.5),
           ([0.0, 1.0], L.TIME_CLAMP, 0.0, float("nan")), ([0.0, float("inf")], L.TIME_CLAMP, 0.0, 0.5)]
    for times, kind, period, t in bad:
        with pytest.raises(csi.CsiError) as e:
            L.time_series_plan(times, kind, period, t)
        assert e.value.code == -1                                   # CSI_ERR_INVALID_ARGUMENT
        with pytest.raises(ref.InvalidSeries):
            ref.plan(times, kind, period, t)
    lib = L.load()
    n1, n2, w = C.c_int32(), C.c_int32(), C.c_double()
    assert lib.csi_time_series_plan(None, 3, 0, 0.0, 0.0, C.byref(n1), C.byref(n2), C.byref(w)) == -1
    # a period just longer than the span is fine
    assert L.time_series_plan([0.0, 1.0, 2.0], L.TIME_CYCLICAL, 2.5, 2.25) == (2, 0, 0.5)


def test_interpolation_formula_of_the_restatement():
    rng = np.random.default_rng(1)
    data = rng.standard_normal((3, 4, 5))
    assert np.array_equal(ref.interpolate(data, 1, 1, 0.0), data[1])
    w = 0.3
    assert np.array_equal(ref.interpolate(data, 0, 2, w), data[2] * w + data[0] * (1.0 - w))
    assert np.array_equal(ref.at([0.0, 1.0, 2.0], data, ref.LINEAR, 0.0, 3.0), data[2] * 2.0 + data[1] * (1.0 - 2.0))


# ---- ABI: header, ctypes mirror, Julia stub -----------------------------------------------------------------------------------------
def _c_layout(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    exe = tmp_path / "time_series_layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "time_series_layout.c"), "-o", str(exe)])
    return {k: int(v) for k, v in (ln.split("=") for ln in subprocess.check_output([str(exe)]).decode().split())}


FIELDS = ["nt", "indexing", "backend", "window", "period", "times", "data", "ld", "slice_stride"]


def test_c_compiler_layout_matches_ctypes(tmp_path):
    got = _c_layout(tmp_path)
    T = L.TimeSeries
    assert [f[0] for f in T._fields_] == FIELDS
    assert C.sizeof(T) == got["sizeof"] == 56
    for f in FIELDS:
        assert getattr(T, f).offset == got["offset_" + f], f
    assert (got["CSI_TIME_CLAMP"], got["CSI_TIME_CYCLICAL"], got["CSI_TIME_LINEAR"]) == (L.TIME_CLAMP, L.TIME_CYCLICAL, L.TIME_LINEAR) == (0, 1, 2)
    assert (got["CSI_SERIES_DEVICE"], got["CSI_SERIES_HOST"]) == (L.SERIES_DEVICE, L.SERIES_HOST) == (0, 1)
    assert got["CSI_VERSION"] == 100 and got["CSI_F_COUNT_TOTAL"] == len(L.F)         # no slot was added
    assert all(got[k] == 4 for k in ("plan_result_bytes", "set_result_bytes", "update_result_bytes", "status_result_bytes"))
    assert (csi.Clamp.kind, csi.Cyclical.kind, csi.Linear.kind) == (0, 1, 2)


def test_c_compiler_layout_matches_julia_stub(tmp_path):
    """struct CsiTimeSeries of julia/ClimaSeaIceHIP.jl (never executed here), laid out by C's rules, against gcc's; the three ccalls."""
    got = _c_layout(tmp_path)
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    m = re.search(r"^struct\s+CsiTimeSeries\b[^\n]*\n(.*?)\nend", stub, re.S | re.M)
    assert m, "struct CsiTimeSeries is missing from the Julia stub"
    body = re.sub(r"#[^\n]*", "", m.group(1))
    fields = re.findall(r"([A-Za-z_]\w*)::((?:Ptr\{[^}]*\})|\w+)", body)
    size_of = {"Cdouble": 8, "Float64": 8, "Int32": 4, "Cint": 4, "Int64": 8}
    off, offsets = 0, {}
    for name, t in fields:
        s = 8 if t.startswith("Ptr{") else size_of[t]
        off = (off + s - 1) // s * s
        offsets[name] = off
        off += s
    assert list(offsets) == FIELDS
    assert offsets == {f: got["offset_" + f] for f in FIELDS} and (off + 7) // 8 * 8 == got["sizeof"]
    for name, args in (("csi_time_series_set", r"\(Ptr\{Cvoid\}, Int32, Ptr\{CsiTimeSeries\}\)"),
                       ("csi_time_series_update", r"\(Ptr\{Cvoid\}, Cdouble\)"),
                       ("csi_time_series_status", r"\(Ptr\{Cvoid\}, Int32, Ptr\{Int32\}, Ptr\{Int64\}\)")):
        assert re.search(r"ccall\(\(:" + name + r", libcsi\), Int32, " + args, stub), name
    assert re.search(r"function attach_time_series!\(ctx, slot, times, host_array; window", stub)


def test_library_exports_the_new_entry_points_and_lists_the_eleven_slots():
    lib = L.load()
    for name in ("csi_time_series_plan", "csi_time_series_set", "csi_time_series_update", "csi_time_series_status"):
        assert getattr(lib, name).argtypes is not None and name in L.SYMBOLS
    assert len(L.SERIES_SLOTS) == 11 and all(s in L.F for s in L.SERIES_SLOTS)
    text = open(os.path.join(ROOT, "include", "csi.h")).read()
    assert "RECALLED" in text[text.index("forcing time series interpolated"):text.index("csi_time_series_plan(const double")]
