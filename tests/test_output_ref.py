"""CPU tests of the device-side output's definition: the NumPy restatement (tests/output_ref.py) of the record layout, ownership,
masking, conversion, accumulation order and division; the layout rule against the library's pure host function; the ABI as gcc,
ctypes and the Julia stub see it; the argument checks that need no device."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import climaseaice_jl_amd as csi
import output_ref as ref

L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["csi_output_plan_layout", "csi_output_create", "csi_output_layout", "csi_output_record_bytes", "csi_output_accumulate",
           "csi_output_snapshot", "csi_output_test", "csi_output_wait", "csi_output_release", "csi_output_destroy"]


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes, dtypes", [
    ([(7, 65), (8, 64), (7, 64), (7, 64), (8, 65)], ["f32"] * 5),
    ([(7, 65), (8, 64), (7, 64), (7, 64), (8, 65)], ["f64"] * 5),
    ([(1, 1)], ["f32"]), ([(1, 1), (1, 2), (2, 1)], ["f64", "f32", "f64"]),
    ([(2048, 2048)] * 4, ["f32"] * 4), ([(3, 1025)] * 16, ["f32", "f64"] * 8),
])
def test_layout_rule_and_the_library_agree(shapes, dtypes):
    offs, total = ref.layout(shapes, dtypes)
    assert all(o % 256 == 0 for o in offs) and total % 256 == 0
    for k in range(1, len(offs)):          # dense, in list order, no overlap, less than one alignment unit of padding
        size = shapes[k - 1][0] * shapes[k - 1][1] * (4 if dtypes[k - 1] == "f32" else 8)
        assert 0 <= offs[k] - offs[k - 1] - size < 256
    got = L.output_plan_layout(shapes, [L.OUT_F32 if d == "f32" else L.OUT_F64 for d in dtypes])
    assert got == (offs, total)


def test_layout_refuses_bad_input():
    for shapes, dtypes in (([], []), ([(0, 4)], [0]), ([(4, 4)], [2]), ([(1, 1)] * 17, [0] * 17)):
        with pytest.raises(csi.CsiError) as e:
            L.output_plan_layout(shapes, dtypes)
        assert e.value.code == -1


# ---- elements -------------------------------------------------------------------------------------------------------------------------
def test_fp32_conversion_of_the_planted_values():
    x = np.array([1e300, -1e300, 1e-40, -1e-40, 1e-46, -1e-46, 0.0, -0.0, np.inf, -np.inf, np.nan, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24])
    y = ref.convert(x, "f32")
    assert y.dtype == np.float32
    assert y[0] == np.inf and y[1] == -np.inf                                   # overflow
    assert y[2] != 0 and abs(float(y[2])) < np.finfo(np.float32).tiny and y[3] == -y[2]      # subnormal results are kept
    assert y[4] == 0 and not np.signbit(y[4]) and y[5] == 0 and np.signbit(y[5])             # below half the smallest: a signed zero
    assert not np.signbit(y[6]) and np.signbit(y[7]) and np.isnan(y[10])
    assert y[11] == np.float32(1.0) and y[12] == np.float32(1.0 + 2.0 ** -22)   # ties to even, both ways
    assert ref.convert(x, "f64").dtype == np.float64 and ref.same_bits(ref.convert(x, "f64"), x)


def test_accumulation_rounds_the_product_before_the_sum():
    """acc + (x * w) with the product rounded differs from the fused result on operands chosen for it."""
    x, w, acc = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0
    two_step = float(ref.accumulate(np.array([acc]), np.array([x]), w)[0])
    assert two_step == acc + (x * w)
    exact = Fraction(x) * Fraction(w) + Fraction(acc)
    assert Fraction(two_step) != exact and float(exact) != two_step            # a fused multiply-add would return float(exact)


def test_average_is_a_division_not_a_reciprocal():
    W = ref.total_weight([120.0, 37.5, 0.1, 1e-3])
    assert W == ((120.0 + 37.5) + 0.1) + 1e-3
    rng = np.random.default_rng(1)
    acc = rng.random(4096) * 100
    assert not np.array_equal(ref.average(acc, W), acc * (1.0 / W))
    assert np.array_equal(ref.average(acc, W), np.array([a / W for a in acc]))


def test_averaged_is_the_ordered_weighted_sum():
    rng = np.random.default_rng(2)
    xs = [rng.standard_normal((3, 5)) for _ in range(4)]
    ws = [120.0, 37.5, 0.1, 1e-3]
    want = ((((0.0 + xs[0] * ws[0]) + xs[1] * ws[1]) + xs[2] * ws[2]) + xs[3] * ws[3]) / ref.total_weight(ws)
    assert ref.same_bits(ref.averaged(xs, ws), want)
    assert not ref.same_bits(ref.averaged(xs[::-1], ws[::-1]), want)            # the order is part of the definition


def test_mask_fills_inactive_cells_only():
    x = np.arange(12.0).reshape(3, 4)
    mask = np.ones((3, 4), np.uint8)
    mask[0, :] = mask[:, 0] = 0
    for fill in (np.nan, -999.0):
        y = ref.element(x, "f32", mask, fill)
        assert ref.same_bits(y[mask == 0], np.full(6, fill, np.float32))
        assert np.array_equal(y[mask != 0], x[mask != 0].astype(np.float32))
    assert ref.same_bits(ref.element(x, "f64"), x)


def test_same_bits_can_fail():
    a = np.array([0.0, np.nan, 1.0])
    assert ref.same_bits(a, a.copy())
    assert not ref.same_bits(a, np.array([-0.0, np.nan, 1.0]))
    assert not ref.same_bits(a, np.array([0.0, 1.0, 1.0]))
    assert not ref.same_bits(a, a.astype(np.float32))


# ---- interiors and ownership ----------------------------------------------------------------------------------------------------------
LOCS = {"u": (csi.Face, csi.Center), "v": (csi.Center, csi.Face), "h": (csi.Center, csi.Center), "s12": (csi.Face, csi.Face)}


@pytest.mark.parametrize("topo", [(csi.Periodic, csi.Periodic), (csi.Bounded, csi.Bounded), (csi.Periodic, csi.Bounded)])
def test_interior_excludes_halos_and_has_the_bounded_face(topo):
    g = csi.RectilinearGrid((5, 3), x=(0, 5), y=(0, 3), topology=topo, halo=(3, 2))
    for name, loc in LOCS.items():
        f = csi.Field(loc, g, None, name)
        f.fill_parent(np.nan)
        nx = 5 + (loc[0] is csi.Face and topo[0] is csi.Bounded)
        ny = 3 + (loc[1] is csi.Face and topo[1] is csi.Bounded)
        f.interior().fill_(1.0)
        x = ref.interior(f.numpy(), g.Hx, g.Hy)
        assert x.shape == (ny, nx) and (x == 1.0).all()
        assert np.isnan(f.numpy()).sum() == f.numpy().size - nx * ny


def test_tile_interiors_partition_the_global_field():
    G = csi.RectilinearGrid((8, 6), x=(0, 8), y=(0, 6), topology=(csi.Bounded, csi.Bounded), halo=(2, 2))
    for name, loc in LOCS.items():
        gx, gy = G.interior_size(*loc)
        seen = np.zeros((gy, gx), int)
        for rank in range(4):
            t = csi.TileGrid(G, 2, 2, rank % 2, rank // 2)
            ny, nx = ref.interior(csi.Field(loc, t, None, name).numpy(), t.Hx, t.Hy).shape
            seen[t.j_off:t.j_off + ny, t.i_off:t.i_off + nx] += 1
        assert (seen == 1).all(), name


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def _c_layout(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    exe = tmp_path / "output_layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "output_layout.c"), "-o", str(exe)])
    return {k: int(v) for k, v in (ln.split("=") for ln in subprocess.check_output([str(exe)]).decode().split())}


def test_c_compiler_layout_matches_ctypes(tmp_path):
    got = _c_layout(tmp_path)
    T = L.OutputField
    assert [f[0] for f in T._fields_] == ["field_id", "dtype", "averaged", "masked", "fill_value"]
    assert got["sizeof"] == C.sizeof(T) == 24
    for name, _ in T._fields_:
        assert got["offset_" + name] == getattr(T, name).offset, name
    assert (got["CSI_OUT_F64"], got["CSI_OUT_F32"]) == (L.OUT_F64, L.OUT_F32)
    assert (got["CSI_OUTPUT_MAX_FIELDS"], got["CSI_OUTPUT_MAX_SETS"], got["CSI_OUTPUT_MAX_SLOTS"]) == \
        (L.OUTPUT_MAX_FIELDS, L.OUTPUT_MAX_SETS, L.OUTPUT_MAX_SLOTS)
    assert got["create_result_bytes"] == got["wait_result_bytes"] == 4


def test_c_compiler_layout_matches_julia_stub(tmp_path):
    got = _c_layout(tmp_path)
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    m = re.search(r"^struct\s+CsiOutputField\b[^\n]*\n(.*?)\nend", stub, re.S | re.M)
    assert m, "struct CsiOutputField is missing from the Julia stub"
    size = {"Int32": 4, "Cdouble": 8}
    at = 0
    for name, t in re.findall(r"(\w+)::(\w+)", re.sub(r"#[^\n]*", "", m.group(1))):
        at = -(-at // size[t]) * size[t]
        assert got["offset_" + name] == at, name
        at += size[t]
    assert -(-at // 8) * 8 == got["sizeof"]
    for entry in ("csi_output_create", "csi_output_layout", "csi_output_record_bytes", "csi_output_accumulate", "csi_output_snapshot",
                  "csi_output_wait", "csi_output_release", "csi_output_destroy"):
        assert f"(:{entry}, libcsi)" in stub, entry
    assert "function write_output!(" in stub


def test_symbols_are_exported_and_declared():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "csi.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in L.SYMBOLS and re.search(r"int32_t\s+" + name + r"\(", header), name


def test_entries_refuse_a_null_context():
    """The argument checks that need no device: every entry that takes a context returns CSI_ERR_INVALID_ARGUMENT for NULL."""
    lib = L.load()
    f = (L.OutputField * 1)(L.OutputField(L.F["H"], L.OUT_F32, 0, 0, 0.0))
    i32, i64, vp = C.c_int32(), C.c_int64(), C.c_void_p()
    calls = {"csi_output_create": (f, 1, 2, C.byref(i32)), "csi_output_layout": (1, 0, C.byref(i64), C.byref(i32), C.byref(i32)),
             "csi_output_record_bytes": (1, C.byref(i64)), "csi_output_accumulate": (1, 1.0), "csi_output_snapshot": (1, C.byref(i32)),
             "csi_output_test": (1, 0, C.byref(i32)), "csi_output_wait": (1, 0, C.byref(vp)), "csi_output_release": (1, 0),
             "csi_output_destroy": (1,)}
    assert sorted(calls) == sorted(n for n in ENTRIES if n != "csi_output_plan_layout")
    for name, args in calls.items():
        assert getattr(lib, name)(None, *args) == -1, name
    assert lib.csi_output_plan_layout(None, None, None, 1, None, None) == -1
