"""CPU tests of the Lagrangian ice drifters (include/csi.h, "Lagrangian ice drifters"): csi_drifters_locate and a host build of the
sub-step of csrc/drifters_dev.h (tests/drifters_host.cpp, g++) bit for bit against the NumPy restatement tests/drifters_ref.py;
properties of the restatement that a wrong rule would break, with how far each of four mistakes moves the answer; the sanitized
stand-alone program; the struct as gcc, ctypes and the Julia stub lay it out; the Python front end.  Nothing here needs a GPU."""
import ctypes as C
import json
import os
import re
import subprocess
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import climaseaice_jl_amd as csi
import drifters_cases as dc
import drifters_ref as ref

L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaseaice.jl_amd", "csrc")
HOST_SRC = os.path.join(ROOT, "tests", "drifters_host.cpp")
EPS = 2.0 ** -53          # unit roundoff: every +, -, *, / is off by at most EPS relative


# ---- the C rule against the restatement ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("drifters") / "libdrifters_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, HOST_SRC, "-o", so])
    lib = C.CDLL(so)
    dp, lg = C.POINTER(C.c_double), C.c_long
    lib.drifters_host_advance.argtypes = [C.c_int] * 6 + [dp, lg, dp, lg, dp, dp, lg, C.c_void_p, lg, dp, dp, C.POINTER(C.c_int32), C.c_double, C.c_int]
    return lib


def host_advance(lib, G, u, v, xi, eta, tau, m):
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    xi, eta = np.array(xi, dtype=np.float64), np.array(eta, dtype=np.float64)
    st = np.full(xi.size, -1, dtype=np.int32)
    dxfc, dycf = np.ascontiguousarray(G.dxfc), np.ascontiguousarray(G.dycf)
    mask = None if G.active is None else np.ascontiguousarray(G.active, dtype=np.uint8)
    lib.drifters_host_advance(G.Nx, G.Ny, G.Hx, G.Hy, int(G.periodic_x), int(G.periodic_y), ptr(u), u.shape[1], ptr(v), v.shape[1], ptr(dxfc), ptr(dycf),
                              dxfc.shape[1], None if mask is None else mask.ctypes.data, xi.size, ptr(xi), ptr(eta),
                              st.ctypes.data_as(C.POINTER(C.c_int32)), float(tau), int(m))
    return xi, eta, st


def test_locate_matches_the_restatement_on_the_edge_table():
    Nx, Ny = 37, 29
    X, Y = ref.edge_positions(Nx, Ny)
    want = ref.locate(Nx, Ny, X, Y)
    for q in range(X.size):
        got = L.drifters_locate(Nx, Ny, X[q], Y[q])
        for k in ("ia", "ja", "ib", "jb", "ic", "jc"):
            assert got[k] == want[k][q], (k, X[q], Y[q])
        for k in ("sx", "sy", "rx", "ry"):
            assert dc.same_bits(np.float64(got[k]), want[k][q]), (k, X[q], Y[q])
        # the one ring, whatever the position holds
        assert 1 <= got["ia"] <= Nx and 0 <= got["ja"] <= Ny and 0 <= got["ib"] <= Nx and 1 <= got["jb"] <= Ny
        assert 1 <= got["ic"] <= Nx and 1 <= got["jc"] <= Ny
    # two rows of the table, stated: on the last face the last column pair with weight 1; the halo rows
    s = L.drifters_locate(Nx, Ny, float(Nx), 0.25)
    assert (s["ia"], s["sx"], s["ja"], s["sy"]) == (Nx, 1.0, 0, 0.75)
    s = L.drifters_locate(Nx, Ny, 12.0, Ny - 0.25)
    assert (s["ia"], s["sx"], s["ja"], s["sy"], s["jb"], s["ry"]) == (13, 0.0, Ny, 0.25, Ny, 0.75)
    with pytest.raises(csi.CsiError):
        L.drifters_locate(0, 5, 1.0, 1.0)


@pytest.mark.parametrize("topo", ["pp", "bb", "pb"])
@pytest.mark.parametrize("kind", dc.KINDS)
def test_host_build_of_the_sub_step_matches_the_restatement_bit_for_bit(host_lib, topo, kind):
    g = dc.make_grid(37, 29, topo, kind)
    u, v = dc.parents(g, seed=3)
    ex, ey = ref.edge_positions(g.Nx, g.Ny)
    rx, ry = dc.positions(g, 300, seed=1)
    xi, eta = np.concatenate([ex, rx]), np.concatenate([ey, ry])
    bits = 0
    for active in (None, dc.land(g, seed=2)):
        G = dc.ref_grid(g, active)
        for tau, m in ((900.0, 1), (2500.0, 3), (-1700.0, 2), (0.0, 1), (4e6, 1)):
            want = ref.advance(G, u, v, xi, eta, tau * m, m)
            got = host_advance(host_lib, G, u, v, xi, eta, tau, m)
            assert dc.same_bits(got[0], want[0]) and dc.same_bits(got[1], want[1]), (tau, m)
            assert np.array_equal(got[2], want[2]), (tau, m)
            bits |= int(np.bitwise_or.reduce(want[2]))
            # NaN / Inf rows are INACTIVE and untouched; the rows that are finite stay finite or are lost as (NaN, NaN)
            inactive = ~(np.isfinite(xi) & np.isfinite(eta))
            assert np.all(want[2][inactive] == ref.INACTIVE) and dc.same_bits(want[0][inactive], xi[inactive])
            lost = (want[2] & ref.LOST) != 0
            assert np.all(np.isnan(want[0][lost]) & np.isnan(want[1][lost])) and not np.any(lost & inactive)
    # every status bit the topology allows occurs (a Periodic direction never clamps)
    assert bits == 31 - (ref.CLAMPED_X if topo[0] == "p" else 0) - (ref.CLAMPED_Y if topo[1] == "p" else 0)


def test_periodic_norm_edge_values():
    N = 37
    r, _ = ref.norm(np.array([-1e-17, N + 1e-13, float(N), 0.0, -0.25, 2.0 * N + 3.0, np.nan, np.inf, 1e300, -1e300]), N, True)
    assert r[0] == 0.0                                   # x - N * floor(x / N) rounds to exactly N: the seam
    assert -1e-17 + N == N                               # (that rounding, checked here)
    assert 0 < r[1] < 1e-12 and r[2] == 0.0 and r[3] == 0.0 and r[4] == N - 0.25 and r[5] == 3.0
    assert np.isnan(r[6]) and np.isnan(r[7]) and 0 <= r[8] < N and 0 <= r[9] < N
    raw, _ = ref.norm(np.array([-1e-17]), N, True, wrap_rule=False)
    assert raw[0] == N                                   # the mistake "norm without the >= N -> 0 rule" leaves the drifter ON the far edge
    b, c = ref.norm(np.array([-0.5, 0.0, 3.0, float(N), N + 1e-13, np.nan, np.inf]), N, False)
    assert list(b[:5]) == [0.0, 0.0, 3.0, N, N] and np.isnan(b[5]) and b[6] == N
    assert list(c) == [True, False, False, False, True, False, True]


# ---- properties of the restatement ---------------------------------------------------------------------------------------------------------

def test_uniform_flow_is_exact_over_a_full_wrap():
    """Uniform periodic grid, u * tau / dx = 3/8 and v * tau / dy = -1/4 cells per sub-step, positions on a 1/8 lattice: every product and
    sum of the rule is exact, so after k sub-steps the drifters sit EXACTLY at (x0 + 3k/8) mod Nx, (y0 - k/4) mod Ny, and after 256 they
    are back (256 * 3/8 = 3 Nx, 256 / 4 = 4 Ny at 32 x 16)."""
    g = csi.RectilinearGrid((32, 16), x=(0.0, 32 * 1024.0), y=(0.0, 16 * 512.0), topology=(csi.Periodic, csi.Periodic), halo=(3, 3))
    G = dc.ref_grid(g)
    u = np.full(g.field_size(csi.Face, csi.Center)[::-1], 0.375 * 1024.0 / 64.0)       # tau = 64 s
    v = np.full(g.field_size(csi.Center, csi.Face)[::-1], -0.25 * 512.0 / 64.0)
    rng = np.random.default_rng(0)
    x0, y0 = rng.integers(0, 32 * 8, 200) / 8.0, rng.integers(0, 16 * 8, 200) / 8.0
    xi, eta = x0.copy(), y0.copy()
    for k in range(1, 257):
        xi, eta, st = ref.advance(G, u, v, xi, eta, 64.0 * 4, 4) if k % 4 == 0 else (xi, eta, None)
        if st is not None:
            assert np.array_equal(xi, (x0 + 0.375 * k) % 32.0) and np.array_equal(eta, (y0 - 0.25 * k) % 16.0), k
            assert not st.any()
    assert np.array_equal(xi, x0) and np.array_equal(eta, y0)


def _rotation(N=32, omega=1e-4, d=1000.0):
    """A rigid rotation about the centre of a Bounded uniform N x N grid with dx = dy = d: u = -omega (y - yc), v = omega (x - xc) at
    their own nodes, halo ring included: A = -omega (eta - N/2), B = omega (xi - N/2), linear in the index-space position."""
    g = csi.RectilinearGrid((N, N), x=(0.0, N * d), y=(0.0, N * d), topology=(csi.Bounded, csi.Bounded), halo=(3, 3))
    G = dc.ref_grid(g)
    nu, nv = g.field_size(csi.Face, csi.Center), g.field_size(csi.Center, csi.Face)
    ju = np.arange(nu[1])[:, None] - (g.Hy - 1)          # row index j of u: y = (j - 1/2) d
    iv = np.arange(nv[0])[None, :] - (g.Hx - 1)          # column index i of v: x = (i - 1/2) d
    u = np.broadcast_to(-omega * ((ju - 0.5) * d - N * d / 2), nu[::-1]).copy()
    v = np.broadcast_to(omega * ((iv - 0.5) * d - N * d / 2), nv[::-1]).copy()
    return G, u, v


def test_rigid_rotation_one_midpoint_step_multiplies_r2_by_one_plus_theta4_over_4():
    """Staggered bilinear interpolation is exact on a linear field, so one midpoint step is r' = (1 + theta J + theta^2 J^2 / 2) r with
    J the quarter turn: |r'|^2 = ((1 - theta^2 / 2)^2 + theta^2) |r|^2 = (1 + theta^4 / 4) |r|^2.  Forward Euler gives 1 + theta^2.

    Rounding bound, first order in EPS = 2^-53, N = 32, R = N / 2 the largest |xi - N/2|:
      a stored u, v:       3 roundings of the form (j - 1/2) d - N d / 2 times omega      relative 3 EPS of |A| <= omega R
      A = u / dx:          1                                                             -> each A, B within 4 EPS omega R
      the bilinear form:   1 - s, a product, a sum, a product, a sum per value           -> 5 EPS omega R more: |da| <= 9 EPS omega R
      eta - 1/2, xi - fx:  exact here (positions are multiples of 2^-40 in [2, 30])
      a stage:             tau * a (1), xi + ... (1, of |xi| <= N)                         -> |d xi| <= tau |da| + EPS (theta R + N)
      two stages:          the midpoint's error enters the second rate times theta       -> |d xi'| <= (1 + theta)(9 theta R + theta R + N) EPS
    so each coordinate is within D = (1 + theta)(10 theta R + N) EPS of the exact map, |r'|^2 within 2 sqrt(2) |r'| D + O(EPS^2), and the
    test's own r^2, ratio and 1 + theta^4 / 4 add 6 EPS relative.  With r >= 4: bound = 2 sqrt(2) (1 + theta) D / (4 EPS) + 6, in EPS."""
    N, omega, tau = 32, 1e-4, 3000.0
    theta = omega * tau                                   # 0.3
    G, u, v = _rotation(N, omega)
    rng = np.random.default_rng(1)
    ang, rad = rng.random(400) * 2 * np.pi, 4.0 + 8.0 * rng.random(400)
    q = 2.0 ** -40
    xi, eta = np.round((N / 2 + rad * np.cos(ang)) / q) * q, np.round((N / 2 + rad * np.sin(ang)) / q) * q
    r2 = (xi - N / 2) ** 2 + (eta - N / 2) ** 2
    x1, y1, st = ref.advance(G, u, v, xi, eta, tau, 1)
    assert not st.any()
    ratio = ((x1 - N / 2) ** 2 + (y1 - N / 2) ** 2) / r2
    R = N / 2
    D = (1 + theta) * (10 * theta * R + N)
    bound = (2 * np.sqrt(2) * (1 + theta) * D / 4.0 + 6) * EPS
    err = np.abs(ratio - (1 + theta ** 4 / 4)).max()
    print(f"rigid rotation: max |r'^2 / r^2 - (1 + theta^4 / 4)| = {err:.3e} = {err / EPS:.1f} EPS (bound {bound / EPS:.1f} EPS)")
    assert err <= bound
    # MISTAKE: forward Euler for the midpoint rule: 1 + theta^2
    a, b = ref.rate(G, u, v, xi, eta)
    xe, ye = xi + tau * a, eta + tau * b
    euler = np.abs(((xe - N / 2) ** 2 + (ye - N / 2) ** 2) / r2 - (1 + theta ** 4 / 4)).max()
    print(f"mistake, Euler for midpoint: {euler:.3e} = {euler / bound:.3g} bounds")
    assert euler > 1e9 * bound and abs(euler - (theta ** 2 - theta ** 4 / 4)) < 1e-12


def test_linear_rate_field_on_a_distorted_grid_is_interpolated_exactly():
    """A(xi, eta) = a0 + a1 xi + a2 eta at the u points and B likewise at the v points, turned into velocities with the distorted grid's
    dx^fc and dy^cf: the rule divides them out again, and the bilinear form of a linear field is the field.  Bound, first order: u = A dx
    (1 rounding, A itself 4 from its formula), u / dx (1), the bilinear form (5 as above): 11 EPS of max |A|; x 2 for slack in the weights'
    own rounding near faces: 22 EPS max |A|."""
    g = dc.make_grid(37, 29, "bb", "full")
    G = dc.ref_grid(g)
    m = g.metrics()
    shape = G.dxfc.shape
    i = np.arange(shape[1])[None, :] - (g.Hx - 1.0)
    j = np.arange(shape[0])[:, None] - (g.Hy - 1.0)
    coef = (3e-4, 2e-5, -1.5e-5)
    lin = lambda x, y: coef[0] + coef[1] * x + coef[2] * y      # noqa: E731
    nu, nv = g.field_size(csi.Face, csi.Center), g.field_size(csi.Center, csi.Face)
    u = (lin(i - 1.0, j - 0.5) * m["dxfc"])[:nu[1], :nu[0]].copy()
    v = (lin(i - 0.5, j - 1.0) * m["dycf"])[:nv[1], :nv[0]].copy()
    xi, eta = dc.positions(g, 500, seed=4)
    a, b = ref.rate(G, u, v, xi, eta)
    amax = np.abs(lin(i, j)).max()
    bound = 22 * EPS * amax
    err = max(np.abs(a - lin(xi, eta)).max(), np.abs(b - lin(xi, eta)).max())
    print(f"linear field, distorted grid: max error {err:.3e} = {err / (EPS * amax):.2f} EPS max|A| (bound 22)")
    assert err <= bound
    # MISTAKE: dx^cc for dx^fc
    wrong = ref.RefGrid(g.Nx, g.Ny, g.Hx, g.Hy, False, False, m["dxcc"], m["dycf"])
    e1 = np.abs(ref.rate(wrong, u, v, xi, eta)[0] - lin(xi, eta)).max()
    print(f"mistake, dx^cc for dx^fc: {e1:.3e} = {e1 / bound:.3g} bounds")
    assert e1 > 1e6 * bound
    # MISTAKE: the half-cell offset of eta dropped for u (t = eta instead of eta - 1/2): the A form evaluated half a cell higher
    inner = (eta > 1) & (eta < g.Ny - 1)
    e2 = np.abs(ref.rate(G, u, v, xi[inner], eta[inner] + 0.5)[0] - lin(xi[inner], eta[inner])).max()
    print(f"mistake, half-cell offset dropped for u: {e2:.3e} = {e2 / bound:.3g} bounds")
    assert e2 > 1e6 * bound and abs(e2 - abs(coef[2]) * 0.5) < 1e-12


def test_land_holds_and_walls_clamp():
    g = csi.RectilinearGrid((8, 6), x=(0.0, 8000.0), y=(0.0, 6000.0), topology=(csi.Bounded, csi.Bounded), halo=(2, 2))
    active = np.ones((6, 8), dtype=bool)
    active[2, 4] = False                                   # cell (5, 3): [4, 5) x [2, 3)
    G = dc.ref_grid(g, active)
    u = np.full(g.field_size(csi.Face, csi.Center)[::-1], 1.0)      # one cell per 1000 s eastward
    v = np.zeros(g.field_size(csi.Center, csi.Face)[::-1])
    xi, eta = np.array([3.5, 3.5, 7.5, 0.25]), np.array([2.5, 3.5, 1.0, 5.0])
    x, y, st = ref.advance(G, u, v, xi, eta, 1000.0, 1)
    assert list(x) == [3.5, 4.5, 8.0, 1.25] and list(y) == list(eta)
    assert list(st) == [ref.HELD, 0, ref.CLAMPED_X, 0]
    # each sub-step is judged on its own: two half steps -- the first lands at 4.0, inside the land cell [4, 5): held twice
    x, y, st = ref.advance(G, u, v, xi, eta, 1000.0, 2)
    assert x[0] == 3.5 and st[0] == ref.HELD and x[2] == 8.0 and st[2] == ref.CLAMPED_X
    # a drifter that would jump OVER the land cell is not held: the rule looks at where it lands
    x, y, st = ref.advance(G, u, v, xi[:1], eta[:1], 2000.0, 1)
    assert x[0] == 5.5 and st[0] == 0
    # -u: the western wall
    x, y, st = ref.advance(G, -u, v, xi, eta, 1000.0, 1)
    assert x[3] == 0.0 and st[3] == ref.CLAMPED_X and x[1] == 2.5


# ---- the sanitized stand-alone program -----------------------------------------------------------------------------------------------------

def test_edge_table_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/drifters_host.cpp with its own main: csrc/drifters_dev.h on parents of exactly a model's extents, every edge position at five
    step lengths, three topologies, with and without land, under -fsanitize=address,undefined,float-cast-overflow."""
    exe = str(tmp_path / "drifters_sanitized")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined,float-cast-overflow",
                        "-fno-sanitize-recover=all", "-DDRIFTERS_HOST_MAIN", "-I" + CSRC, HOST_SRC, "-o", exe], capture_output=True, text=True)
    if p.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", p.stderr):
        pytest.skip("sanitizer_runtime_missing: g++ has no address / undefined-behaviour sanitizer runtime here")
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "status bits seen 31" in r.stdout


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------

def _c_layout(tmp_path):
    exe = str(tmp_path / "drifters_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drifters_layout.c"), "-o", exe])
    return json.loads(subprocess.check_output([exe]).decode())


def test_c_layout_matches_ctypes_and_the_julia_stub(tmp_path):
    got = _c_layout(tmp_path)
    assert got["sizeof_drifters"] == C.sizeof(L.Drifters) == 32
    for name, _ in L.Drifters._fields_:
        assert got[f"csi_drifters.{name}"] == getattr(L.Drifters, name).offset, name
    for n in ("CLAMPED_X", "CLAMPED_Y", "HELD", "LOST", "INACTIVE"):
        assert got["CSI_DRIFTER_" + n] == getattr(L, "DRIFTER_" + n) == getattr(ref, n)
    for k, n in enumerate(("XI", "ETA", "U", "V", "H", "A", "HS")):
        assert got["CSI_DRIFTER_COL_" + n] == getattr(L, "DRIFTER_COL_" + n) == 1 << k
    assert got["CSI_DRIFTER_COL_ALL"] == L.DRIFTER_COL_ALL == 127 and got["CSI_VERSION"] == 100
    from climaseaice_jl_amd.drifters import COLUMNS
    assert COLUMNS == ref.COLUMNS
    # the stub: the struct laid out by C's rules, the constants, the three ccalls
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    body = re.search(r"^struct CsiDrifters\n(.*?)\nend", stub, re.S | re.M).group(1)
    fields = re.findall(r"(\w+)::((?:Ptr\{\w+\})|\w+)", body)
    size = {"Int64": 8, "Int32": 4, "Cdouble": 8}
    off, offsets = 0, {}
    for name, t in fields:
        s = 8 if t.startswith("Ptr{") else size[t]
        off = (off + s - 1) // s * s
        offsets[name] = off
        off += s
    assert offsets == {n: got[f"csi_drifters.{n}"] for n, _ in L.Drifters._fields_} and off == got["sizeof_drifters"]
    for const, prefix in (("DRIFTER_STATUS", "CSI_DRIFTER_"), ("DRIFTER_COLUMNS", "CSI_DRIFTER_COL_")):
        vals = {k: int(x) for k, x in re.findall(r"(\w+)\s*=\s*(\d+)", re.search(r"^const %s = \((.*?)\)" % const, stub, re.M).group(1))}
        assert vals and vals == {k: got[prefix + k] for k in vals}, const
    assert re.search(r"ccall\(\(:csi_drifters_advance, libcsi\), Int32, \(Ptr\{Cvoid\}, Ref\{CsiDrifters\}, Cdouble, Int32\)", stub)
    assert re.search(r"ccall\(\(:csi_drifters_sample, libcsi\), Int32, \(Ptr\{Cvoid\}, Ref\{CsiDrifters\}, Int32, Ptr\{Cvoid\}, Int64\)", stub)
    assert re.search(r"ccall\(\(:csi_drifters_stats, libcsi\), Int32, \(Ptr\{Cvoid\}, Ref\{Int64\}\)", stub)
    assert "function advance_drifters!" in stub


# ---- the front end -------------------------------------------------------------------------------------------------------------------------

def test_seeding_at_cell_centres():
    g = csi.RectilinearGrid((10, 7), x=(0, 1), y=(0, 1))
    d = csi.Drifters.at_cell_centers(g, stride=4)
    xi, eta, st = d.numpy()
    assert list(xi) == [0.5, 4.5, 8.5, 0.5, 4.5, 8.5] and list(eta) == [0.5] * 3 + [4.5] * 3 and not st.any() and st.dtype == np.int32
    where = np.zeros((7, 10), dtype=bool)
    where[4, :] = True
    d = csi.Drifters.at_cell_centers(g, stride=(4, 1), where=where)
    assert list(d.numpy()[0]) == [0.5, 4.5, 8.5] and list(d.numpy()[1]) == [4.5] * 3
    assert csi.Drifters.at_cell_centers(g).n == 70 and csi.Drifters(g, [], []).n == 0
    assert d.status_counts() == dict(free=3, clamped_x=0, clamped_y=0, held=0, lost=0, inactive=0)
    with pytest.raises(ValueError, match="same length"):
        csi.Drifters(g, [1.0], [1.0, 2.0])
    with pytest.raises(ValueError, match="stride"):
        csi.Drifters.at_cell_centers(g, stride=0)


def test_coordinate_round_trip_on_the_two_regular_grids():
    """x -> xi = (x - x0) / dx -> x' = x0 + xi * dx: a difference, a quotient, a product and a sum, each rounded once.  First order:
    |x' - x| <= EPS (3 |x - x0| + |x'|) <= 4 EPS (|x| + |x0|) -- stated per coordinate below."""
    rng = np.random.default_rng(2)
    grids = [csi.RectilinearGrid((37, 29), x=(-2.5e5, 7.1e5), y=(1.0e6, 1.9e6), topology=(csi.Bounded, csi.Bounded)),
             csi.LatitudeLongitudeGrid((64, 16), longitude=(-30, 50), latitude=(55, 85))]
    for g in grids:
        (x0, x1), (y0, y1) = (g.x, g.y) if isinstance(g, csi.RectilinearGrid) else (g.longitude, g.latitude)
        x, y = x0 + (x1 - x0) * rng.random(1000), y0 + (y1 - y0) * rng.random(1000)
        d = csi.Drifters.from_coordinates(g, x, y)
        xi, eta, _ = d.numpy()
        assert xi.min() >= 0 and xi.max() <= g.Nx and eta.min() >= 0 and eta.max() <= g.Ny
        X, Y = d.coordinates()
        assert np.all(np.abs(X - x) <= 4 * EPS * (np.abs(x) + abs(x0))) and np.all(np.abs(Y - y) <= 4 * EPS * (np.abs(y) + abs(y0)))
    # the nodes themselves: cell centre (i, j) is (i - 1/2, j - 1/2)
    g = grids[0]
    d = csi.Drifters.at_cell_centers(g)
    X, Y = d.coordinates()
    assert np.allclose(X[:g.Nx], g.xnodes(csi.Center), rtol=0, atol=4 * EPS * 1e6) and np.allclose(Y[::g.Nx], g.ynodes(csi.Center), rtol=0, atol=8 * EPS * 2e6)


def test_unsupported_grids_and_columns_are_refused_by_name():
    rect = csi.RectilinearGrid((16, 12), x=(0, 1), y=(0, 1), topology=(csi.Periodic, csi.Bounded), halo=(4, 4))
    curv = csi.OrthogonalCurvilinearGrid.from_grid(rect)
    with pytest.raises(NotImplementedError, match="OrthogonalCurvilinearGrid"):
        csi.Drifters.from_coordinates(curv, [0.5], [0.5])
    with pytest.raises(NotImplementedError, match="OrthogonalCurvilinearGrid"):
        csi.Drifters(curv, [0.5], [0.5]).coordinates()
    with pytest.raises(NotImplementedError, match="migrate between ranks"):
        csi.Drifters(csi.TileGrid(rect, 1, 2, 0, 0), [0.5], [0.5])
    folded = csi.RectilinearGrid((16, 12), x=(0, 1), y=(0, 1), topology=(csi.Periodic, csi.RightFolded), halo=(4, 4))
    with pytest.raises(NotImplementedError, match="fold re-orients"):
        csi.Drifters(folded, [0.5], [0.5])
    from climaseaice_jl_amd.drifters import column_mask, columns_of
    assert column_mask(["v", "xi", "aice"]) == 1 + 8 + 32 and columns_of(41) == ["xi", "v", "aice"]
    with pytest.raises(ValueError, match="'shear'"):
        column_mask(["xi", "shear"])
    d = csi.Drifters(rect, [0.5], [0.5])
    with pytest.raises(NotImplementedError, match="time averages"):
        csi.DrifterWriter(d, csi.AveragedTimeInterval(1.0), "unused")
    other = SimpleNamespace(grid=csi.RectilinearGrid((8, 8), x=(0, 1), y=(0, 1)), device="cpu")
    with pytest.raises(ValueError, match="another grid"):
        d.advance(other, 1.0)


def _fake_model(g, seed=0):
    """A model-like object on the CPU, as tests/test_output_frontend.py makes them for the stand-in recorder of tests/output_ref.py: .grid,
    .clock, .fields (name -> Field), .output_writers."""
    rng = np.random.default_rng(seed)
    fields = OrderedDict()
    for n, loc in (("u", (csi.Face, csi.Center)), ("v", (csi.Center, csi.Face)), ("h", (csi.Center, csi.Center)), ("aice", (csi.Center, csi.Center))):
        f = csi.Field(loc, g, None, n)
        f.data.copy_(torch.from_numpy(rng.random(tuple(f.data.shape))))
        fields[n] = f
    return SimpleNamespace(grid=g, clock=SimpleNamespace(time=0.0, iteration=0), fields=fields, output_writers=OrderedDict(), drifters=None)


def test_writer_on_a_stand_in_model(tmp_path):
    """DrifterWriter driven through the begin / after_step protocol, its records taken by a NumPy stand-in for the device call (the
    restatement's sample on the model's CPU fields, as tests/output_ref.py stands in for the device recorder): growable files that are
    valid after every record, one row per drifter, rows in COLUMNS order whatever order was asked for."""
    g = csi.RectilinearGrid((12, 9), x=(0.0, 12e3), y=(0.0, 9e3), topology=(csi.Periodic, csi.Bounded), halo=(2, 2))
    m = _fake_model(g)
    G = dc.ref_grid(g)
    d = csi.Drifters.at_cell_centers(g, stride=4)

    def sampler(drifters, model, names):
        xi, eta, _ = drifters.numpy()
        return ref.sample(G, {k: f.numpy() for k, f in model.fields.items()}, xi, eta, names)

    w = csi.DrifterWriter(d, csi.IterationInterval(2), str(tmp_path / "tracks"), columns=("h", "xi", "u", "eta"), sampler=sampler)
    m.output_writers["tracks"] = w
    want = []
    for step in range(5):
        for x in m.output_writers.values():
            x.begin(m)
        if step == 0:
            want.append(sampler(d, m, w.names))
        xi, eta, st = ref.advance(G, m.fields["u"].numpy(), m.fields["v"].numpy(), *d.numpy()[:2], 700.0, 2)
        d.restore({"drifters.xi": xi, "drifters.eta": eta, "drifters.status": st})
        m.clock.time += 700.0
        m.clock.iteration += 1
        for x in m.output_writers.values():
            x.after_step(m, 700.0)
        if m.clock.iteration % 2 == 0:
            want.append(sampler(d, m, w.names))
        got = np.load(str(tmp_path / "tracks" / "xi.npy"))            # valid after every record
        assert got.shape == (len(want), d.n)
    w.close()
    assert w.names == ["xi", "eta", "u", "h"] and w.records == 3
    out = csi.load_tracks(str(tmp_path / "tracks"))
    assert list(out["iteration"]) == [0, 2, 4] and list(out["time"]) == [0.0, 1400.0, 2800.0] and out["status"].dtype == np.int32
    for k, name in enumerate(w.names):
        assert dc.same_bits(out[name], np.array([r[k] for r in want])), name
    assert not np.array_equal(out["xi"][0], out["xi"][2])
    with pytest.raises(FileExistsError):
        csi.DrifterWriter(d, csi.IterationInterval(2), str(tmp_path / "tracks"))


def test_checkpoint_carries_the_drifters_only_when_they_are_set():
    g = csi.RectilinearGrid((12, 9), x=(0.0, 12e3), y=(0.0, 9e3), halo=(2, 2))
    fm = _fake_model(g)
    f = fm.fields
    m = SimpleNamespace(grid=g, clock=fm.clock, velocities=SimpleNamespace(u=f["u"], v=f["v"]), ice_thickness=f["h"], ice_concentration=f["aice"],
                        snow_thickness=None, timestepper=SimpleNamespace(Gn=SimpleNamespace(), Psi_minus=None), dynamics=None, mass_fluxes=None,
                        ocean=None, drifters=None, synchronize=lambda: None)
    m.copy_to_field = lambda fld, a: fld.data.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    keys = set(csi.prognostic_state(m))
    assert not any(k.startswith("drifters") for k in keys)
    m.drifters = csi.Drifters(g, [1.5, 2.25, np.nan], [3.0, 0.5, 1.0])
    m.drifters.status[1] = ref.HELD
    state = csi.prognostic_state(m)
    assert set(state) == keys | {"drifters.xi", "drifters.eta", "drifters.status"}
    m.drifters.xi[:] = 0.0
    m.drifters.status[:] = 0
    csi.restore_prognostic_state(m, state)
    xi, eta, st = m.drifters.numpy()
    assert dc.same_bits(xi, np.array([1.5, 2.25, np.nan])) and list(eta) == [3.0, 0.5, 1.0] and list(st) == [0, ref.HELD, 0]
    # an older checkpoint without drifters restores the fields and leaves the drifters alone
    csi.restore_prognostic_state(m, {k: v for k, v in state.items() if not k.startswith("drifters")})
    assert list(m.drifters.numpy()[2]) == [0, ref.HELD, 0]
    with pytest.raises(ValueError, match="drifters.xi has 2 entries"):
        csi.restore_prognostic_state(m, dict(state, **{"drifters.xi": np.zeros(2)}))
