"""Prescribed free-drift velocity fields (`free_drift = (u, v)`) and StressBalanceFreeDrift as the model's dynamics, CPU suite: the
public interface, the ABI (header, ctypes binding, Julia stub, exported symbols), properties of the test-side restatement
(tests/free_drift_ref.py) on the CPU oracle and the generated code of the new kernel.  Nothing here needs a GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
from free_drift_ref import FreeDriftRef, free_drift_arrays, marginal_band

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "csi.h")
STUB = os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl")


def _grid(topo=(csi.Periodic, csi.Periodic)):
    return csi.RectilinearGrid((12, 10), x=(0.0, 12e3), y=(0.0, 10e3), topology=topo, halo=(4, 4))


# ---- public interface --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topo", [(csi.Periodic, csi.Periodic), (csi.Bounded, csi.Bounded)], ids=["periodic", "walls"])
def test_prescribed_free_drift_fields_are_accepted_in_every_value_form(topo):
    g = _grid(topo)
    nxu, nyu = g.interior_size(csi.Face, csi.Center)
    nxv, nyv = g.interior_size(csi.Center, csi.Face)
    au, av = np.full((nyu, nxu), 0.03), np.full((nyv, nxv), -0.01)
    fu, fv = csi.XFaceField(g, None, "fdu"), csi.YFaceField(g, None, "fdv")
    forms = [dict(u=0.05, v=-0.02), dict(u=au, v=av), dict(u=fu, v=fv), dict(u=au, v=0.0), (au, av), (0.1, fv)]
    for fd in forms:
        d = csi.SeaIceMomentumEquation(g, free_drift=fd)
        assert isinstance(d.free_drift, csi.FreeDriftVelocities)
        want = (fd["u"], fd["v"]) if isinstance(fd, dict) else fd
        assert d.free_drift.u is want[0] and d.free_drift.v is want[1]           # stored as given
    # every solver / rheology takes it
    for kw in (dict(rheology=csi.ViscousRheology(nu=10.0)), dict(solver=csi.ExplicitSolver())):
        assert isinstance(csi.SeaIceMomentumEquation(g, free_drift=dict(u=au, v=av), **kw).free_drift, csi.FreeDriftVelocities)


def test_prescribed_free_drift_fields_of_the_wrong_kind_are_refused_by_name():
    g = _grid()
    with pytest.raises(ValueError, match=r"free_drift\.u.*interior shape"):
        csi.SeaIceMomentumEquation(g, free_drift=dict(u=np.zeros((3, 3)), v=0.0))
    with pytest.raises(ValueError, match=r"free_drift\.v.*field at"):
        csi.SeaIceMomentumEquation(g, free_drift=dict(u=0.0, v=csi.XFaceField(g, None, "wrong location")))
    with pytest.raises(ValueError, match="keys 'u' and 'v'"):
        csi.SeaIceMomentumEquation(g, free_drift=dict(u=0.0))
    with pytest.raises(TypeError, match=r"free_drift\.u"):
        csi.SeaIceMomentumEquation(g, free_drift=dict(u=None, v=0.0))
    with pytest.raises(NotImplementedError, match="free_drift"):
        csi.SeaIceMomentumEquation(g, free_drift="ocean")


def test_none_and_stress_balance_free_drift_behave_as_before():
    g = _grid()
    assert csi.SeaIceMomentumEquation(g).free_drift is None
    fd = csi.StressBalanceFreeDrift()                                      # today's spelling of shape 1: must keep constructing
    assert fd.top_momentum_stress is None and fd.bottom_momentum_stress is None
    assert csi.SeaIceMomentumEquation(g, free_drift=fd).free_drift is fd


def test_stress_balance_free_drift_as_dynamics_checks_the_stresses_where_it_is_used():
    semi = csi.SemiImplicitStress(ue=0.1)
    for top, bottom in (((0.01, 0.0), semi), (semi, (0.0, 0.02)), (None, semi), (dict(u=0.01, v=0.0), semi)):
        d = csi.StressBalanceFreeDrift(top_momentum_stress=top, bottom_momentum_stress=bottom)
        assert d.check_as_dynamics() is d and d.top_momentum_stress is top and d.bottom_momentum_stress is bottom
    # the reference's two messages (stress_balance_free_drift.jl:24-32), raised when used as dynamics, not in the constructor
    both = csi.StressBalanceFreeDrift(top_momentum_stress=semi, bottom_momentum_stress=csi.SemiImplicitStress())
    with pytest.raises(ValueError, match="not both"):
        both.check_as_dynamics()
    for neither in (csi.StressBalanceFreeDrift(), csi.StressBalanceFreeDrift(top_momentum_stress=(0.01, 0.01))):
        with pytest.raises(ValueError, match="requires using a `SemiImplicitStress`"):
            neither.check_as_dynamics()


def test_model_constructor_checks_the_dynamics_before_it_touches_a_device():
    g = _grid()
    with pytest.raises(ValueError, match="requires using a `SemiImplicitStress`"):
        csi.SeaIceModel(g, dynamics=csi.StressBalanceFreeDrift())
    with pytest.raises(NotImplementedError, match="dynamics"):
        csi.SeaIceModel(g, dynamics="free drift")


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def _enum(text, name):
    return int(re.search(name + r"\s*=\s*(\d+)", text).group(1))


def test_header_binding_and_stub_agree_on_the_new_enums_slots_and_prototypes():
    text = open(HEADER).read()
    L = csi._lib
    assert (_enum(text, "CSI_FREE_DRIFT_NONE"), _enum(text, "CSI_FREE_DRIFT_STRESS_BALANCE"), _enum(text, "CSI_FREE_DRIFT_FIELDS")) \
        == (L.FREE_DRIFT_NONE, L.FREE_DRIFT_STRESS_BALANCE, L.FREE_DRIFT_FIELDS) == (0, 1, 2)
    assert (_enum(text, "CSI_DYNAMICS_MOMENTUM_EQUATION"), _enum(text, "CSI_DYNAMICS_FREE_DRIFT")) \
        == (L.DYNAMICS_MOMENTUM_EQUATION, L.DYNAMICS_FREE_DRIFT) == (0, 1)
    # the new slots form a third enum numbered from CSI_F_COUNT_ALL on; the two older lists keep their values
    old = len(L.FIELD_IDS) + len(L.THERMO_FIELD_IDS)
    assert L.FREE_DRIFT_FIELD_IDS == ["FREE_DRIFT_U", "FREE_DRIFT_V"]
    assert (L.F["FREE_DRIFT_U"], L.F["FREE_DRIFT_V"]) == (old, old + 1)
    assert [L.F[n] for n in L.FIELD_IDS + L.THERMO_FIELD_IDS] == list(range(old))
    m = re.search(r"typedef enum \{([^}]*)\} csi_free_drift_field_id;", text)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"CSI_F_(\w+)", body) == ["FREE_DRIFT_U", "COUNT_ALL", "FREE_DRIFT_V", "COUNT_TOTAL"]
    assert re.search(r"CSI_F_FREE_DRIFT_U\s*=\s*CSI_F_COUNT_ALL", body)
    assert re.search(r"#define CSI_VERSION 100\b", text)
    for name, nargs in {"csi_dynamics_set": 2, "csi_free_drift_set": 2}.items():
        m = re.search(r"int32_t\s+" + name + r"\(([^)]*)\)", text)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in L.SYMBOLS
    # the Julia stub: the same slot numbers, kind 2 for a NamedTuple, the dynamics kind, and no silent fall-through to kind 0
    stub = open(STUB, encoding="utf-8").read()
    assert int(re.search(r"FREE_DRIFT_U=(\d+)", stub).group(1)) == L.F["FREE_DRIFT_U"]
    assert int(re.search(r"FREE_DRIFT_V=(\d+)", stub).group(1)) == L.F["FREE_DRIFT_V"]
    assert int(re.search(r"TOP_HEAT_FLUX=(\d+)", stub).group(1)) == L.F["TOP_HEAT_FLUX"]
    assert re.search(r"set_free_drift!\(ctx, fd::NamedTuple\)", stub) and re.search(r"set_free_drift_kind!\(ctx, 2\)", stub)
    assert re.search(r"set_free_drift!\(ctx, fd\) = error\(", stub)
    assert "isa StressBalanceFreeDrift ? 1 : 0" not in stub
    assert re.search(r"time_step_momentum!\(model, dynamics::StressBalanceFreeDrift, Δt\)", stub)
    assert re.search(r":csi_dynamics_set, libcsi\), Int32, \(Ptr\{Cvoid\}, Int32\), ctx\.handle, 1\)", stub)


def test_library_exports_the_new_entry_point():
    L = csi._lib.load()
    assert L.csi_dynamics_set.argtypes is not None and len(L.csi_dynamics_set.argtypes) == 2


def test_c_compiler_sees_the_new_slots_after_the_old_ones(tmp_path):
    """tests/free_drift_layout.c compiled with gcc against include/csi.h: the values a C client gets for the new enumerators."""
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    exe = tmp_path / "free_drift_layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "free_drift_layout.c"), "-o", str(exe)])
    got = dict(ln.split("=") for ln in subprocess.check_output([str(exe)]).decode().split())
    L = csi._lib
    assert int(got["CSI_F_COUNT"]) == len(L.FIELD_IDS) and int(got["CSI_F_COUNT_ALL"]) == len(L.FIELD_IDS) + len(L.THERMO_FIELD_IDS)
    assert int(got["CSI_F_FREE_DRIFT_U"]) == L.F["FREE_DRIFT_U"] and int(got["CSI_F_FREE_DRIFT_V"]) == L.F["FREE_DRIFT_V"]
    assert int(got["CSI_F_COUNT_TOTAL"]) == len(L.F)
    assert (int(got["CSI_FREE_DRIFT_FIELDS"]), int(got["CSI_DYNAMICS_FREE_DRIFT"]), int(got["CSI_VERSION"])) == (2, 1, 100)


# ---- properties of the restatement (CPU oracle underneath) ---------------------------------------------------------------------------
def _problem(free_drift=True, **kw):
    c = cases.make_case(free_drift=free_drift, **kw)
    return c, cases.oracle_problem(c)


def test_zero_explicit_stress_gives_the_external_velocity_bit_for_bit(oracle_lib):
    c, p = _problem(Nx=14, Ny=12, top=None, ue=0.05, ve=-0.02, random_uv=0.03)
    r = FreeDriftRef(p, dynamics=True)
    assert np.all(r.explicit_stress_magnitude("u") == 0.0)
    r.free_drift_dynamics_step()
    assert np.all(p.interior("u") == 0.05) and np.all(p.interior("v") == -0.02)
    # ... also with array-valued external velocities: the field-forcing case with its stress arrays zeroed
    c = cases.make_case(Nx=14, Ny=12, topo=("periodic", "bounded"), field_forcing=True, free_drift=True)
    c["top_u"][...] = 0.0
    c["top_v"][...] = 0.0
    p = cases.oracle_problem(c)
    FreeDriftRef(p, dynamics=True).free_drift_dynamics_step()
    Ny = c["Ny"]                               # (the step writes rows 1 .. Ny: the wall faces of row Ny + 1 keep their state)
    assert np.array_equal(p.interior("u"), c["ue_f"]) and np.array_equal(p.interior("v")[:Ny], c["ve_f"][:Ny])


@pytest.mark.parametrize("kw", [dict(), dict(topo=("periodic", "bounded"), field_forcing=True, land=0.15),
                                dict(topo=("periodic", "bounded"), wind_drag="arrays", bottom="arrays")], ids=["numbers", "arrays_land", "top_semi"])
def test_dynamics_step_does_not_depend_on_the_incoming_velocities(kw, oracle_lib):
    out = []
    for seed_uv in (0.0, 0.2):
        c, p = _problem(Nx=14, Ny=12, random_uv=seed_uv, u0=0.1 + seed_uv, **kw)
        FreeDriftRef(p, dynamics=True).free_drift_dynamics_step()
        out.append((p.f["u"].copy(), p.f["v"].copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.abs(out[0][0]).max() > 0 and np.abs(out[0][1]).max() > 0


def test_dynamics_step_on_a_fold_satisfies_the_folds_symmetry(oracle_lib):
    c, p = _problem(Nx=16, Ny=12, topo=("periodic", "folded"), field_forcing=True)
    FreeDriftRef(p, dynamics=True).free_drift_dynamics_step()
    s = p.s
    Nx, Ny, Hx, Hy = s.Nx, s.Ny, s.Hx, s.Hy
    at = lambda a, i, j: a[j + Hy - 1, i + Hx - 1]
    u, v = p.f["u"], p.f["v"]
    # include/csi.h CSI_RIGHT_FOLDED: u (Face, Center): u[i, Ny + k] = -u[Nx - i + 2, Ny - k]; v (Center, Face): v[i, Ny + k] = -v[Nx - i + 1, Ny - k + 1]
    for k in range(1, Hy + 1):
        for i in range(2, Nx + 1):
            assert at(u, i, Ny + k) == -at(u, Nx - i + 2, Ny - k), (i, k)
        for i in range(1, Nx + 1):
            assert at(v, i, Ny + k) == -at(v, Nx - i + 1, Ny - k + 1), (i, k)
    assert np.abs(p.interior("u")).max() > 0


def test_prescribed_fields_reach_exactly_the_marginal_points(oracle_lib):
    """The explicit step of the restatement with prescribed fields: marginal points hold F, the rest does not see it."""
    c = marginal_band(cases.make_case(Nx=24, Ny=20, random_uv=0.03))
    p = cases.oracle_problem(c)
    rng = np.random.default_rng(4)
    Fu, Fv = 0.04 * rng.standard_normal(p.f["u"].shape), 0.04 * rng.standard_normal(p.f["v"].shape)
    r = FreeDriftRef(p, fields=(Fu, Fv), viscous=True)
    mu, mv = r.marginal("u"), r.marginal("v")
    assert mu.mean() >= 0.10 and mv.mean() >= 0.10, (mu.mean(), mv.mean())       # 24 x 20 periodic, rows 8 .. 13 banded
    r.compute_tendencies(60.0)
    r.explicit_step(60.0)
    s = p.s
    inner = (slice(s.Hy, s.Hy + s.Ny), slice(s.Hx, s.Hx + s.Nx))
    assert np.array_equal(p.f["u"][inner][mu], Fu[inner][mu]) and np.array_equal(p.f["v"][inner][mv], Fv[inner][mv])
    assert not np.any(p.f["u"][inner][~mu] == Fu[inner][~mu])


def test_oracle_closed_forms_as_arrays_match_the_pointwise_calls(oracle_lib):
    c, p = _problem(Nx=14, Ny=12, topo=("bounded", "bounded"), ue=0.05, ve=-0.02)
    Fu, Fv = free_drift_arrays(p)
    assert Fu.shape == p.interior("u").shape and Fv.shape == p.interior("v").shape
    assert Fu[3, 4] == p.L.ora_free_drift_u(p.ptr, 5, 4) and Fv[2, 7] == p.L.ora_free_drift_v(p.ptr, 8, 3)


# ---- generated code of the new kernel (hipcc cross-compiles; nothing runs) -----------------------------------------------------------
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("isa")
    path = d / "momentum_free_drift.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-ffp-contract=off",
                        "--cuda-device-only", "-S", os.path.join(ROOT, "climaseaice.jl_amd", "csrc", "momentum_free_drift.hip"), "-o", str(path),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(path).read().split("\n")
    start = next(k for k, ln in enumerate(lines) if re.match(r"^_ZN3csi3mom17k_free_drift_step\S*:", ln))
    end = next(k for k in range(start, len(lines)) if lines[k].strip().startswith("s_endpgm"))
    return lines[start:end + 1], r.stderr


def test_free_drift_step_issues_every_load_before_the_first_wait(kernel_asm):
    body, _ = kernel_asm
    seq = []
    for ln in body:
        t = ln.strip()
        if t.startswith(("global_load", "buffer_load", "flat_load", "scratch_load")):
            seq.append("L")
        elif t.startswith("s_waitcnt") and "vmcnt" in t:
            seq.append("W" + re.search(r"vmcnt\((\d+)\)", t).group(1))
    loads = seq.count("L")
    first_wait = next(k for k, s in enumerate(seq) if s.startswith("W"))
    # tau_x at 4 points, tau_y at 4 points, u_e, v_e: ten operands, all in flight together, none waited for alone
    assert loads == 10 and seq[:first_wait].count("L") == loads, "".join(seq)
    assert sum(1 for a, b in zip(seq, seq[1:]) if a == "L" and b == "W0") == 0


def test_free_drift_step_uses_no_scratch_and_no_lds(kernel_asm):
    body, remarks = kernel_asm
    get = lambda key: int(re.search(key + r"[^:]*:\s*(\d+)", remarks).group(1))
    assert get("ScratchSize") == 0 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0 and get("LDS Size") == 0
    assert get(r"Occupancy \[waves/SIMD\]") == 8
    assert not any(ln.strip().startswith(("scratch_", "ds_")) for ln in body)
