"""ViscousRheology and the ExplicitSolver, CPU suite: the public interface, the ABI, the test-side restatement
(tests/momentum_ref.py) and the generated code of the new FAST kernels.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
import climaseaice_jl_amd as csi
from momentum_ref import Ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "csi.h")


def _grid(topo=(csi.Periodic, csi.Periodic)):
    return csi.RectilinearGrid((12, 10), x=(0.0, 12e3), y=(0.0, 10e3), topology=topo, halo=(4, 4))


# ---- public interface --------------------------------------------------------------------------------------------------------------
def test_viscous_rheology_constructs_without_auxiliary_fields():
    g = _grid()
    d = csi.SeaIceMomentumEquation(g, rheology=csi.ViscousRheology(nu=1000))
    assert isinstance(d.rheology, csi.ViscousRheology) and d.rheology.nu == 1000.0
    assert vars(d.auxiliaries.fields) == {}                    # Auxiliaries(::ViscousRheology) = NamedTuple(), Rheologies.jl:33
    assert isinstance(d.solver, csi.SplitExplicitSolver) and d.solver.substeps == 150
    assert csi.ViscousRheology().nu == 1000.0                  # viscous_rheology.jl:9 default


def test_explicit_solver_constructs_for_both_rheologies():
    g = _grid()
    for rheo in (None, csi.ViscousRheology(nu=10.0)):
        d = csi.SeaIceMomentumEquation(g, rheology=rheo, solver=csi.ExplicitSolver())
        assert isinstance(d.solver, csi.ExplicitSolver)
    evp = csi.SeaIceMomentumEquation(g, solver=csi.ExplicitSolver())
    assert len(vars(evp.auxiliaries.fields)) == 10             # EVP keeps its ten fields


def test_field_valued_nu_is_refused_by_name():
    g = _grid()
    with pytest.raises(NotImplementedError, match="nu must be a Number"):
        csi.ViscousRheology(nu=csi.CenterField(g, None, "nu"))
    with pytest.raises(NotImplementedError, match="function"):
        csi.ViscousRheology(nu=lambda x, y: 1.0)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_new_enums_slots_and_prototypes():
    text = open(HEADER).read()
    enum = lambda name: int(re.search(name + r"\s*=\s*(\d+)", text).group(1))
    assert (enum("CSI_RHEOLOGY_EVP"), enum("CSI_RHEOLOGY_VISCOUS")) == (csi._lib.RHEOLOGY_EVP, csi._lib.RHEOLOGY_VISCOUS) == (0, 1)
    assert (enum("CSI_SOLVER_SPLIT_EXPLICIT"), enum("CSI_SOLVER_EXPLICIT")) == (csi._lib.SOLVER_SPLIT_EXPLICIT, csi._lib.SOLVER_EXPLICIT) == (0, 1)
    ids = csi._lib.FIELD_IDS
    assert ids[-2:] == ["GU", "GV"] and ids.index("GU") == ids.index("FORCING_V") + 1      # appended after CSI_F_FORCING_V
    body = text[text.index("CSI_F_U = 0"):text.index("CSI_F_COUNT")]
    assert re.findall(r"CSI_F_(\w+)", body)[-3:] == ["FORCING_V", "GU", "GV"]
    protos = {"csi_rheology_set": 3, "csi_momentum_solver_set": 2, "csi_compute_momentum_tendencies": 2}
    for name, nargs in protos.items():
        m = re.search(r"int32_t\s+" + name + r"\(([^)]*)\)", text)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in csi._lib.SYMBOLS


def test_library_exports_the_new_entry_points():
    L = csi._lib.load()
    for name in ("csi_rheology_set", "csi_momentum_solver_set", "csi_compute_momentum_tendencies"):
        assert getattr(L, name).argtypes is not None


# ---- properties of the restatement (CPU oracle underneath) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_built(oracle_lib):
    return oracle_lib


def _problem(**kw):
    c = cases.make_case(**kw)
    return c, cases.oracle_problem(c)


def test_viscous_divergence_of_a_linear_field_is_zero_in_the_interior(oracle_built):
    c, p = _problem(Nx=12, Ny=10, topo=("bounded", "bounded"), patches=False, noise=0.0)
    s = p.s
    nj, ni = p.f["u"].shape
    I, J = np.meshgrid(np.arange(ni) - s.Hx + 1, np.arange(nj) - s.Hy + 1)
    p.f["u"][...] = 3.0 * I - 2.0 * J + 1.0                     # integer-valued linear fields: exact differences
    nj, ni = p.f["v"].shape
    I, J = np.meshgrid(np.arange(ni) - s.Hx + 1, np.arange(nj) - s.Hy + 1)
    p.f["v"][...] = -1.0 * I + 4.0 * J
    r = Ref(p, nu=1000.0)
    u, v = p.f["u"], p.f["v"]
    for j in range(3, s.Ny - 1):
        for i in range(3, s.Nx - 1):
            assert r.div1(u, v, i, j) == 0.0 and r.div2(u, v, i, j) == 0.0, (i, j)


def test_zero_viscosity_without_forcing_leaves_active_ice_at_rest(oracle_built):
    c, p = _problem(Nx=12, Ny=10, coriolis=None, top=None, bottom=None, patches=False, random_uv=0.05, seed=7)
    u0, v0 = p.interior("u").copy(), p.interior("v").copy()
    r = Ref(p, nu=0.0)
    r.viscous_subcycle(100.0, 3)
    assert np.array_equal(p.interior("u"), u0) and np.array_equal(p.interior("v"), v0)


def test_viscous_substep_is_independent_of_the_visiting_order(oracle_built):
    c, p = _problem(Nx=12, Ny=10, random_uv=0.05, land=0.15, immersed_bc=((0.1, -0.2, 0.05, 0.3), (0.2, 0.1, -0.1, 0.05)))
    r = Ref(p, nu=5e4)
    base = {k: p.f[k].copy() for k in ("u", "v")}
    r.viscous_component_step("u", 12.0)
    first = p.f["u"].copy()
    assert not np.array_equal(first, base["u"])
    perm = np.random.default_rng(11).permutation(p.s.Nx * p.s.Ny)
    for k in ("u", "v"):
        np.copyto(p.f[k], base[k])
    r.viscous_component_step("u", 12.0, order=perm)
    assert np.array_equal(p.f["u"], first)


# ---- generated code of the new FAST kernels (hipcc cross-compiles; nothing runs) -----------------------------------------------------
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# kernel-name fragment -> (loads in flight before the first vector-memory wait -- None: EVERY load of the kernel --, most
# `load ... vmcnt(0)` drains tolerated).  The viscous sub-step kernels gather all operands of a point -- velocities, h, aice, metrics,
# mask bytes, Coriolis parameter, stress arrays, forcing, free drift -- with unconditional loads from selected addresses
# (csrc/momentum_dev.h), so no load waits for another; the explicit steps issue their point loads first (the rest belong to the
# stress gather; none is waited for alone).  No gated kernel touches scratch memory: the halo images of store_with_images
# (csrc/csi_dev.h) sit in fixed slots.
GATED = {
    ("momentum_viscous", "12k_visc_ustepILb1E"): (None, 0), ("momentum_viscous", "12k_visc_vstepILb1E"): (None, 0),
    ("momentum_viscous", "12k_visc_ustepILb0E"): (None, 0), ("momentum_viscous", "12k_visc_vstepILb0E"): (None, 0),
    ("momentum_explicit", "12k_expl_ustepILb1E"): (11, 0), ("momentum_explicit", "12k_expl_vstepILb1E"): (13, 0),
    ("momentum_explicit", "12k_tendenciesILb1ELb0E"): (None, 0), ("momentum_explicit", "12k_tendenciesILb1ELb1E"): (40, 1),
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = {}
    for src in ("momentum_viscous", "momentum_explicit"):
        path = tmp_path_factory.mktemp("isa") / (src + ".s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-ffp-contract=off",
                               "--cuda-device-only", "-S", os.path.join(ROOT, "climaseaice.jl_amd", "csrc", src + ".hip"), "-o", str(path)],
                              stderr=subprocess.DEVNULL)
        lines = open(path).read().split("\n")
        starts = [(k, ln.split(":")[0]) for k, ln in enumerate(lines) if re.match(r"^_ZN3csi\S*: ", ln)]
        out[src] = {name: lines[k:(starts[n + 1][0] if n + 1 < len(starts) else len(lines))] for n, (k, name) in enumerate(starts)}
    return out


def _sequence(body):
    seq = []
    for ln in body:
        t = ln.strip()
        if t.startswith(("global_load", "buffer_load", "flat_load")):
            seq.append("L")
        elif t.startswith("s_waitcnt") and "vmcnt" in t:
            seq.append("W" + re.search(r"vmcnt\((\d+)\)", t).group(1))
    return seq


@pytest.mark.parametrize("key", list(GATED))
def test_fast_kernels_issue_the_point_loads_before_the_first_wait(asm, key):
    src, frag = key
    need, drains_allowed = GATED[key]
    names = [n for n in asm[src] if frag in n]
    assert len(names) == 1, (frag, names)
    seq = _sequence(asm[src][names[0]])
    first_wait = next(k for k, s in enumerate(seq) if s.startswith("W"))
    need = seq.count("L") if need is None else need
    assert seq[:first_wait].count("L") >= need, f"{names[0]}: {''.join(seq)[:200]}"
    drains = sum(1 for a, b in zip(seq, seq[1:]) if a == "L" and b == "W0")
    assert drains <= drains_allowed, f"{names[0]}: {drains} single-load round trips"
    assert not any(ln.strip().startswith("scratch_") for ln in asm[src][names[0]]), f"{names[0]} touches scratch memory"
