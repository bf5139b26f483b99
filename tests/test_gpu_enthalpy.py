"""The enthalpy-method column model on the GPU (include/csi.h, "enthalpy-method column model"; climaseaice.jl_amd/enthalpy.py).  Every
comparison is BIT FOR BIT against the NumPy restatement (tests/enthalpy_ref.py): H's interior, all of T (halo levels included), phi's
interior, all of kappa, and the clock.  Every test asserts last_launch() against tests/enthalpy_layouts.py first.  The shapes are the
smallest at which the kernel can go wrong: Nz 1, 2, 3, the example's 20, the largest on-chip Nz of the rule and one above it; 1, 63,
64, 65 columns and 130 x 3 (a partial last wave, several rows); 1, 2, 3, 37 sub-steps, the launch cap and one more."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import climaseaice_jl_amd as csi
import enthalpy_layouts as lay
import enthalpy_ref as ref
import time_series_ref as tsr

pytestmark = pytest.mark.gpu
L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEXING = {tsr.CLAMP: csi.Clamp, tsr.LINEAR: csi.Linear, tsr.CYCLICAL: csi.Cyclical}
CAP = lay.MAX_SUBSTEPS
NZ_CHIP, NZ_STEP = lay.LARGEST_ON_CHIP_NZ, lay.LARGEST_ON_CHIP_NZ + 1


def stretched_faces(Nz):
    k = np.arange(Nz + 1)
    return -2.0 + 2.0 * (k / Nz) ** 1.7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pair(Nx, Ny, zf, bottom=None, top=None, **params):
    """(library model, restatement) with the same faces, parameters and boundary temperatures.  A boundary: None, a number, an
    (Ny, Nx) array, or ("series", times, data, indexing[, period])."""
    zf = np.asarray(zf, dtype=np.float64)
    g = csi.ColumnGrid((Nx, Ny, zf.size - 1), z=zf)
    lib_side, ref_side = [], []
    for b in (bottom, top):
        if isinstance(b, tuple):
            _, times, data, indexing, *period = b
            ix = INDEXING[indexing](*period) if period else INDEXING[indexing]()
            lib_side.append(csi.ValueBoundaryCondition(csi.ColumnTimeSeries(g, times, data, time_indexing=ix)))
            ref_side.append(ref.Series(times, data, indexing, period[0] if period else 0.0))
        else:
            lib_side.append(None if b is None else csi.ValueBoundaryCondition(b))
            ref_side.append(b)
    names = dict(c="ice_heat_capacity", L="fusion_enthalpy")
    kw = {names[k]: v for k, v in params.items() if k in names}
    closure = csi.MolecularDiffusivity(params.get("kappa_ice", 1e-5), params.get("kappa_water", 1e-6))
    m = csi.EnthalpyMethodSeaIceModel(g, closure=closure, boundary_conditions=dict(T=csi.FieldBoundaryConditions(bottom=lib_side[0], top=lib_side[1])), **kw)
    r = ref.Model(Nx, Ny, zf, bottom=ref_side[0], top=ref_side[1], **params)
    return m, r


def start(m, r, T0):
    m.set(T=T0)
    r.set_T(T0)
    m.update_state()
    r.update_state()


def check_launch(m, n):
    p = lay.plan(m.grid.Nz)
    launches, first = lay.launches(p, n)
    want = dict(form="on_chip" if p["form"] == lay.ON_CHIP else "per_step", launches=launches, substeps_per_launch=first, lds_bytes=p["lds_bytes"])
    assert m.last_launch() == want, (m.last_launch(), want)


def same(m, r, what=""):
    m.synchronize()
    for name, f, want, whole in (("H", m.state.H, r.H, False), ("T", m.state.T, r.T, True), ("phi", m.state.phi, r.phi, False),
                                 ("kappa", m.closure.kappa, r.kappa, True)):
        got = f.numpy()
        a, b = (got, want) if whole else (got[1:-1], want[1:-1])
        bad = bits(a) != bits(b)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:3].tolist(), a[bad][:3], b[bad][:3])
    assert bits([m.clock.time])[0] == bits([r.time])[0] and m.clock.iteration == r.iteration, (what, m.clock.time, r.time)


def advance(m, r, dt, n):
    m.time_steps(dt, n)
    check_launch(m, n)
    r.time_steps(dt, n)


def profile(rng, Nz, Ny, Nx):
    """Warm below, cold above, noisy: both phases, cells on either side of zero next to each other."""
    return np.linspace(1.5, -4.0, Nz)[:, None, None] + rng.uniform(-0.8, 0.8, (Nz, Ny, Nx))


def stable_dt(zf):
    return 0.1 * float(np.min(np.diff(zf))) ** 2 / 1e-5


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Nz", [1, 2, 3, 20, NZ_CHIP, NZ_STEP])
@pytest.mark.parametrize("stretched", [False, True])
def test_depths(Nz, stretched):
    rng = np.random.default_rng(Nz)
    Nx, Ny = 65, 2
    zf = stretched_faces(Nz) if stretched and Nz > 1 else ref.uniform_faces(-1.0, 0.0, Nz)
    m, r = pair(Nx, Ny, zf, bottom=1.1, top=rng.uniform(-8.0, -2.0, (Ny, Nx)))
    start(m, r, profile(rng, Nz, Ny, Nx))
    advance(m, r, stable_dt(zf), 37)
    same(m, r)
    assert lay.plan(Nz)["form"] == (lay.PER_STEP if Nz == NZ_STEP else lay.ON_CHIP)


@pytest.mark.parametrize("Nx, Ny", [(1, 1), (63, 1), (64, 1), (65, 1), (130, 3)])
@pytest.mark.parametrize("Nz", [3, NZ_STEP])
def test_columns(Nx, Ny, Nz):
    rng = np.random.default_rng(Nx)
    zf = stretched_faces(Nz)
    times = ref.step_times(1.5 * stable_dt(zf), 6)
    m, r = pair(Nx, Ny, zf, bottom=("series", times, rng.uniform(0.5, 1.5, (6, Ny, Nx)), tsr.LINEAR), top=rng.uniform(-8.0, -2.0, (Ny, Nx)))
    start(m, r, profile(rng, Nz, Ny, Nx))
    advance(m, r, stable_dt(zf), 7)
    same(m, r)


@pytest.mark.parametrize("n", [1, 2, 3, 37, CAP, CAP + 1])
def test_substep_counts(n):
    rng = np.random.default_rng(n)
    Nx, Ny, Nz = 65, 2, 20
    zf = ref.uniform_faces(-1.0, 0.0, Nz)
    dt = stable_dt(zf)
    times = ref.step_times(dt, 40)                  # (n above 40: beyond the last node, extrapolated below and clamped above)
    m, r = pair(Nx, Ny, zf, bottom=("series", times, ref.example_ice_ocean_temperature(times * 500), tsr.LINEAR),
                top=("series", times, rng.uniform(-8.0, -2.0, (40, Ny, Nx)), tsr.CLAMP))
    start(m, r, profile(rng, Nz, Ny, Nx))
    advance(m, r, dt, n)
    same(m, r)


# ---- boundary temperatures ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["none", "number", "array", "scalar series", "plane series"])
@pytest.mark.parametrize("side", ["bottom", "top"])
@pytest.mark.parametrize("Nz", [4, NZ_STEP])
def test_each_boundary_kind_on_each_side(kind, side, Nz):
    rng = np.random.default_rng(len(kind) + Nz)
    Nx, Ny = 70, 2
    zf = stretched_faces(Nz)
    dt = stable_dt(zf)
    times = ref.step_times(2 * dt, 5)               # a node on every second step time, the others half way
    mean = 1.0 if side == "bottom" else -5.0
    b = {"none": None, "number": mean, "array": mean + rng.uniform(-1, 1, (Ny, Nx)),
         "scalar series": ("series", times, mean + rng.uniform(-1, 1, 5), tsr.LINEAR),
         "plane series": ("series", times, mean + rng.uniform(-1, 1, (5, Ny, Nx)), tsr.LINEAR)}[kind]
    other = -3.0 if side == "bottom" else 0.7
    m, r = pair(Nx, Ny, zf, **{side: b, "top" if side == "bottom" else "bottom": other})
    start(m, r, profile(rng, Nz, Ny, Nx))
    advance(m, r, dt, 6)
    same(m, r)


@pytest.mark.parametrize("indexing", [tsr.CLAMP, tsr.LINEAR, tsr.CYCLICAL])
def test_series_indexing_nodes_on_step_times_and_times_beyond_the_last_node(indexing):
    rng = np.random.default_rng(indexing)
    Nx, Ny, Nz = 66, 1, 5
    zf = stretched_faces(Nz)
    dt = stable_dt(zf)
    times = ref.step_times(dt, 4)                   # nodes exactly ON the first four step times; the run goes nine steps beyond them
    assert tsr.plan(times, indexing, 0.0, times[2])[:2] == (2, 2)
    m, r = pair(Nx, Ny, zf, bottom=("series", times, np.array([1.0, 1.4, 0.6, 1.2]), indexing),
                top=("series", times, rng.uniform(-8.0, -2.0, (4, Ny, Nx)), indexing))
    start(m, r, profile(rng, Nz, Ny, Nx))
    advance(m, r, dt, 13)
    same(m, r)
    last = tsr.plan(times, indexing, 0.0, float(r.time) - dt)
    assert {tsr.CLAMP: last == (3, 3, 0.0), tsr.LINEAR: last[:2] == (2, 3) and last[2] > 1.0, tsr.CYCLICAL: last[0] <= 3}[indexing]
    # a given period
    if indexing == tsr.CYCLICAL:
        m, r = pair(Nx, Ny, zf, bottom=("series", times, np.array([1.0, 1.4, 0.6, 1.2]), indexing, 5.5 * dt), top=-4.0)
        start(m, r, profile(rng, Nz, Ny, Nx))
        advance(m, r, dt, 13)
        same(m, r)


# ---- per cell -----------------------------------------------------------------------------------------------------------------------------

def test_zero_and_negative_zero_are_not_frozen():
    Nx, Ny, Nz = 4, 1, 6
    zf = ref.uniform_faces(-1.0, 0.0, Nz)
    m, r = pair(Nx, Ny, zf, bottom=0.5, top=-2.0)
    H = np.zeros((Nz, Ny, Nx))
    H[:, 0, 0] = [1.0, 0.0, -0.0, -1.0, 0.0, -2.0]
    H[:, 0, 1] = [-0.0] * Nz
    H[:, 0, 2] = [0.0] * Nz
    H[:, 0, 3] = [5e-324, -5e-324, 0.0, -0.0, 1.0, -1.0]
    m.set(H=H)
    r.set_H(H)
    same(m, r, "set H")
    m.update_state()
    r.update_state()
    same(m, r, "update_state")
    assert np.all(r.phi[1:-1, 0, 1] == 0.0) and np.all(r.phi[1:-1, 0, 2] == 0.0) and r.phi[3, 0, 0] == 0.0 and r.phi[4, 0, 0] == 1.0
    assert np.signbit(m.state.T.numpy()[3, 0, 0]) and not np.signbit(m.state.T.numpy()[2, 0, 0])
    advance(m, r, stable_dt(zf), 3)
    same(m, r, "steps")


# ---- invariances ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Nz", [20, NZ_STEP])
def test_fused_steps_equal_single_steps_and_split_calls(Nz):
    rng = np.random.default_rng(3)
    Nx, Ny, n, a = 65, 1, 11, 4
    zf = ref.uniform_faces(-1.0, 0.0, Nz)
    dt = stable_dt(zf)
    times = ref.step_times(dt, n + 2)
    T0 = profile(rng, Nz, Ny, Nx)
    top = rng.uniform(-8.0, -2.0, (n + 2, Ny, Nx))
    states = []
    for how in ("fused", "single", "split"):
        m, r = pair(Nx, Ny, zf, bottom=("series", times, np.linspace(1.2, 0.2, n + 2), tsr.LINEAR), top=("series", times, top, tsr.LINEAR))
        start(m, r, T0)
        if how == "fused":
            m.time_steps(dt, n)
            check_launch(m, n)
        elif how == "single":
            for _ in range(n):
                m.time_step(dt)
                check_launch(m, 1)
        else:
            m.time_steps(dt, a)
            check_launch(m, a)
            m.time_steps(dt, n - a)
            check_launch(m, n - a)
        r.time_steps(dt, n)
        same(m, r, how)
        states.append(m.prognostic_state())
    for s in states[1:]:
        assert s["clock"] == states[0]["clock"]
        for k in ("H", "T", "phi", "kappa"):
            assert np.array_equal(bits(s[k]), bits(states[0][k])), k


CHILD_CASE = dict(Nx=130, Ny=3, Nz=20, n=70, seed=17)


def child_case(path_out=None):
    """One fixed case, run by this process and -- with CSI_ENTH_PATH in its environment -- by a child; the child writes its state."""
    c = CHILD_CASE
    rng = np.random.default_rng(c["seed"])
    zf = stretched_faces(c["Nz"])
    dt = stable_dt(zf)
    times = ref.step_times(dt, 30)
    m, r = pair(c["Nx"], c["Ny"], zf, bottom=("series", times, np.linspace(1.2, 0.2, 30), tsr.CLAMP),
                top=("series", times, rng.uniform(-8.0, -2.0, (30, c["Ny"], c["Nx"])), tsr.CYCLICAL))
    start(m, r, profile(rng, c["Nz"], c["Ny"], c["Nx"]))
    m.time_steps(dt, c["n"])
    if path_out:
        s = m.prognostic_state()
        np.savez(path_out, form=m.last_launch()["form"], launches=m.last_launch()["launches"], time=s["clock"][0],
                 **{k: s[k] for k in ("H", "T", "phi", "kappa")})
    return m, r, dt


def test_on_chip_equals_per_step_in_a_child_process(tmp_path):
    """CSI_ENTH_PATH is read when a context is created: the forced forms run in child processes of their own."""
    m, r, dt = child_case()
    check_launch(m, CHILD_CASE["n"])
    assert m.last_launch()["form"] == "on_chip"
    r.time_steps(dt, CHILD_CASE["n"])
    same(m, r)
    mine = m.prognostic_state()
    for forced, form, launches in (("1", "per_step", CHILD_CASE["n"]), ("2", "on_chip", 2)):
        out = str(tmp_path / f"child{forced}.npz")
        env = dict(os.environ, CSI_ENTH_PATH=forced, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True, env=env, timeout=240, cwd=ROOT)
        got = np.load(out)
        assert str(got["form"]) == form and int(got["launches"]) == launches
        assert bits([float(got["time"])])[0] == bits([mine["clock"][0]])[0]
        for k in ("H", "T", "phi", "kappa"):
            assert np.array_equal(bits(got[k]), bits(mine[k])), (forced, k)


def test_forced_paths_and_bad_values(monkeypatch):
    rng = np.random.default_rng(2)
    zf = stretched_faces(100)
    monkeypatch.setenv("CSI_ENTH_PATH", "2")                 # deeper than the rule takes on chip, but one wave's image fits a CU
    m, r = pair(65, 1, zf, bottom=1.0, top=-4.0)
    start(m, r, profile(rng, 100, 1, 65))
    m.time_steps(stable_dt(zf), 5)
    assert m.last_launch() == dict(form="on_chip", launches=1, substeps_per_launch=5, lds_bytes=lay.lds_bytes(100))
    r.time_steps(stable_dt(zf), 5)
    same(m, r)
    with pytest.raises(csi.CsiError, match="does not fit") as e:
        csi.EnthalpyMethodSeaIceModel(csi.ColumnGrid(lay.LARGEST_FORCED_NZ + 1, z=(-1, 0)))
    assert e.value.code == -4
    for bad in ("3", "-1", "x", "1.5"):
        monkeypatch.setenv("CSI_ENTH_PATH", bad)
        with pytest.raises(csi.CsiError, match="CSI_ENTH_PATH"):
            csi.Context(0)
    monkeypatch.setenv("CSI_ENTH_PATH", "0")
    csi.Context(0).close()


# ---- set!, a fresh model ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Nz", [8, NZ_STEP])
def test_a_fresh_model_bare_step_then_update_state_then_steps(Nz):
    rng = np.random.default_rng(8)
    Nx, Ny = 65, 1
    zf = ref.uniform_faces(-1.0, 0.0, Nz)
    dt = stable_dt(zf)
    m, r = pair(Nx, Ny, zf, bottom=1.0, top=-5.0)
    T0 = profile(rng, Nz, Ny, Nx)
    m.set(T=T0)
    r.set_T(T0)
    same(m, r, "set T on a fresh model")
    H0 = m.state.H.numpy().copy()
    assert np.all(m.closure.kappa.numpy() == 0.0)
    advance(m, r, dt, 1)                                      # kappa = 0: H stays; the step's update_state fills phi and kappa
    same(m, r, "bare step")
    assert np.array_equal(m.state.H.numpy(), H0) and np.any(m.closure.kappa.numpy() != 0.0)
    m.update_state()
    r.update_state()
    advance(m, r, dt, 9)
    same(m, r, "steps")
    assert not np.array_equal(m.state.H.numpy(), H0)


def test_set_T_and_set_H_on_a_model_whose_porosity_is_not_zero():
    rng = np.random.default_rng(9)
    Nx, Ny, Nz = 65, 2, 7
    zf = stretched_faces(Nz)
    times = ref.step_times(10.0, 4)
    m, r = pair(Nx, Ny, zf, bottom=("series", times, np.array([1.0, 0.5, 0.2, 0.1]), tsr.LINEAR), top=rng.uniform(-8.0, -2.0, (Ny, Nx)))
    start(m, r, profile(rng, Nz, Ny, Nx))
    advance(m, r, 10.0, 2)
    assert 0 < r.phi[1:-1].sum() < r.phi[1:-1].size
    T1 = profile(rng, Nz, Ny, Nx)
    m.set(T=T1)
    r.set_T(T1)
    same(m, r, "set T")
    assert np.any(r.H[1:-1] != r.c * r.T[1:-1])               # the latent term of the porosity held
    H1 = rng.uniform(-6.0, 3.0, (Nz, Ny, Nx))
    m.set(H=H1)
    r.set_H(H1)                                               # T's halos at the clock's time, 20 s: between two nodes
    same(m, r, "set H")
    with pytest.raises(ValueError, match="Cannot set both"):
        m.set(T=1.0, H=1.0)


def test_poisoned_halos_and_porosity_are_never_read():
    rng = np.random.default_rng(10)
    for Nz in (5, NZ_STEP):
        Nx, Ny = 65, 1
        zf = stretched_faces(Nz)
        m, r = pair(Nx, Ny, zf, bottom=1.0, top=-5.0)
        start(m, r, profile(rng, Nz, Ny, Nx))
        H = m.state.H.numpy().copy()
        H[0], H[-1] = np.nan, np.nan
        m.state.H.set_parent(H)
        m.state.phi.set_parent(np.full_like(H, np.nan))
        advance(m, r, stable_dt(zf), 3)
        same(m, r, f"Nz {Nz}")                                  # T's and kappa's halo levels included
        got = m.state.H.numpy()
        assert np.all(np.isnan(got[0])) and np.all(np.isnan(got[-1])) and np.all(np.isnan(m.state.phi.numpy()[[0, -1]]))
        assert np.all(np.isfinite(m.state.T.numpy())) and np.all(np.isfinite(m.closure.kappa.numpy()))


# ---- thickness ------------------------------------------------------------------------------------------------------------------------------

def test_ice_thickness():
    rng = np.random.default_rng(12)
    Nx, Ny, Nz = 70, 2, 9
    zf = stretched_faces(Nz)
    m, r = pair(Nx, Ny, zf)
    T = np.sort(rng.uniform(-6.0, 1.5, (Nz, Ny, Nx)), axis=0)[::-1].copy()      # mixed, monotone
    T[:, 0, 0] = -3.0                                          # wholly frozen
    T[:, 0, 1] = 0.5                                           # wholly liquid
    T[:, 0, 2] = [1.0, 0.5, -1.0, 0.7, -2.0, -3.0, 0.2, -4.0, -5.0]      # not monotone: the first level below Tm from the bottom counts
    T[:, 0, 3] = [1.0, 0.5, -0.1, -0.1, -2.0, -3.0, -3.5, -4.0, -5.0]    # Tm equal to a cell's value: T >= Tm holds there
    T[:, 0, 4] = [-0.1] * Nz                                   # ... in every cell
    T[:, 0, 5] = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -0.5]          # the last pair
    T[:, 0, 6] = [1.0, -0.5, -0.5, -0.5, -0.5, -0.5, -0.5, -0.5, -0.5]   # the first pair
    m.set(T=T)
    r.set_T(T)
    assert m.last_launch()["form"] is None                     # no time step yet
    for Tm in (-0.1, 0.0, -2.0):
        got, want = m.ice_thickness(Tm), r.ice_thickness(Tm)
        assert np.array_equal(bits(got), bits(want)), Tm
    h = m.ice_thickness()
    assert h[0, 0] == 2.0 and h[0, 1] == 0.0 and h[0, 4] == 0.0 and 0 < h[0, 2] < 2.0
    assert h[0, 2] == r.ice_thickness()[0, 2] and -r.zc[2] < h[0, 2] < -r.zc[1]      # between levels 2 and 3 (1-based), not further up


# ---- checkpoint, errors, the reference's own test and example -----------------------------------------------------------------------------

def test_checkpoint_round_trip_mid_run():
    rng = np.random.default_rng(13)
    Nx, Ny, Nz = 65, 2, 20
    zf = ref.uniform_faces(-1.0, 0.0, Nz)
    dt = stable_dt(zf)
    times = ref.step_times(dt, 30)
    mk = lambda: pair(Nx, Ny, zf, bottom=("series", times, np.linspace(1.2, 0.2, 30), tsr.LINEAR), top=rng_top)      # noqa: E731
    rng_top = rng.uniform(-8.0, -2.0, (Ny, Nx))
    m, r = mk()
    T0 = profile(rng, Nz, Ny, Nx)
    m.set(T=T0)                                               # NOT followed by update_state: T and kappa are not functions of H here
    r.set_T(T0)
    advance(m, r, dt, 1)
    saved = m.prognostic_state()
    advance(m, r, dt, 20)
    same(m, r)
    end = m.prognostic_state()
    m2, _ = mk()
    m2.restore_prognostic_state(saved)
    assert m2.clock.time == saved["clock"][0] and m2.clock.iteration == 1
    m2.time_steps(dt, 20)
    again = m2.prognostic_state()
    assert again["clock"] == end["clock"]
    for k in ("H", "T", "phi", "kappa"):
        assert np.array_equal(bits(again[k]), bits(end[k])), k


def test_errors_by_name():
    lib = L.load()
    ctx = csi.Context(0)
    zf = np.array([-1.0, -0.5, 0.0])

    def create(Nx=2, Ny=1, Nz=2, faces=zf, c=2.0):
        p = L.EnthalpyParams(Nx, Ny, Nz, 0, faces.ctypes.data_as(C.POINTER(C.c_double)), c, 4.0, 330.0, 1e-5, 1e-6)
        h = C.c_void_p()
        return lib.csi_enthalpy_create(ctx.h, C.byref(p), C.byref(h)), h

    msg = lambda: lib.csi_last_error(ctx.h).decode()          # noqa: E731
    for kw, words in ((dict(Nz=0), "Nx, Ny, Nz >= 1"), (dict(faces=np.array([-1.0, -1.0, 0.0])), "strictly increasing"),
                      (dict(faces=np.array([-1.0, np.nan, 0.0])), "strictly increasing"), (dict(c=0.0), "must not be zero"),
                      (dict(c=float("inf")), "must be finite")):
        rc, _ = create(**kw)
        assert rc == -1 and words in msg(), (kw, msg())
    rc, h = create()
    assert rc == 0
    t = C.c_double()
    # unbound arrays, by name
    assert lib.csi_enthalpy_time_step(h, 1.0, 1, 0.0, C.byref(t)) == -2 and "array H is not bound" in msg()
    assert lib.csi_enthalpy_update_state(h, 0.0) == -2 and lib.csi_enthalpy_set(h, L.ENTH_T, 0.0) == -2
    import torch
    arrays = [torch.zeros((4, 1, 2), dtype=torch.float64, device="cuda:0") for _ in range(4)]
    torch.cuda.synchronize()
    for which, a in enumerate(arrays[:3]):
        assert lib.csi_enthalpy_bind(h, which, C.c_void_p(a.data_ptr())) == 0
    assert lib.csi_enthalpy_time_step(h, 1.0, 1, 0.0, C.byref(t)) == -2 and "array kappa is not bound" in msg()
    assert lib.csi_enthalpy_ice_thickness(h, -0.1, None) == -1
    assert lib.csi_enthalpy_bind(h, 3, C.c_void_p(arrays[3].data_ptr())) == 0 and lib.csi_enthalpy_bind(h, 4, None) == -1
    for dt, n, time, words in ((float("nan"), 1, 0.0, "dt must be finite"), (float("inf"), 1, 0.0, "dt must be finite"), (1.0, 0, 0.0, "n >= 1"),
                               (1.0, -2, 0.0, "n >= 1"), (1.0, 1, float("nan"), "time must be finite")):
        assert lib.csi_enthalpy_time_step(h, dt, n, time, C.byref(t)) == -1 and words in msg(), words
    # boundary conditions that are not built: refused by name
    B = lib.csi_enthalpy_boundary_set
    assert B(h, L.ENTH_H_TOP, L.ENTH_BC_NUMBER, 1.0, None, None) == -4 and "boundary condition on H" in msg()
    assert B(h, L.ENTH_H_BOTTOM, L.ENTH_BC_NONE, 0.0, None, None) == 0
    assert B(h, L.ENTH_T_TOP, L.ENTH_BC_FLUX, 1.0, None, None) == -4 and "flux or gradient" in msg()
    assert B(h, L.ENTH_T_BOTTOM, L.ENTH_BC_GRADIENT, 1.0, None, None) == -4
    assert B(h, L.ENTH_T_TOP, L.ENTH_BC_NUMBER, float("nan"), None, None) == -1 and B(h, 7, 0, 0.0, None, None) == -1
    assert B(h, L.ENTH_T_TOP, 9, 0.0, None, None) == -1 and B(h, L.ENTH_T_TOP, L.ENTH_BC_ARRAY, 0.0, None, None) == -1
    times = np.array([0.0, 1.0])
    data = torch.zeros(2, dtype=torch.float64, device="cuda:0")
    ts = L.TimeSeries(2, L.TIME_LINEAR, L.SERIES_HOST, 0, 0.0, times.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(data.data_ptr()), 1, 1)
    assert B(h, L.ENTH_T_TOP, L.ENTH_BC_SERIES_SCALAR, 0.0, None, C.byref(ts)) == -4 and "HOST series backend" in msg()
    ts.backend = L.SERIES_DEVICE
    ts.ld, ts.slice_stride = 1, 1
    assert B(h, L.ENTH_T_TOP, L.ENTH_BC_SERIES_PLANE, 0.0, None, C.byref(ts)) == -1 and "too small" in msg()      # planes of 2 need ld >= 2
    assert B(h, L.ENTH_T_TOP, L.ENTH_BC_SERIES_SCALAR, 0.0, None, C.byref(ts)) == 0
    bad = np.array([1.0, 1.0])
    ts.times = bad.ctypes.data_as(C.POINTER(C.c_double))
    assert B(h, L.ENTH_T_TOP, L.ENTH_BC_SERIES_SCALAR, 0.0, None, C.byref(ts)) == -1 and "strictly increasing" in msg()
    assert lib.csi_enthalpy_time_step(h, 1.0, 3, 0.0, C.byref(t)) == 0 and t.value == 3.0
    ctx.call("csi_sync")
    # a model that survives its context's destruction is freed with it (nothing to assert but that neither call faults); destroy is explicit here
    assert lib.csi_enthalpy_destroy(h) == 0
    rc, h2 = create()
    assert rc == 0
    ctx.close()


def test_the_references_own_test_restated():
    """test/runtests.jl:9-28: size 3, z = (-3, 0), kappa_ice = kappa_water = 1e-5, no boundary conditions, a fresh model; the
    Simulation's run! calls update_state!, then three steps of 0.1 / kappa."""
    m, r = pair(1, 1, ref.uniform_faces(-3.0, 0.0, 3), kappa_ice=1e-5, kappa_water=1e-5)
    assert isinstance(m, csi.EnthalpyMethodSeaIceModel)
    m.update_state()
    r.update_state()
    for _ in range(3):
        m.time_step(0.1 / 1e-5)
        check_launch(m, 1)
        r.time_step(0.1 / 1e-5)
    same(m, r)
    assert m.clock.iteration == 3 and np.all(m.state.H.numpy()[1:-1] == 0.0) and np.all(m.closure.kappa.numpy() == 1e-5)


def test_the_example_over_two_hours_and_more():
    """examples/diffusive_ice_column_model.jl: 288 steps, an hour (144 steps: launches of 64, 64 and 16 sub-steps) per call."""
    r, dt = ref.example_model(288)
    g = csi.ColumnGrid(20, z=(-1, 0), topology=(csi.Flat, csi.Flat, csi.Bounded))
    assert np.array_equal(g.z_faces, r.zf) and dt == 0.1 * g.minimum_zspacing() ** 2 / 1e-5
    times = ref.step_times(dt, 290)
    bc = csi.FieldBoundaryConditions(top=csi.ValueBoundaryCondition(csi.ColumnTimeSeries(g, times, ref.example_air_ice_temperature(times))),
                                     bottom=csi.ValueBoundaryCondition(csi.ColumnTimeSeries(g, times, ref.example_ice_ocean_temperature(times))))
    m = csi.EnthalpyMethodSeaIceModel(g, closure=csi.MolecularDiffusivity(kappa_ice=1e-5, kappa_water=1e-6), boundary_conditions=dict(T=bc))
    m.set(T=1.1)
    m.update_state()
    for hour in range(2):
        m.time_steps(dt, 144)
        check_launch(m, 144)
        assert m.last_launch()["launches"] == 3
        r.time_steps(dt, 144)
        same(m, r, f"hour {hour + 1}")
        assert np.array_equal(bits(m.ice_thickness()), bits(r.ice_thickness()))
    assert 0 < r.phi[1:-1].sum() < 20 and 0.0 < m.ice_thickness()[0, 0] < 1.0


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    child_case(sys.argv[2])
