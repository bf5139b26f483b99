"""Device-side output on the GPU (include/csi.h csi_output_*; climaseaice.jl_amd/output.py).  Every comparison is BIT FOR BIT against
tests/output_ref.py applied to the parent arrays (Field.numpy()) of the same model, NaN equal to NaN: nothing here has a tolerance.
STRICT and FAST must give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import output_ref as ref

pytestmark = pytest.mark.gpu
L = csi._lib
DEV = "cuda:0"

LOC = {"U": (1, 0), "V": (0, 1), "H": (0, 0), "A": (0, 0), "S12": (1, 1)}          # (Face in x, Face in y)
FIVE = ["U", "V", "H", "A", "S12"]                                                  # three record shapes in one launch
SPECIALS = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300, 1e-40, 1e-46, -1e-46]
TOPOS = {"pp": (L.PERIODIC, L.PERIODIC), "bb": (L.BOUNDED, L.BOUNDED), "pb": (L.PERIODIC, L.BOUNDED), "pf": (L.PERIODIC, L.RIGHT_FOLDED)}
NXS = [1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1025]        # (a block covers 256 columns: no wider sizes needed)
NYS = [1, 2, 7]


class Raw:
    """A context with a grid and fields bound to torch tensors, without a model: what the kernels see and nothing else."""

    def __init__(self):
        self.ctx = L.Context(0)
        self.t = {}

    def grid(self, Nx, Ny, Hx, Hy, topo, names=FIVE, seed=0):
        self.ctx.call("csi_sync")
        met = L.Metrics()
        met.dx = met.dy = 1000.0
        self.ctx.call("csi_grid_set", Nx, Ny, Hx, Hy, topo[0], topo[1], L.METRIC_UNIFORM, C.byref(met))
        self.N, self.H = (Nx, Ny), (Hx, Hy)
        rng = np.random.default_rng(seed)
        self.t = {}
        for k, n in enumerate(names):
            ni = Nx + 2 * Hx + (LOC[n][0] and topo[0] == L.BOUNDED)
            nj = Ny + 2 * Hy + (LOC[n][1] and topo[1] == L.BOUNDED)
            a = np.full((nj, ni), np.nan)                      # halos hold NaN: no halo value may appear in a record
            x = rng.standard_normal((nj - 2 * Hy, ni - 2 * Hx)) * 10.0 ** rng.integers(-3, 4)
            for c, (j, i) in enumerate(((0, 0), (0, -1), (-1, 0), (-1, -1))):
                x[j, i] = SPECIALS[(4 * k + c) % len(SPECIALS)]
            a[Hy:nj - Hy, Hx:ni - Hx] = x
            self.t[n] = torch.from_numpy(a).to(DEV)
            self.ctx.call("csi_field_bind", L.F[n], C.c_void_p(self.t[n].data_ptr()), ni, ni, nj)
        torch.cuda.synchronize()

    def set(self, name, interior):
        """Rewrite a field's interior from a host array (the library's stream is drained first: it may still read the old values)."""
        self.ctx.call("csi_sync")
        Hx, Hy = self.H
        nj, ni = self.t[name].shape
        self.t[name][Hy:nj - Hy, Hx:ni - Hx].copy_(torch.from_numpy(np.ascontiguousarray(interior)))
        torch.cuda.synchronize()

    def interior(self, name):
        return ref.interior(self.t[name].cpu().numpy(), *self.H)

    def record(self, handle, slot, shapes, dtypes):
        rec = self.ctx.output_wait(handle, slot).copy()
        self.ctx.output_release(handle, slot)
        return ref.split_record(rec, shapes, dtypes)


@pytest.fixture(scope="module")
def raw():
    r = Raw()
    yield r
    r.ctx.close()


# ---- pack layout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", [(1, 1), (3, 2), (4, 4), (5, 3)], ids=lambda h: f"halo{h[0]}{h[1]}")
@pytest.mark.parametrize("topo", list(TOPOS))
def test_pack_layout(raw, halo, topo):
    checked = 0
    for Ny in NYS:
        for Nx in NXS:
            raw.grid(Nx, Ny, halo[0], halo[1], TOPOS[topo], seed=Nx + 7 * Ny)
            want64 = [raw.interior(n) for n in FIVE]
            shapes = [x.shape for x in want64]
            assert shapes[2] == (Ny, Nx) and shapes[0] == (Ny, Nx + (topo == "bb")) and shapes[4][0] == Ny + (topo in ("bb", "pb"))
            for dtype in ("f64", "f32"):
                h = raw.ctx.output_create([(n, L.OUT_F32 if dtype == "f32" else L.OUT_F64, 0, 0, 0.0) for n in FIVE], 2)
                offs, total = ref.layout(shapes, [dtype] * 5)
                assert [raw.ctx.output_layout(h, k) for k in range(5)] == [(o, ny, nx) for o, (ny, nx) in zip(offs, shapes)]
                assert raw.ctx.output_record_bytes(h) == total
                got = {}
                for mode in (L.MODE_STRICT, L.MODE_FAST):
                    raw.ctx.call("csi_set_mode", mode)
                    got[mode] = raw.record(h, raw.ctx.output_snapshot(h), shapes, [dtype] * 5)
                raw.ctx.output_destroy(h)
                for k, n in enumerate(FIVE):
                    want = ref.element(want64[k], dtype)
                    for mode, g in got.items():
                        assert ref.same_bits(g[k], want), (Nx, Ny, dtype, n, mode, np.argwhere(~(g[k] == want) & ~np.isnan(want))[:4].tolist())
                    checked += 1
    assert checked == len(NYS) * len(NXS) * 2 * 5


def test_planted_values_reach_fp32_as_inf_subnormal_and_signed_zero(raw):
    raw.grid(5, 2, 3, 2, TOPOS["pp"], names=["H"])
    x = np.array([[1e300, -1e300, 1e-40, 1e-46, -1e-46], [np.nan, np.inf, -0.0, 0.0, 1.0 + 2.0 ** -24]])
    raw.set("H", x)
    h = raw.ctx.output_create([("H", L.OUT_F32, 0, 0, 0.0)], 1)
    (y,) = raw.record(h, raw.ctx.output_snapshot(h), [(2, 5)], ["f32"])
    raw.ctx.output_destroy(h)
    assert ref.same_bits(y, ref.convert(x, "f32"))
    assert y[0, 0] == np.inf and y[0, 1] == -np.inf and 0 < y[0, 2] < np.finfo(np.float32).tiny
    assert y[0, 3] == 0 and not np.signbit(y[0, 3]) and y[0, 4] == 0 and np.signbit(y[0, 4]) and y[1, 4] == 1.0


# ---- mask -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [np.nan, -999.0])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_mask(raw, fill, dtype):
    Nx, Ny, Hx, Hy = 67, 9, 3, 2
    raw.grid(Nx, Ny, Hx, Hy, TOPOS["bb"], names=["H", "A", "U"], seed=3)
    act = np.ones((Ny, Nx), np.uint8)
    act[0, :] = act[-1, :] = act[:, 0] = act[:, -1] = 0
    act[4, 5:40:3] = 0
    full = np.full((Ny + 2 * Hy, Nx + 2 * Hx), 7, np.uint8)          # (halo bytes are never read: whatever they hold changes nothing)
    full[Hy:Hy + Ny, Hx:Hx + Nx] = act
    mask = torch.from_numpy(full).to(DEV)
    torch.cuda.synchronize()
    raw.ctx.call("csi_mask_set", C.c_void_p(mask.data_ptr()), full.shape[1])
    d = L.OUT_F32 if dtype == "f32" else L.OUT_F64
    with pytest.raises(csi.CsiError, match=r"field u.*\(Center, Center\)") as e:
        raw.ctx.output_create([("H", d, 0, 1, fill), ("U", d, 0, 1, fill)], 1)
    assert e.value.code == -1
    h = raw.ctx.output_create([("H", d, 0, 1, fill), ("A", d, 0, 0, fill), ("U", d, 0, 0, fill)], 1)
    shapes = [(Ny, Nx), (Ny, Nx), (Ny, Nx + 1)]
    got = raw.record(h, raw.ctx.output_snapshot(h), shapes, [dtype] * 3)
    assert ref.same_bits(got[0], ref.element(raw.interior("H"), dtype, act, fill))
    assert ref.same_bits(got[1], ref.element(raw.interior("A"), dtype)) and ref.same_bits(got[2], ref.element(raw.interior("U"), dtype))
    if fill == -999.0:
        assert (got[0][act == 0] == -999.0).all() and (got[0] == -999.0).sum() == (act == 0).sum()
    # without a mask the same set packs h as it is
    raw.ctx.call("csi_mask_set", None, 0)
    got = raw.record(h, raw.ctx.output_snapshot(h), shapes, [dtype] * 3)
    assert ref.same_bits(got[0], ref.element(raw.interior("H"), dtype))
    raw.ctx.output_destroy(h)


# ---- averages ---------------------------------------------------------------------------------------------------------------------------
WEIGHTS = [120.0, 37.5, 0.1, 1e-3]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("halo", [(4, 4), (3, 2)], ids=["halo44", "halo32"])
def test_averages(raw, dtype, halo):
    Nx, Ny = 130, 11
    raw.grid(Nx, Ny, halo[0], halo[1], TOPOS["bb"], names=["H", "U", "A", "V"], seed=5)
    d = L.OUT_F32 if dtype == "f32" else L.OUT_F64
    # h and u averaged, aice and v snapshots: a set that mixes both; h masked (no mask set: nothing is filled)
    h = raw.ctx.output_create([("H", d, 1, 1, -1.0), ("U", d, 1, 0, 0.0), ("A", d, 0, 0, 0.0), ("V", d, 0, 0, 0.0)], 2)
    shapes = [(Ny, Nx), (Ny, Nx + 1), (Ny, Nx), (Ny + 1, Nx)]
    with pytest.raises(csi.CsiError, match="W == 0"):
        raw.ctx.output_snapshot(h)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(csi.CsiError, match="weight"):
            raw.ctx.output_accumulate(h, bad)
    rng = np.random.default_rng(8)
    for window in range(2):                  # the second window starts from zero
        states = {"H": [], "U": []}
        for mode, w in zip((L.MODE_STRICT, L.MODE_FAST) * 2, WEIGHTS):
            for n in states:
                x = rng.standard_normal(raw.interior(n).shape) * 3.0
                x[0, 0], x[-1, -1] = (np.inf, 1e300) if window == 0 else (-0.0, 1e-300)
                raw.set(n, x)
                states[n].append(x)
            raw.ctx.call("csi_set_mode", mode)
            raw.ctx.output_accumulate(h, w)
        got = raw.record(h, raw.ctx.output_snapshot(h), shapes, [dtype] * 4)
        for k, n in enumerate(("H", "U")):
            want = ref.element(ref.averaged(states[n], WEIGHTS), dtype)
            assert ref.same_bits(got[k], want), (window, n, np.argwhere(got[k] != want)[:4].tolist())
        assert ref.same_bits(got[2], ref.element(raw.interior("A"), dtype)) and ref.same_bits(got[3], ref.element(raw.interior("V"), dtype))
        with pytest.raises(csi.CsiError, match="W == 0"):
            raw.ctx.output_snapshot(h)
    raw.ctx.output_destroy(h)


# ---- slots, errors ----------------------------------------------------------------------------------------------------------------------
def test_slots(raw):
    raw.grid(65, 7, 4, 4, TOPOS["pp"], names=["H"], seed=1)
    h = raw.ctx.output_create([("H", L.OUT_F64, 0, 0, 0.0)], 2)
    shape = [(7, 65)]
    xs = [np.full((7, 65), float(k)) + np.arange(65.0) / 64 for k in range(13)]
    raw.set("H", xs[0]); s0 = raw.ctx.output_snapshot(h)
    raw.set("H", xs[1]); s1 = raw.ctx.output_snapshot(h)
    assert (s0, s1) == (0, 1)
    raw.set("H", xs[2])
    with pytest.raises(csi.CsiError, match="no free slot") as e:          # refused, and nothing changes
        raw.ctx.output_snapshot(h)
    assert e.value.code == -1
    # wait on slot 1 returns slot 1's record while slot 0 is still in flight
    assert np.array_equal(ref.split_record(raw.ctx.output_wait(h, 1), shape, ["f64"])[0], xs[1])
    assert np.array_equal(ref.split_record(raw.ctx.output_wait(h, 0), shape, ["f64"])[0], xs[0])
    raw.ctx.output_release(h, 0)
    with pytest.raises(csi.CsiError, match="not in flight"):
        raw.ctx.output_wait(h, 0)
    with pytest.raises(csi.CsiError, match="not in flight"):
        raw.ctx.output_release(h, 0)
    with pytest.raises(csi.CsiError, match="slot out of range"):
        raw.ctx.output_test(h, 2)
    assert raw.ctx.output_snapshot(h) == 0                                # after a release it succeeds
    assert np.array_equal(raw.record(h, 1, shape, ["f64"])[0], xs[1])     # ... and the unreleased record was not touched
    assert np.array_equal(raw.record(h, 0, shape, ["f64"])[0], xs[2])
    # ten records through two slots arrive in order
    pending, got = [], []
    for k in range(3, 13):
        if len(pending) == 2:
            got.append(raw.record(h, pending.pop(0), shape, ["f64"])[0])
        raw.set("H", xs[k])
        pending.append(raw.ctx.output_snapshot(h))
    while pending:
        assert raw.ctx.output_test(h, pending[0]) in (True, False)
        got.append(raw.record(h, pending.pop(0), shape, ["f64"])[0])
    assert all(np.array_equal(g, x) for g, x in zip(got, xs[3:])) and len(got) == 10
    raw.ctx.output_destroy(h)
    with pytest.raises(csi.CsiError, match="bad handle"):
        raw.ctx.output_snapshot(h)


def test_create_errors_and_invalidation(raw):
    raw.grid(16, 4, 2, 2, TOPOS["pp"], names=["H", "A"], seed=2)
    for fields, slots, code, text in (([("U", 0, 0, 0, 0.0)], 1, -2, "field u is not bound"), ([("H", 2, 0, 0, 0.0)], 1, -1, "dtype"),
                                      ([("H", 0, 0, 0, 0.0)], 0, -1, "slots"), ([("H", 0, 0, 0, 0.0)], 65, -1, "slots"),
                                      ([], 1, -1, "n must be"), ([("H", 0, 0, 0, 0.0)] * 17, 1, -1, "n must be")):
        with pytest.raises(csi.CsiError, match=text) as e:
            raw.ctx.output_create(fields, slots)
        assert e.value.code == code
    hs = [raw.ctx.output_create([("H", 0, 0, 0, 0.0)], 1) for _ in range(4)]
    assert sorted(hs) == [1, 2, 3, 4]
    with pytest.raises(csi.CsiError, match="at most 4 output sets"):
        raw.ctx.output_create([("H", 0, 0, 0, 0.0)], 1)
    for h in hs[1:]:
        raw.ctx.output_destroy(h)
    # re-binding a field of the set to another array invalidates it; a field outside the set does not
    raw.keep = [raw.t["A"].clone(), raw.t["H"].clone()]
    other = raw.keep[0]
    raw.ctx.call("csi_field_bind", L.F["A"], C.c_void_p(other.data_ptr()), other.shape[1], other.shape[1], other.shape[0])
    raw.ctx.output_release(hs[0], raw.ctx.output_snapshot(hs[0]))
    other = raw.keep[1]
    raw.ctx.call("csi_field_bind", L.F["H"], C.c_void_p(other.data_ptr()), other.shape[1], other.shape[1], other.shape[0])
    with pytest.raises(csi.CsiError, match="field h was re-bound"):
        raw.ctx.output_snapshot(hs[0])
    raw.ctx.output_destroy(hs[0])
    h = raw.ctx.output_create([("H", 0, 0, 0, 0.0)], 1)
    met = L.Metrics()
    met.dx = met.dy = 1.0
    raw.ctx.call("csi_grid_set", 16, 4, 2, 2, L.PERIODIC, L.PERIODIC, L.METRIC_UNIFORM, C.byref(met))
    with pytest.raises(csi.CsiError, match="csi_grid_set was called"):
        raw.ctx.output_record_bytes(h)
    raw.ctx.output_destroy(h)


# ---- on a model -------------------------------------------------------------------------------------------------------------------------
def small_case():
    return cases.make_case(Nx=64, Ny=48, topo=("bounded", "bounded"), substeps=12, random_uv=0.02)


def small_model(c, mode="fast", **kw):
    return cases.csi_model(c, mode=mode, timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), **kw)


NAMES = ["h", "aice", "u", "v"]
PARENT_LAUNCHES = (6, 12)       # (kernel launches, sub-steps) of the last sub-cycle of one RK3 step of small_case()


def parents(m):
    m.synchronize()
    return {n: csi.bound_fields(m)[n][0].numpy().copy() for n in NAMES}


@pytest.fixture(scope="module")
def twin():
    """The twin model's parent arrays after 0 .. 12 steps, computed once and left unchanged."""
    c = small_case()
    m = small_model(c)
    states = [parents(m)]
    for k in range(12):
        csi.time_step(m, c["dt"])
        if k == 0:
            launches = m.ctx.last_launches()
        states.append(parents(m))
    return c, states, launches


def test_the_record_is_the_state_at_the_call(twin):
    c, states, _ = twin
    m = small_model(c)
    for _ in range(3):
        csi.time_step(m, c["dt"])
    h = m.ctx.output_create([(csi.bound_fields(m)[n][1], L.OUT_F64, 0, 0, 0.0) for n in NAMES], 1)
    slot = m.ctx.output_snapshot(h)
    for _ in range(3):                       # queued behind the pack launch without any synchronisation: they overwrite the fields
        csi.time_step(m, c["dt"])
    rec = m.ctx.output_wait(h, slot).copy()
    m.ctx.output_release(h, slot)
    shapes = [ref.interior(states[3][n], 4, 4).shape for n in NAMES]
    for n, got in zip(NAMES, ref.split_record(rec, shapes, ["f64"] * 4)):
        assert ref.same_bits(got, ref.interior(states[3][n], 4, 4)), n
    after = parents(m)
    assert all(ref.same_bits(after[n], states[6][n]) for n in NAMES)          # the snapshot did not disturb the run
    m.ctx.output_destroy(h)


@pytest.mark.parametrize("mode", ["fast", "strict"])
def test_front_end_end_to_end(twin, tmp_path, mode):
    c, states, _ = twin
    if mode == "strict":                     # another arithmetic: its own twin, stepped here beside the model
        t = small_model(c, mode=mode)
        states = [parents(t)]
    m = small_model(c, mode=mode)
    dt = c["dt"]
    m.output_writers["snap"] = csi.OutputWriter(m, NAMES, csi.IterationInterval(5), str(tmp_path / "snap"), dtype="f32")
    m.output_writers["avg"] = csi.OutputWriter(m, {"h": m.ice_thickness, "u": m.velocities.u}, csi.AveragedTimeInterval(4 * dt),
                                               str(tmp_path / "avg"), dtype="f64", slots=1)
    for k in range(12):
        csi.time_step(m, dt)
        if mode == "strict":
            csi.time_step(t, dt)
            states.append(parents(t))
    for w in m.output_writers.values():
        w.close()
    snap, avg = csi.load_output(str(tmp_path / "snap")), csi.load_output(str(tmp_path / "avg"))
    assert list(snap["iteration"]) == [0, 5, 10] and list(snap["time"]) == [0.0, 5 * dt, 10 * dt]
    for r, it in enumerate((0, 5, 10)):
        for n in NAMES:
            assert ref.same_bits(snap[n][r], ref.element(ref.interior(states[it][n], 4, 4), "f32")), (n, it)
    assert list(avg["time"]) == [4 * dt, 8 * dt, 12 * dt]
    for r in range(3):
        for n in ("h", "u"):
            want = ref.averaged([ref.interior(states[4 * r + k][n], 4, 4) for k in (1, 2, 3, 4)], [dt] * 4)
            assert ref.same_bits(avg[n][r], want), (n, r)


def test_unbound_field_is_refused_by_name(twin, tmp_path):
    c = twin[0]
    m = small_model(c)
    with pytest.raises(ValueError, match="'hs'"):
        csi.OutputWriter(m, ["h", "hs"], csi.IterationInterval(1), str(tmp_path / "a"))
    stray = csi.CenterField(m.grid, m.device, "stray")
    with pytest.raises(ValueError, match="'stray'"):
        csi.OutputWriter(m, {"stray": stray}, csi.IterationInterval(1), str(tmp_path / "b"))
    with csi.OutputWriter(m, ["sigma12", "top_u" if "top_u" in csi.bound_fields(m) else "Gn.h"], csi.IterationInterval(1),
                          str(tmp_path / "c"), dtype="f64") as w:
        w.write(m)
    got = csi.load_output(str(tmp_path / "c"))
    m.synchronize()
    assert ref.same_bits(got["sigma12"][0], ref.interior(m.dynamics.auxiliaries.fields.s12.numpy(), 4, 4))


def test_a_run_without_writers_launches_what_it_launched(twin, tmp_path, monkeypatch):
    """No writer attached: no output entry point is called, and csi_last_launches of a step is the parent commit's value for this
    configuration (PARENT_LAUNCHES: measured with the parent's build of the library).  A writer's launches are not part of it."""
    c, _, launches = twin
    assert launches == PARENT_LAUNCHES
    m = small_model(c)
    called = []
    for name in ("output_create", "output_accumulate", "output_snapshot"):
        monkeypatch.setattr(type(m.ctx), name, lambda self, *a, _n=name: called.append(_n))
    assert len(m.output_writers) == 0
    csi.time_step(m, c["dt"])
    assert called == [] and m.ctx.last_launches() == PARENT_LAUNCHES
    monkeypatch.undo()
    with csi.OutputWriter(m, NAMES, csi.IterationInterval(1), str(tmp_path / "w")) as w:
        m.output_writers["w"] = w
        csi.time_step(m, c["dt"])
        assert m.ctx.last_launches() == PARENT_LAUNCHES and len(w.pending) == 2


# ---- tiles ------------------------------------------------------------------------------------------------------------------------------
def test_tiles_write_their_own_interiors(twin, tmp_path):
    from test_gpu_local_tiles import run_tile_threads
    c, states, _ = twin
    dt, steps = c["dt"], 4

    def attach(m, root):
        m.output_writers["snap"] = csi.OutputWriter(m, NAMES, csi.IterationInterval(2), str(root / "snap"), dtype="f64")
        m.output_writers["avg"] = csi.OutputWriter(m, NAMES, csi.AveragedTimeInterval(2 * dt), str(root / "avg"), dtype="f32")

    def tile(rank, group):
        m = small_model(small_case(), tile=(2, 2, rank), local_group=group)
        attach(m, tmp_path / "tiled")
        for _ in range(steps):               # (the writers run inside time_step, after validate_all has returned)
            csi.time_step(m, dt)
        for w in m.output_writers.values():
            w.close()
        transport = m.ctx.halo_transport()
        del m
        return transport

    run_tile_threads(4, tile)
    snap, avg = csi.load_output(str(tmp_path / "tiled" / "snap")), csi.load_output(str(tmp_path / "tiled" / "avg"))
    assert list(snap["iteration"]) == [0, 2, 4] and list(avg["time"]) == [2 * dt, 4 * dt]
    for n in NAMES:
        for r, it in enumerate((0, 2, 4)):
            assert ref.same_bits(snap[n][r], ref.interior(states[it][n], 4, 4)), ("snap", n, it)
        for r in range(2):
            want = ref.element(ref.averaged([ref.interior(states[2 * r + k][n], 4, 4) for k in (1, 2)], [dt] * 2), "f32")
            assert ref.same_bits(avg[n][r], want), ("avg", n, r)
    assert snap["u"].shape == (3, 48, 65) and snap["v"].shape == (3, 49, 64)
