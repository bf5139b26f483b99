"""k_time_series (csrc/time_series.hip) and k_time_series_regrid (csrc/time_series_regrid.hip) on every alignment class of the bound
array and on the shapes at which their block layout can go wrong: the cases of tests/series_alignment_cases.py, whose coverage
tests/test_series_alignment_table.py proves.  Every other GPU test of the two kernels builds its grid with halo (4, 4) and so reaches
classes 0 and 1 only; here the first interior row also starts 8 bytes behind a 16-byte boundary (classes 2 and 3: the other two
layouts of a regrid map, the shifted ring of a HOST series), by the halo of a grid with csi.Field parents and by arrays bound by hand.

The oracles are the NumPy restatements the existing modules use (tests/time_series_ref.py, tests/regrid_ref.py) and EVERY comparison
is bit for bit: each line of the definition is two products and one sum in a stated order, compiled without contraction."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import regrid_ref as rref
import series_alignment_cases as T
import time_series_ref as tref
from test_gpu_time_series import (CONFIGS, STATE, TIMES, assert_same, dynamics_hook, forcing_data, omip_hook, state_of, write_omip_arrays)

pytestmark = pytest.mark.gpu
L = csi._lib
DEV = "cuda:0"
LOC = {"fc": (csi.Face, csi.Center), "cf": (csi.Center, csi.Face), "cc": (csi.Center, csi.Center)}
LOCATION = {"fc": L.REGRID_FACE_CENTER, "cf": L.REGRID_CENTER_FACE, "cc": L.REGRID_CENTER_CENTER}
SENTINEL, UNUSED = -777.0, 1e300              # what the parents hold outside the interior / the series' own padding
INVALID_ARGUMENT = -1                         # CSI_ERR_INVALID_ARGUMENT
NONUNIFORM = np.array([3.0, 10.0, 11.0, 40.0, 41.5])
# a node (n1 == n2, the `same` path), between nodes, below the first and above the last slice (Linear: weights outside [0, 1])
PROBE = (10.0, 5.1, -20.0, 100.0)
MODES = (("strict", L.MODE_STRICT), ("fast", L.MODE_FAST))


def source_nodes(Nx, Ny, periodic):
    """(x nodes, y nodes) of a source grid in the coordinates of RectilinearGrid((Nx, Ny), x=(0, Nx), y=(0, Ny)), for any Nx, Ny >= 1:
    7 x 3 periodic in x with the inferred period (the wrap gap lies inside the grid), y nodes beyond it; 5 x 4 bounded, columns and rows
    clamp at both ends."""
    if periodic:
        return np.linspace(0.0, Nx, 7, endpoint=False), np.linspace(-1.0, Ny + 1.0, 3)
    return np.linspace(0.25 * Nx, 0.8 * Nx, 5), np.linspace(0.4, Ny - 0.3, 4)


class Target:
    """One bound array: a csi.Field parent (base on a 16-byte boundary, ld = ni) or, bound by hand, a flat buffer whose base lies
    base_off doubles into it and whose rows are ld doubles apart.  The WHOLE buffer holds the sentinel -- ld padding, the element
    before an offset base and one behind the last row included."""

    def __init__(self, grid, halo, loc, interior, base_off=None, ld_extra=0, name=""):
        self.Hx, self.Hy = halo
        self.ny, self.nx = interior
        self.ni, self.nj = self.nx + 2 * self.Hx, self.ny + 2 * self.Hy
        if base_off is None:
            self.field = csi.Field(LOC[loc], grid, DEV, name)
            assert (self.field.ni, self.field.nj) == (self.ni, self.nj)
            self.flat, self.base_off, self.ld = self.field.data.view(-1), 0, self.ni
        else:
            self.base_off, self.ld = base_off, self.ni + ld_extra
            self.flat = torch.empty(base_off + self.nj * self.ld + 1, dtype=torch.float64, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.flat.fill_(SENTINEL)
        self.ptr = self.flat.data_ptr() + 8 * self.base_off
        j, i = np.meshgrid(np.arange(self.ny), np.arange(self.nx), indexing="ij")
        self.index = self.base_off + (self.Hy + j) * self.ld + self.Hx + i
        self.first = self.ptr + 8 * (self.Hx + self.Hy * self.ld)
        self.cls = T.class_of_address(self.first, self.ld)

    def bind(self, ctx, slot):
        ctx.call("csi_field_bind", L.F[slot], C.c_void_p(self.ptr), self.ld, self.ni, self.nj)

    def refill(self):
        self.flat.fill_(SENTINEL)
        torch.cuda.synchronize()

    def read(self, what=()):
        """the interior, after asserting that every other element of the buffer still holds the sentinel"""
        flat = self.flat.cpu().numpy()
        outside = np.ones(flat.size, dtype=bool)
        outside[self.index] = False
        assert np.all(flat[outside] == SENTINEL), (what, "written outside the interior at flat index", np.flatnonzero(outside & (flat != SENTINEL))[:6].tolist(),
                                                   "base_off, ld", (self.base_off, self.ld))
        return flat[self.index]


class Bench:
    """A bare context with a Bounded x Bounded grid; slots bound to Targets, series set through the ABI."""

    def __init__(self, Nx, Ny, halo):
        self.Nx, self.Ny, self.halo = Nx, Ny, halo
        self.g = csi.RectilinearGrid((Nx, Ny), x=(0.0, float(Nx)), y=(0.0, float(Ny)), topology=(csi.Bounded, csi.Bounded), halo=halo)
        self.ctx = L.Context(0)
        met = L.Metrics()
        met.dx = met.dy = 1.0
        self.ctx.call("csi_grid_set", Nx, Ny, halo[0], halo[1], L.BOUNDED, L.BOUNDED, L.METRIC_UNIFORM, C.byref(met))
        self.keep, self.before, self.targets, self.want, self.maps = [], [], {}, {}, {}

    def close(self):
        self.ctx.call("csi_sync")
        self.ctx.close()

    def interior(self, loc):
        return self.Ny + T.LOCS[loc][1], self.Nx + T.LOCS[loc][0]

    def target(self, slot, base_off=None, ld_extra=0):
        loc = T.SLOT_LOC[slot]
        t = Target(self.g, self.halo, loc, self.interior(loc), base_off, ld_extra, slot.lower())
        torch.cuda.synchronize()
        t.bind(self.ctx, slot)
        self.targets[slot] = t
        return t

    def series(self, data, backend, kind=L.TIME_LINEAR, pad=0, src_off=0, window=3, times=NONUNIFORM, period=0.0):
        """A csi_time_series over data (nt, ny, nx) in a layout of its own: pad extra doubles per row and pad extra rows per slice,
        the base src_off doubles behind the (16-byte aligned) start of its buffer."""
        nt, ny, nx = data.shape
        ld, stride = nx + pad, (ny + pad) * (nx + pad)
        lay = np.full(src_off + nt * stride + 1, UNUSED)
        view = lay[src_off:src_off + nt * stride].reshape(nt, ny + pad, nx + pad)
        view[:, :ny, :nx] = data
        times = np.ascontiguousarray(times, dtype=np.float64)
        held = torch.from_numpy(lay).to(DEV) if backend == "device" else lay
        ptr = (held.data_ptr() if backend == "device" else lay.ctypes.data)
        assert backend != "device" or ptr % 16 == 0
        st = L.TimeSeries(nt, kind, L.SERIES_DEVICE if backend == "device" else L.SERIES_HOST, window, period,
                          times.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(ptr + 8 * src_off), ld, stride)
        self.keep += [held, times, st]
        self.before.append((held, lay.copy()))
        torch.cuda.synchronize()
        return st

    def map(self, loc, rotated, rng):
        """one library map per (location, rotated): (map id, the restatement's plan, (cos, sin) or None)"""
        key = (loc, rotated)
        if key not in self.maps:
            xs, ys = source_nodes(self.Nx, self.Ny, periodic=loc != "cf")
            m = rref.plan_points(xs, ys, loc != "cf", 0.0, *self.g.target_nodes(*LOC[loc]))
            rot = None
            if rotated:
                th = rng.uniform(-np.pi, np.pi, size=self.interior(loc))
                rot = (np.cos(th), np.sin(th))
            self.maps[key] = (self.ctx.regrid_map_create(LOCATION[loc], *m, (ys.size, xs.size), *(rot or (None, None))), m, rot, (ys.size, xs.size))
        return self.maps[key]

    def set_series(self, slot, rng, backend, pad=0, src_off=0, **kw):
        data = _draw(rng, self.interior(T.SLOT_LOC[slot]))
        st = self.series(data, backend, pad=pad, src_off=src_off, **kw)
        self.ctx.call("csi_time_series_set", L.F[slot], C.byref(st))
        times, kind, period = kw.get("times", NONUNIFORM), kw.get("kind", L.TIME_LINEAR), kw.get("period", 0.0)
        self.want[slot] = lambda t: tref.at(times, data, kind, period, t)

    def set_regridded(self, slot, role, rng, backend, pad=0, src_off=0, shared=False):
        loc = T.SLOT_LOC[slot]
        pair = role != "scalar"
        map_id, m, rot, shape = self.map(loc, pair and not shared, rng)
        east = _draw(rng, shape)
        st = self.series(east, backend, pad=pad, src_off=src_off)
        if pair:
            north, comp = _draw(rng, shape), 0 if role == "pair_x" else 1
            other = self.series(north, backend, pad=pad, src_off=1 - src_off)
            self.ctx.call("csi_time_series_set_regridded", L.F[slot], C.byref(st), map_id, C.byref(other), comp)
            self.want[slot] = lambda t: rref.pair_at(NONUNIFORM, east, north, L.TIME_LINEAR, 0.0, t, m, rot[0], rot[1], comp)
        else:
            self.ctx.call("csi_time_series_set_regridded", L.F[slot], C.byref(st), map_id, None, 0)
            self.want[slot] = lambda t: rref.at(NONUNIFORM, east, L.TIME_LINEAR, 0.0, t, m)

    def update(self, t):
        self.ctx.time_series_update(t)
        self.ctx.call("csi_sync")

    def check(self, t, what=(), slots=None):
        for slot in slots or self.want:
            want, got = self.want[slot](t), self.targets[slot].read((what, slot, t))
            assert got.shape == want.shape, (what, slot, got.shape, want.shape)
            assert np.array_equal(got, want), (what, slot, t, "class", self.targets[slot].cls, "points that differ (j, i)",
                                               np.argwhere(got != want)[:6].tolist(), "of", got.shape)

    def sources_untouched(self):
        for held, copy in self.before:
            now = held.cpu().numpy() if isinstance(held, torch.Tensor) else held
            assert now.tobytes() == copy.tobytes()


def _draw(rng, shape):
    return rng.standard_normal((T.NT,) + tuple(shape)) * 10.0 ** rng.integers(-3, 3, size=(T.NT, 1, 1))


@pytest.fixture
def bench():
    made = []

    def make(*a, **k):
        made.append(Bench(*a, **k))
        return made[-1]
    yield make
    for b in made:
        b.close()


# ---- every case of the table -----------------------------------------------------------------------------------------------------------
def test_the_probe_times():
    plans = [tref.plan(NONUNIFORM, L.TIME_LINEAR, 0.0, t) for t in PROBE]
    assert plans[0][:2] == (1, 1) and plans[1][:2] == (0, 1) and 0.0 < plans[1][2] < 1.0
    assert plans[2][2] < 0.0 and plans[3][2] > 1.0


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_update_equals_the_restatement(case, bench):
    """Every slot of the case set and updated at the four probe times in STRICT and in FAST: the interior equals the restatement bit for
    bit, every other element of the parent -- ld padding, the element before an offset base -- still holds the sentinel, the sources
    are byte-identical afterwards; the arrays have the classes the table computed for them."""
    b = bench(case.Nx, case.Ny, case.halo)
    rng = np.random.default_rng(sum(map(ord, case.id)))
    for s in case.slots:
        t = b.target(s.name, *((None, 0) if case.route == "halo" else (s.base_off, s.ld_extra)))
        assert (t.nj, t.ni, t.ld) == T.parent(case, s) and (t.ny, t.nx) == T.interior(case, s)
        assert t.cls == T.alignment_class(case, s), (case.id, s.name, t.cls)
        assert (case.route == "halo") == hasattr(t, "field")
    for s in case.slots:
        if case.kernel == "series":
            b.set_series(s.name, rng, case.backend, s.pad, s.src_off)
        else:
            b.set_regridded(s.name, s.role, rng, case.backend, s.pad, s.src_off, shared=case.shared)
    maps = len(b.maps)
    assert maps == (0 if case.kernel == "series" else (1 if case.shared else len(case.slots)))
    updates = 0
    for name, mode in MODES:
        b.ctx.call("csi_set_mode", mode)
        for t in PROBE:
            b.update(t)
            updates += 1
            b.check(t, (case.id, name))
            # one launch of the regridding kernel per update, whatever the number of slots; the maps alive are the ones made
            assert b.ctx.regrid_stats() == (updates if case.kernel == "regrid" else 0, maps)
    b.sources_untouched()


# ---- the shifted ring of a HOST series ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,window", [(10, 3), (9, 2)], ids=["nt10_window3", "nt9_window2"])
def test_window_residency_and_upload_counts_on_classes_2_and_3(nt, window, bench):
    """tests/test_gpu_time_series.py's walk (test_window_residency_and_upload_counts) on a halo (3, 2) grid: the (Face, Center) field is
    of class 3, the (Center, Face) one of class 2 -- the ring slices start one double into their allocation."""
    b = bench(130, 5, (3, 2))
    tu, tv = b.target("TOP_U"), b.target("TOP_V")
    assert (tu.cls, tv.cls) == (3, 2)
    rng = np.random.default_rng(nt)
    times = np.arange(nt) * 1.0
    period = float(nt)                                              # (what Cyclical infers)
    data = {}
    for slot, t in (("TOP_U", tu), ("TOP_V", tv)):
        data[slot] = rng.standard_normal((nt, t.ny, t.nx))
        st = b.series(data[slot], "host", kind=L.TIME_CYCLICAL, window=window, times=times, pad=1)
        b.ctx.call("csi_time_series_set", L.F[slot], C.byref(st))
        b.want[slot] = lambda t, d=data[slot]: tref.at(times, d, L.TIME_CYCLICAL, 0.0, t)
        assert b.ctx.time_series_status(slot, window) == ([-1] * window, 0)
    walk = [0.3 + k * (2.5 * period / 40.0) for k in range(40)]
    entries, prev = 0, None
    for k, t in enumerate(walk):
        n1, n2, _ = tref.plan(times, L.TIME_CYCLICAL, 0.0, t)
        assert n1 != n2
        b.update(t)
        b.check(t, (nt, window, k))
        if prev is None:
            entries = 3 if window == 3 else 2
        elif (n1, n2) != prev:
            assert n1 == prev[1]                                    # (the walk skips no interval)
            entries += 1
        for slot in ("TOP_U", "TOP_V"):
            resident, uploads = b.ctx.time_series_status(slot, window)
            assert n1 in resident and n2 in resident, (slot, k, t, (n1, n2), resident)
            assert len(set(r for r in resident if r >= 0)) == len([r for r in resident if r >= 0])
            if window == 3:
                assert (n2 + 1) % nt in resident, (slot, k, t, resident)      # already there before the walk reaches it
            assert uploads == entries, (slot, k, t, uploads, entries)           # one slice per change of interval, never one per step
        prev = (n1, n2)
    assert entries < len(walk)
    for t in (walk[-1] + 5.0, walk[-1] + 5.0 - 7.0, walk[0]):
        n1, n2, _ = tref.plan(times, L.TIME_CYCLICAL, 0.0, t)
        b.update(t)
        b.check(t, (nt, window, "jump", t))
        for slot in ("TOP_U", "TOP_V"):
            resident, _ = b.ctx.time_series_status(slot, window)
            assert n1 in resident and n2 in resident, (slot, t, (n1, n2), resident)
    b.sources_untouched()


# ---- re-binding a driven slot ---------------------------------------------------------------------------------------------------------------
# On a 130 x 5 grid with halo (4, 4) the (Center, Center) parent is 138 doubles wide: an array bound by hand has class
# 2 * base_off + ld_extra.  Transitions: the first row's alignment only (same ld), the row stride only, both.
LAYOUT_OF_CLASS = {0: (0, 0), 1: (0, 1), 2: (1, 0), 3: (1, 1)}
TRANSITIONS = ((0, 2), (2, 3), (3, 0), (1, 2))


@pytest.mark.parametrize("backend", T.BACKENDS)
@pytest.mark.parametrize("kind", ["series", "regrid"])
def test_rebinding_to_another_class_is_refused_until_the_series_is_set_again(kind, backend, bench):
    """After a set, the slot bound to an array of another class: a HOST series on the model grid (whose ring has the old array's row
    stride and alignment) and a regridded series of either backend (whose map layout is the old class's) refuse the update by name, a
    fresh set makes it succeed; another array of the SAME class and ld needs no new set.  (A DEVICE series on the model grid reads the
    caller's slices with whatever alignment they have: k_time_series takes any destination, so its update succeeds.)"""
    rng = np.random.default_rng(17)
    for old, new in TRANSITIONS:
        b = bench(130, 5, (4, 4))
        first = b.target("SNOWFALL", *LAYOUT_OF_CLASS[old])
        assert first.cls == old

        def set_():
            if kind == "series":
                b.set_series("SNOWFALL", rng, backend, pad=1)
            else:
                b.set_regridded("SNOWFALL", "scalar", rng, backend, pad=1)
        set_()
        b.update(5.1)
        b.check(5.1, (kind, backend, old, "first array"))
        # another array of the same class and ld: no new set, and the NEW array is written (the old one not at all)
        first.refill()
        same = b.target("SNOWFALL", *LAYOUT_OF_CLASS[old])
        assert same.cls == old and same.ptr != first.ptr
        b.update(20.0)
        b.check(20.0, (kind, backend, old, "second array of the same class"))
        assert np.all(first.flat.cpu().numpy() == SENTINEL)
        # an array of another class
        other = b.target("SNOWFALL", *LAYOUT_OF_CLASS[new])
        assert other.cls == new
        if kind == "series" and backend == "device":
            b.update(12.5)
        else:
            with pytest.raises(csi.CsiError, match="snowfall: the field was re-bound with another") as e:
                b.ctx.time_series_update(12.5)
            assert e.value.code == INVALID_ARGUMENT
            b.ctx.call("csi_sync")
            assert np.all(other.flat.cpu().numpy() == SENTINEL)       # (refused before anything was launched)
            set_()
            b.update(12.5)
        b.check(12.5, (kind, backend, old, new, "after the set on the new class"))
        if kind == "regrid":
            assert b.ctx.regrid_stats() == (3, 1)                     # two layouts of the one map; refused updates launch nothing
        b.sources_untouched()


# ---- the front end off the (4, 4) halo ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["device", "host"])
def test_series_driven_evp_run_equals_hand_updated_run_on_halo_5_3(backend):
    """tests/test_gpu_time_series.py's test_series_driven_evp_run_equals_hand_updated_run, config stress_ocean_freedrift, on a
    halo = (5, 3) grid of its 64 x 48 size: csi.FieldTimeSeries drives six class-2 arrays (74 doubles wide, the interior 5 + 3 * 74
    doubles in).  WENO5 in place of WENO7, which needs four halo rows."""
    config = "stress_ocean_freedrift"
    assert CONFIGS[config][:2] == (("tu", "tv"), True)              # stress arrays, ocean velocities and free-drift fields: six series
    c = cases.make_case(Nx=64, Ny=48, H=(5, 3), topo=("periodic", "bounded"), substeps=12, random_uv=0.05, land=0.15)
    assert (c["g"].Hx, c["g"].Hy) == (5, 3)
    data = forcing_data(c["g"])
    kw = dict(mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    held = []
    with dynamics_hook(omip_hook(data, True, held, config, backend=csi.InMemory() if backend == "device" else csi.InMemory(3))):
        A = cases.csi_model(c, **kw)
    with dynamics_hook(omip_hook(data, False, held, config)):
        B = cases.csi_model(c, **kw)
    assert sorted(A._series) == ["BOT_U", "BOT_V", "FREE_DRIFT_U", "FREE_DRIFT_V", "TOP_U", "TOP_V"] and not B._series
    for comp in "UV":
        f = A.external_stress_field("TOP", comp)
        assert T.class_of_address(f.data.data_ptr() + 8 * (5 + 3 * f.ni), f.ni) == 2
    crossed = set()
    for n in range(5):
        crossed.add(tref.plan(TIMES, L.TIME_LINEAR, 0.0, A.clock.time)[:2])
        write_omip_arrays(B, data, B.clock.time, config)
        csi.time_step(A, c["dt"])
        csi.time_step(B, c["dt"])
        assert_same(state_of(A, STATE), state_of(B, STATE), (backend, "step", n))
        assert A.ctx.last_path() == B.ctx.last_path() and A.ctx.last_launches() == B.ctx.last_launches()
    assert len(crossed) >= 2                                        # the steps crossed a slice boundary
    assert A.clock.time == B.clock.time == 5 * c["dt"]
    A.clock.time = B.clock.time = 777.0
    write_omip_arrays(B, data, 777.0, config)
    for step in (lambda m: csi.time_step_momentum(m, c["dt"]), csi.update_state):
        step(A); step(B)
    assert_same(state_of(A, STATE), state_of(B, STATE), (backend, "momentum step on its own"))
    for slot in ("TOP", "BOT"):                                     # halos included
        assert np.array_equal(A.external_stress_field(slot, "U").numpy(), B.external_stress_field(slot, "U").numpy())
