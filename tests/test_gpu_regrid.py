"""Forcing time series on a rectilinear source grid, regridded on the device (include/csi.h: csi_regrid_map_create,
csi_time_series_set_regridded, csi_regrid_stats; csrc/time_series_regrid.hip, csrc/csi_time_series.hip; csi.SourceGrid,
csi.RegriddedTimeSeries, csi.RegriddedVectorTimeSeries).  The oracle is the NumPy restatement tests/regrid_ref.py; EVERY comparison is
bit for bit, in both modes: each line of the definition is two products and one sum in a stated order."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import regrid_ref as ref
import time_series_ref as tref
from test_gpu_local_tiles import run_tile_threads
from test_gpu_time_series import EVP_FIELDS, assert_same, dynamics_hook, state_of

pytestmark = pytest.mark.gpu
L = csi._lib
FC, CF, CC = (csi.Face, csi.Center), (csi.Center, csi.Face), (csi.Center, csi.Center)
LOCATION = {FC: L.REGRID_FACE_CENTER, CF: L.REGRID_CENTER_FACE, CC: L.REGRID_CENTER_CENTER}
SLOT_LOC = dict(TOP_U=FC, TOP_V=CF, BOT_U=FC, BOT_V=CF, FORCING_U=FC, FORCING_V=CF, FREE_DRIFT_U=FC, FREE_DRIFT_V=CF,
                TOP_HEAT_FLUX=CC, BOTTOM_HEAT_FLUX=CC, SNOWFALL=CC)
NONUNIFORM = np.array([3.0, 10.0, 11.0, 40.0, 41.5])
# a node (n1 == n2), between nodes, below the first and above the last slice (Linear: the weight leaves [0, 1]), the last node
PROBE = (10.0, 5.1, 11.0 + 1e-9, -20.0, 100.0, 41.5)


def sources(Nx, Ny):
    """The three source grids in the coordinates of RectilinearGrid((Nx, Ny), x=(0, Nx), y=(0, Ny)) -- centres at k - 1/2, faces at k:
    8 x 5 periodic: the first x node ON the first centre, a period shorter than the grid (targets in the wrap gap, one and more periods
      up, and -- the face at 0 -- below the first node); y nodes on centres 2 and Ny - 1, so rows clamp at both ends;
    5 x 4 bounded: x nodes on faces 2 and Nx - 3 (columns clamp at both ends), y from the first to the last centre (face row 0 clamps);
    33 x 17 periodic: finer than the 37 x 29 target in x, the inferred period, y nodes beyond the grid (nothing clamps)."""
    return {"8x5_periodic": csi.SourceGrid(np.linspace(0.5, 0.7 * Nx, 8), np.linspace(1.5, Ny - 1.5, 5), periodic_x=True, period=0.9 * Nx),
            "5x4_bounded": csi.SourceGrid(np.linspace(2.0, Nx - 3.0, 5), np.linspace(0.5, Ny - 0.5, 4)),
            "33x17_periodic": csi.SourceGrid(np.linspace(0.0, Nx, 33, endpoint=False), np.linspace(-1.0, Ny + 1.0, 17), periodic_x=True)}


# ---- the ABI driven directly: a bare context (a model without dynamics), fields bound by hand ------------------------------------------
class Driver:
    def __init__(self, Nx, Ny, topo=(csi.Bounded, csi.Periodic), mode="fast"):
        self.g = csi.RectilinearGrid((Nx, Ny), x=(0.0, float(Nx)), y=(0.0, float(Ny)), topology=topo, halo=(4, 4))
        self.m = csi.SeaIceModel(self.g, dynamics=None, advection=None, timestepper="ForwardEuler", mode=mode)
        self.fields, self.keep, self.spec, self.maps, self.before = {}, [], {}, {}, {}

    def plan(self, src, loc):
        return ref.plan_points(src.x, src.y, src.periodic_x, src.period, *self.g.target_nodes(*loc))

    def map(self, src, loc, rotation=None):
        """One library map per (source, location); rotation: (cos, sin) arrays, default none."""
        key = (id(src), loc, rotation is not None)
        if key not in self.maps:
            m = self.plan(src, loc)
            self.maps[key] = (self.m.ctx.regrid_map_create(LOCATION[loc], *m, src.shape, *(rotation or (None, None))), m)
            self.keep.append(src)
        return self.maps[key]

    def bind(self, slot, halo=-777.0):
        fld = csi.Field(SLOT_LOC[slot], self.g, self.m.device, slot.lower())
        fld.fill_parent(halo)                                          # the halo must stay untouched
        self.m._bind(slot, fld)
        self.fields[slot] = fld
        return fld

    def series(self, times, data, kind, period=0.0, backend="device", window=3, pad=0):
        """A csi_time_series over `data` (Nt, sy, sx); pad: extra doubles per row and extra rows per slice of the series' own layout."""
        nt, ny, nx = data.shape
        lay = np.full((nt, ny + pad, nx + pad), 1e300)
        lay[:, :ny, :nx] = data
        times = np.ascontiguousarray(times, dtype=np.float64)
        held = torch.from_numpy(lay).to(self.m.device) if backend == "device" else lay
        ptr = held.data_ptr() if backend == "device" else lay.ctypes.data
        st = L.TimeSeries(nt, kind, L.SERIES_DEVICE if backend == "device" else L.SERIES_HOST, window, period,
                          times.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(ptr), nx + pad, (ny + pad) * (nx + pad))
        self.keep += [held, times, st]
        self.before[id(st)] = (held, lay.copy())
        return st

    def add(self, slot, src, times, data, kind, period=0.0, north=None, component=0, rotation=None, **kw):
        if slot not in self.fields:
            self.bind(slot)
        map_id, m = self.map(src, SLOT_LOC[slot], rotation)
        st = self.series(times, data, kind, period, **kw)
        other = self.series(times, north, kind, period, **kw) if north is not None else None
        torch.cuda.synchronize()
        self.m.ctx.call("csi_time_series_set_regridded", L.F[slot], C.byref(st), map_id, C.byref(other) if other is not None else None, component)
        self.spec[slot] = (times, data, north, kind, period, m, rotation, component, kw.get("window", 3) if kw.get("backend") == "host" else 0)

    def update(self, t):
        self.m.ctx.time_series_update(t)
        self.m.synchronize()

    def want(self, slot, t):
        times, data, north, kind, period, m, rotation, component, _ = self.spec[slot]
        if north is None:
            return ref.at(times, data, kind, period, t, m)
        return ref.pair_at(times, data, north, kind, period, t, m, rotation[0], rotation[1], component)

    def check(self, t, what=()):
        for slot in self.spec:
            want, got = self.want(slot, t), self.fields[slot].interior_numpy()
            assert got.shape == want.shape, (slot, got.shape, want.shape)
            assert np.array_equal(got, want), (what, slot, t, np.abs(got - want).max(), np.argwhere(got != want)[:4].tolist())

    def sources_untouched(self):
        for held, copy in self.before.values():
            now = held.cpu().numpy() if isinstance(held, torch.Tensor) else held
            assert now.tobytes() == copy.tobytes()

    def status(self, slot):
        return self.m.ctx.time_series_status(slot, self.spec[slot][8])


def _rotation(rng, shape):
    th = rng.uniform(-np.pi, np.pi, size=shape)
    return np.cos(th), np.sin(th)


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("source", ["8x5_periodic", "5x4_bounded", "33x17_periodic"])
@pytest.mark.parametrize("shape", [(37, 29), (64, 4), (65, 5), (130, 9)], ids=["37x29", "64x4", "65x5", "130x9"])
def test_update_equals_the_restatement(shape, source, mode):
    """One scalar slot per location on a Bounded x Periodic grid -- the (Face, Center) interior is one column wider, so rows of odd and
    even length, rows that start on and off a 16-byte boundary, lone first / last points and more than one 128 x 8 block occur --, at six
    times: a node (n1 == n2), between nodes, and beyond both ends under Linear (weights outside [0, 1])."""
    Nx, Ny = shape
    d = Driver(Nx, Ny, mode=mode)
    src = sources(Nx, Ny)[source]
    rng = np.random.default_rng(Nx + Ny)
    for k, slot in enumerate(("TOP_U", "TOP_V", "SNOWFALL")):
        d.add(slot, src, NONUNIFORM, rng.standard_normal((5,) + src.shape) * 10.0 ** rng.integers(-3, 3, size=(5, 1, 1)), L.TIME_LINEAR, pad=k)
    assert d.fields["TOP_U"].interior_numpy().shape == (Ny, Nx + 1)
    m = d.spec["TOP_U"][5]
    if source == "8x5_periodic":
        mv = d.spec["TOP_V"][5]
        assert ((m[0] == 7) & (m[1] == 0)).any() and (m[2] == m[3]).any()                                 # the wrap gap (the face at 0), clamped rows
        assert (mv[4][:, 0] == 0.0).all() and (mv[0][:, 0] == mv[1][:, 0]).all()                          # the first centre ON a source node
        assert (m[2][0] == 0).all() and (m[2][-1] == 4).all() and (m[5][0] == 0).all() and (m[5][-1] == 0).all()
    if source == "5x4_bounded":
        assert (m[0][:, 0] == 0).all() and (m[0][:, -1] == 4).all() and (m[4][:, 2] == 0.0).all()         # clamped columns, face 2 on a node
    frac = [tref.plan(NONUNIFORM, L.TIME_LINEAR, 0.0, t)[2] for t in PROBE]
    assert min(frac) < 0.0 and max(frac) > 1.0 and tref.plan(NONUNIFORM, L.TIME_LINEAR, 0.0, PROBE[0])[:2] == (1, 1)
    for t in PROBE:
        d.update(t)
        d.check(t, (shape, source, mode))
    assert d.m.ctx.regrid_stats() == (len(PROBE), 3)                  # three slots, one launch per update; one map per location
    for slot, fld in d.fields.items():                                # nothing but the interior was written
        full = fld.numpy().copy()
        ny, nx = fld.interior_numpy().shape
        full[4:4 + ny, 4:4 + nx] = -777.0
        assert np.all(full == -777.0), slot
    d.sources_untouched()


def test_halos_holding_huge_values_and_nan_stay_and_sources_are_untouched():
    d = Driver(37, 29)
    src = sources(37, 29)["8x5_periodic"]
    rng = np.random.default_rng(1)
    flds = {"TOP_U": d.bind("TOP_U", 1e300), "SNOWFALL": d.bind("SNOWFALL", np.nan)}
    for slot in flds:
        d.add(slot, src, NONUNIFORM, rng.standard_normal((5,) + src.shape), L.TIME_CLAMP, pad=1)
    d.update(7.0)
    d.check(7.0)
    for slot, fld in flds.items():
        full = fld.numpy()
        ny, nx = fld.interior_numpy().shape
        halo = np.ones(full.shape, dtype=bool)
        halo[4:4 + ny, 4:4 + nx] = False
        assert np.all(full[halo] == 1e300) if slot == "TOP_U" else np.all(np.isnan(full[halo])), slot
        assert np.isfinite(full[~halo]).all()
    d.sources_untouched()


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_scalar_slots_a_pair_and_a_model_grid_series_side_by_side(mode):
    """Five regridded slots -- three scalars from two source grids, the two components of a rotated pair -- and a series on the model
    grid in one update: one launch of each kernel, whatever the number of slots."""
    Nx, Ny = 65, 29
    d = Driver(Nx, Ny, topo=(csi.Bounded, csi.Bounded), mode=mode)
    S = sources(Nx, Ny)
    rng = np.random.default_rng(12)
    draw = lambda src, nt: rng.standard_normal((nt,) + src.shape)      # noqa: E731
    rot = {loc: _rotation(rng, tuple(reversed(d.g.interior_size(*loc)))) for loc in (FC, CF)}
    wind = S["33x17_periodic"]
    t5 = np.cumsum(0.5 + rng.random(5))
    east, north = draw(wind, 5), draw(wind, 5)
    d.add("TOP_U", wind, t5, east, L.TIME_CYCLICAL, 0.0, north=north, component=0, rotation=rot[FC])
    d.add("TOP_V", wind, t5, east, L.TIME_CYCLICAL, 0.0, north=north, component=1, rotation=rot[CF], backend="host", window=2)
    d.add("BOT_U", S["5x4_bounded"], NONUNIFORM, draw(S["5x4_bounded"], 5), L.TIME_LINEAR, pad=2)
    d.add("TOP_HEAT_FLUX", S["8x5_periodic"], [0.0, 4.0], draw(S["8x5_periodic"], 2), L.TIME_CLAMP, backend="host")
    d.add("SNOWFALL", wind, t5, draw(wind, 5), L.TIME_LINEAR)
    # ... and FORCING_V on the model grid
    fld = d.bind("FORCING_V")
    ny, nx = fld.interior_numpy().shape
    plain = rng.standard_normal((5, ny, nx))
    st = d.series(NONUNIFORM, plain, L.TIME_LINEAR)
    torch.cuda.synchronize()
    d.m.ctx.call("csi_time_series_set", L.F["FORCING_V"], C.byref(st))
    assert d.m.ctx.regrid_stats() == (0, 5)                           # maps: wind at fc (rotated), cf (rotated), cc; bounded at fc; 8x5 at cc
    times = (-1.0, 0.7, 3.3, 10.0, 11.5, 57.0)
    for n, t in enumerate(times):
        d.update(t)
        d.check(t, mode)
        assert np.array_equal(fld.interior_numpy(), tref.at(NONUNIFORM, plain, L.TIME_LINEAR, 0.0, t))
        assert d.m.ctx.regrid_stats()[0] == n + 1
    # replacing a regridded slot by a model-grid series and back, removing one: the launch count follows the updates, not the slots
    d.m.ctx.call("csi_time_series_set", L.F["SNOWFALL"], None)
    del d.spec["SNOWFALL"]
    d.update(2.0)
    d.check(2.0, "after removing a slot")
    assert d.m.ctx.regrid_stats()[0] == len(times) + 1
    with pytest.raises(csi.CsiError, match="no series"):
        d.m.ctx.time_series_status("SNOWFALL", 0)
    d.sources_untouched()


# ---- the device window of a host-resident series: source-sized slices, one ring per source series -----------------------------------------
@pytest.mark.parametrize("nt,window", [(10, 3), (9, 2)], ids=["nt10_window3", "nt9_window2"])
def test_window_residency_and_upload_counts_of_a_pair(nt, window):
    """tests/test_gpu_time_series.py's walk, for the x component of a pair (two rings; the status reports the east one -- the north one is
    checked through the values) and a scalar slot: 40 times through two and a half periods, then jumps forward, backward and to the start."""
    Nx, Ny = 37, 29
    d = Driver(Nx, Ny)
    src = sources(Nx, Ny)["33x17_periodic"]
    rng = np.random.default_rng(nt)
    times = np.arange(nt) * 1.0
    period = float(nt)                                              # (what Cyclical infers)
    rot = _rotation(rng, (Ny, Nx + 1))
    d.add("TOP_U", src, times, rng.standard_normal((nt,) + src.shape), L.TIME_CYCLICAL, 0.0, north=rng.standard_normal((nt,) + src.shape),
          component=0, rotation=rot, backend="host", window=window)
    d.add("SNOWFALL", src, times, rng.standard_normal((nt,) + src.shape), L.TIME_CYCLICAL, 0.0, backend="host", window=window, pad=1)
    assert d.status("TOP_U") == ([-1] * window, 0) and d.status("SNOWFALL") == ([-1] * window, 0)
    walk = [0.3 + k * (2.5 * period / 40.0) for k in range(40)]
    entries, prev = 0, None
    for k, t in enumerate(walk):
        n1, n2, _ = tref.plan(times, L.TIME_CYCLICAL, 0.0, t)
        assert n1 != n2
        d.update(t)
        d.check(t, (nt, window, k))
        if prev is None:
            entries = 3 if window == 3 else 2
        elif (n1, n2) != prev:
            assert n1 == prev[1]                                    # (the walk skips no interval)
            entries += 1
        for slot in ("TOP_U", "SNOWFALL"):
            resident, uploads = d.status(slot)
            assert n1 in resident and n2 in resident, (slot, k, t, (n1, n2), resident)
            assert len(set(r for r in resident if r >= 0)) == len([r for r in resident if r >= 0])
            if window == 3:
                assert (n2 + 1) % nt in resident, (slot, k, t, resident)      # already there before the walk reaches it
            assert uploads == entries, (slot, k, t, uploads, entries)           # one slice per change of interval, never one per step
        prev = (n1, n2)
    assert entries < len(walk)
    for t in (walk[-1] + 5.0, walk[-1] + 5.0 - 7.0, walk[0]):
        n1, n2, _ = tref.plan(times, L.TIME_CYCLICAL, 0.0, t)
        d.update(t)
        d.check(t, (nt, window, "jump", t))
        resident, _ = d.status("TOP_U")
        assert n1 in resident and n2 in resident, (t, (n1, n2), resident)
    d.sources_untouched()


# ---- refusals of the ABI, by name ------------------------------------------------------------------------------------------------------------
def test_abi_refusals():
    Nx, Ny = 37, 29
    d = Driver(Nx, Ny)
    ctx = d.m.ctx
    src = sources(Nx, Ny)["5x4_bounded"]
    rng = np.random.default_rng(4)
    data = rng.standard_normal((2,) + src.shape)
    st = d.series([0.0, 1.0], data, L.TIME_CLAMP)
    fc_map, m = d.map(src, FC)
    rot_map, _ = d.map(src, FC, _rotation(rng, (Ny, Nx + 1)))
    d.bind("TOP_U"); d.bind("TOP_V"); d.bind("SNOWFALL")
    torch.cuda.synchronize()
    set_ = lambda slot, ts, map_id, other=None, component=0: ctx.call(      # noqa: E731
        "csi_time_series_set_regridded", L.F[slot], C.byref(ts) if ts is not None else None, map_id, C.byref(other) if other is not None else None, component)
    for bad_id in (-1, 7, L.REGRID_MAX_MAPS):
        with pytest.raises(csi.CsiError, match="unknown map"):
            set_("TOP_U", st, bad_id)
    with pytest.raises(csi.CsiError, match="wrong location"):
        set_("TOP_V", st, fc_map)
    with pytest.raises(csi.CsiError, match="wrong location"):
        set_("SNOWFALL", st, fc_map)
    with pytest.raises(csi.CsiError, match="component without other"):
        set_("TOP_U", st, fc_map, None, 1)
    with pytest.raises(csi.CsiError, match="component is 0"):
        set_("TOP_U", st, rot_map, st, 2)
    with pytest.raises(csi.CsiError, match="needs a map with cos and sin"):
        set_("TOP_U", st, fc_map, st, 0)
    with pytest.raises(csi.CsiError, match=r"x component of a pair drives a slot at \(Face, Center\)"):
        set_("TOP_U", st, rot_map, st, 1)
    with pytest.raises(csi.CsiError, match="ts must not be NULL"):
        set_("TOP_U", None, fc_map)
    with pytest.raises(csi.CsiError, match="not one a series may drive"):
        set_("H", st, fc_map)
    small = d.series([0.0, 1.0], data[:, :3, :], L.TIME_CLAMP)            # slices smaller than the map's source
    small.slice_stride = 3 * src.shape[1] - 1
    with pytest.raises(csi.CsiError, match="too small for slices of the map's source shape"):
        set_("TOP_U", small, fc_map)
    with pytest.raises(csi.CsiError, match="bind field bottom_u first") as e:
        set_("BOT_U", st, fc_map)
    assert e.value.code == -2
    # maps: an index out of range, a weight outside [0, 1], extents beyond the layout's limit or not the location's, NULL arrays
    i0, i1, j0, j1, wx, wy = (a.copy() for a in m)
    create = lambda *a, shape=src.shape, loc=L.REGRID_FACE_CENTER, **k: ctx.regrid_map_create(loc, *a, shape, **k)      # noqa: E731
    for k, (arr, value) in enumerate(((i0, src.shape[1]), (i1, -1), (j0, src.shape[0]), (j1, 70000))):
        broken = [a.copy() for a in (i0, i1, j0, j1)]
        broken[k][3, 5] = value
        with pytest.raises(csi.CsiError, match=r"index out of range at point \(5, 3\)"):
            create(*broken, wx, wy)
    for k, value in ((0, 1.0 + 1e-15), (1, -1e-300), (0, np.nan)):
        broken = [wx.copy(), wy.copy()]
        broken[k][2, 1] = value
        with pytest.raises(csi.CsiError, match=r"weight outside \[0, 1\] at point \(1, 2\)"):
            create(i0, i1, j0, j1, *broken)
    with pytest.raises(csi.CsiError, match="beyond the layout's limit"):
        create(i0, i1, j0, j1, wx, wy, shape=(4, 65537))
    with pytest.raises(csi.CsiError, match="beyond the layout's limit"):
        create(i0, i1, j0, j1, wx, wy, shape=(1, 5))
    with pytest.raises(csi.CsiError, match="not the interior of a field at that location"):
        create(i0, i1, j0, j1, wx, wy, loc=L.REGRID_CENTER_CENTER)
    with pytest.raises(csi.CsiError, match="unknown location"):
        create(i0, i1, j0, j1, wx, wy, loc=3)
    with pytest.raises(csi.CsiError, match="cos and sin come together"):
        create(i0, i1, j0, j1, wx, wy, cos=np.ones_like(wx))
    with pytest.raises(csi.CsiError, match="cos and sin must be finite"):
        create(i0, i1, j0, j1, wx, wy, cos=np.full_like(wx, np.inf), sin=np.zeros_like(wx))
    assert ctx.regrid_stats() == (0, 2)                                # (no refused map stayed)
    # at least eight maps; destroying: unknown, in use, then free
    more = [create(i0, i1, j0, j1, wx, wy) for _ in range(L.REGRID_MAX_MAPS - 2)]
    assert ctx.regrid_stats()[1] == L.REGRID_MAX_MAPS >= 8
    with pytest.raises(csi.CsiError, match="CSI_REGRID_MAX_MAPS maps are alive"):
        create(i0, i1, j0, j1, wx, wy)
    for mp in more:
        ctx.call("csi_regrid_map_destroy", mp)
    with pytest.raises(csi.CsiError, match="unknown map"):
        ctx.call("csi_regrid_map_destroy", more[0])
    set_("TOP_U", st, fc_map)
    with pytest.raises(csi.CsiError, match="the series of top_u still uses the map"):
        ctx.call("csi_regrid_map_destroy", fc_map)
    ctx.call("csi_time_series_set", L.F["TOP_U"], None)               # csi_time_series_set(NULL) removes a regridded series too
    ctx.call("csi_regrid_map_destroy", fc_map)
    assert ctx.regrid_stats() == (0, 1)
    ctx.time_series_update(0.5)                                        # nothing set: nothing launched
    assert ctx.regrid_stats() == (0, 1)


# ---- models: a run driven by regridded series equals the run whose arrays the test sets from the restatement --------------------------------
TIMES = np.array([-50.0, 200.0, 400.0, 1000.0])                     # three steps of 120 s from t = 0 cross the node at 200


def forcing(seed=7):
    """A wind stress (E, N) on a 64 x 32 periodic source grid and an ocean current on a second, coarser one, in degrees."""
    rng = np.random.default_rng(seed)
    wind = csi.SourceGrid(np.arange(0.0, 360.0, 5.625) - 180.0, np.linspace(-90.0, 90.0, 32), periodic_x=True)
    ocean = csi.SourceGrid(np.arange(0.0, 360.0, 9.0) - 175.0, np.linspace(-88.0, 89.0, 21), periodic_x=True, period=360.0)
    out = {}
    for name, src, scale in (("tau", wind, 0.05), ("ocean", ocean, 0.05)):
        lam, phi = np.deg2rad(src.x)[None, None, :], np.deg2rad(src.y)[None, :, None]
        ph = np.arange(TIMES.size)[:, None, None]
        east = scale * (np.cos(2 * lam + 0.4 * ph) * np.cos(phi) + 0.2 * rng.standard_normal((TIMES.size,) + src.shape))
        north = scale * (np.sin(3 * lam - 0.3 * ph) * np.sin(2 * phi) + 0.2 * rng.standard_normal((TIMES.size,) + src.shape))
        out[name] = (src, east, north)
    return out


def restated(g, data, name, comp, t, indexing):
    """The array a slot holds at time t: component comp of the pair `name` on grid (or tile) g, from the restatement."""
    src, east, north = data[name]
    loc = (FC, CF)[comp]
    m = ref.plan_points(src.x, src.y, src.periodic_x, src.period, *g.target_nodes(*loc))
    return ref.pair_at(TIMES, east, north, indexing.kind, indexing.period, t, m, *g.rotation(*loc), comp)


def regrid_hook(data, series, indexing, backend=None, t0=0.0):
    def make(g, k):
        if series:
            v = {n: csi.RegriddedVectorTimeSeries(g, src, TIMES, e, nn, time_indexing=indexing, backend=backend) for n, (src, e, nn) in data.items()}
            k["top_momentum_stress"] = (v["tau"].x, v["tau"].y)
            k["bottom_momentum_stress"] = csi.SemiImplicitStress(ue=v["ocean"].x, ve=v["ocean"].y)
        else:
            k["top_momentum_stress"] = (restated(g, data, "tau", 0, t0, indexing), restated(g, data, "tau", 1, t0, indexing))
            k["bottom_momentum_stress"] = csi.SemiImplicitStress(ue=restated(g, data, "ocean", 0, t0, indexing), ve=restated(g, data, "ocean", 1, t0, indexing))
    return make


def write_arrays(m, data, t, indexing):
    m.synchronize()
    for slot, name in (("TOP", "tau"), ("BOT", "ocean")):
        for comp, c in enumerate("UV"):
            m.external_stress_field(slot, c).set(restated(m.grid, data, name, comp, t, indexing))


STATE = ("u", "v", "h", "a")
KW = dict(mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7))


def _pair_of_models(c, data, indexing, backend=None, **kw):
    with dynamics_hook(regrid_hook(data, True, indexing, backend)):
        A = cases.csi_model(c, **dict(KW, **kw))
    with dynamics_hook(regrid_hook(data, False, indexing)):
        B = cases.csi_model(c, **dict(KW, **kw))
    assert sorted(A._series) == ["BOT_U", "BOT_V", "TOP_U", "TOP_V"] and not B._series
    assert A.ctx.regrid_stats()[1] == 4 and B.ctx.regrid_stats() == (0, 0)      # one map per (source, location)
    return A, B


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("grid", ["latlon", "tripolar"])
def test_run_driven_by_regridded_pairs_equals_hand_updated_run(grid, mode):
    """RK3, WENO7, the EVP pair kernel: a wind-stress pair and an ocean-velocity pair on two source grids (model A) against the same
    model with plain arrays that the test rewrites from the restatement before every step (model B), bit for bit after each of three
    steps.  latlon: 64 x 48, the rotation is (1, 0).  tripolar: TripolarGrid((32, 24), halo = (4, 4)) -- the rotation in the cap, the fold
    band."""
    if grid == "latlon":
        c = cases.make_case(Nx=64, Ny=48, grid="latlon", topo=("periodic", "bounded"), substeps=12, random_uv=0.05, land=0.15)
    else:
        c = cases.make_case(Nx=32, Ny=24, grid="tripolar", substeps=12, random_uv=0.05, coriolis_points=True)
    data = forcing()
    ind = csi.Linear()
    A, B = _pair_of_models(c, data, ind, backend=csi.InMemory(3) if mode == "fast" else None, mode=mode)
    base, updates, update = A.ctx.regrid_stats()[0], [], A.ctx.time_series_update
    A.ctx.time_series_update = lambda t: (updates.append(t), update(t))[1]
    crossed = set()
    for n in range(3):
        crossed.add(tref.plan(TIMES, L.TIME_LINEAR, 0.0, A.clock.time)[:2])
        write_arrays(B, data, B.clock.time, ind)
        csi.time_step(A, c["dt"])
        csi.time_step(B, c["dt"])
        assert_same(state_of(A, STATE), state_of(B, STATE), (grid, mode, "step", n))
        assert A.ctx.last_path() == B.ctx.last_path() and A.ctx.last_launches() == B.ctx.last_launches()
        assert A.ctx.last_path()["level"] == (2 if mode == "fast" else 0), A.ctx.last_path()      # (the pair kernel is the FAST path's)
        assert len(updates) >= n + 1 and A.ctx.regrid_stats()[0] == base + len(updates)      # four slots, ONE launch per update
    assert len(crossed) >= 2                                        # the steps crossed a slice boundary
    for slot in ("TOP", "BOT"):                                     # the driven arrays themselves, halos included
        for comp in "UV":
            assert np.array_equal(A.external_stress_field(slot, comp).numpy(), B.external_stress_field(slot, comp).numpy()), (slot, comp)
    if grid == "tripolar":
        s = A.grid.rotation(*FC)[1]
        assert np.abs(s).max() > 0.5                                # (the cap does rotate)


def test_slab_thermodynamics_with_a_regridded_heat_flux_and_shortwave_flux():
    Nx, Ny, DT = 48, 32, 600.0
    g = csi.LatitudeLongitudeGrid((Nx, Ny), longitude=(0, 60), latitude=(60, 85), topology=(csi.Periodic, csi.Bounded), halo=(4, 4))
    src = csi.SourceGrid(np.arange(-10.0, 75.0, 5.0), np.linspace(55.0, 90.0, 9))
    rng = np.random.default_rng(9)
    times = np.array([0.0, 900.0, 1500.0, 4000.0])
    q = 250.0 + 60.0 * rng.standard_normal((4,) + src.shape)
    sw = -120.0 * rng.random((4,) + src.shape)
    h0, a0 = 0.5 + rng.random((Ny, Nx)), 0.3 + 0.7 * rng.random((Ny, Nx))
    h0[:4, :6] = 0.0; a0[:4, :6] = 0.0
    m_cc = ref.plan_points(src.x, src.y, False, 0.0, *g.target_nodes(*CC))
    at = lambda data, kind, t: ref.at(times, data, kind, 0.0, t, m_cc)      # noqa: E731
    models = []
    for series in (True, False):
        top = csi.RegriddedTimeSeries(g, CC, src, times, q, time_indexing=csi.Clamp(), backend=csi.InMemory(2)) if series else at(q, L.TIME_CLAMP, 0.0)
        flux = csi.RegriddedTimeSeries(g, CC, src, times, sw, time_indexing=csi.Linear()) if series else at(sw, L.TIME_LINEAR, 0.0)
        ice = csi.SlabThermodynamics(bottom_salinity=30.0, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        m = csi.SeaIceModel(g, ice_thermodynamics=ice, top_heat_flux=(csi.RadiativeEmission(), csi.ShortwaveRadiation(flux), top, -20.0),
                            bottom_heat_flux=4.0, timestepper="ForwardEuler", mode="strict")
        csi.set_(m, h=h0, aice=a0)
        models.append(m)
    A, B = models
    assert sorted(A._series) == ["SHORTWAVE", "TOP_HEAT_FLUX"] and A.ctx.regrid_stats()[1] == 1            # one source, one location: one map
    names = dict(h=lambda m: m.ice_thickness, a=lambda m: m.ice_concentration, Tu=lambda m: m.ice_top_temperature,
                 q=lambda m: m.external_heat_fluxes.top, sw=lambda m: m.shortwave_flux)
    for n in range(4):
        t = B.clock.time
        B.synchronize()
        B.external_heat_fluxes.top.set(at(q, L.TIME_CLAMP, t))
        B.shortwave_flux.set(at(sw, L.TIME_LINEAR, t))
        csi.time_step(A, DT); csi.time_step(B, DT)
        A.synchronize(); B.synchronize()
        for k, f in names.items():
            x, y = f(A).interior_numpy(), f(B).interior_numpy()
            assert np.array_equal(x, y), (n, k, np.abs(x - y).max())
    assert np.abs(A.ice_thickness.interior_numpy() - h0).max() > 1e-4


def _tile_run(m, c):
    res = {}
    m.clock.time = 100.0
    csi.time_step_momentum(m, c["dt"])
    m.synchronize()
    res.update({f"mom_{f}": EVP_FIELDS[f](m).interior_numpy().copy() for f in ("u", "v")})
    m.clock.time = 330.0
    csi.time_step(m, c["dt"])
    m.synchronize()
    res.update({f"step_{f}": EVP_FIELDS[f](m).interior_numpy().copy() for f in STATE})
    return res


def test_tiled_1x2_run_equals_untiled():
    """Every rank holds the whole source and builds the map of ITS tile; a 1 x 2 tiling in one process against the untiled run."""
    c = cases.make_case(Nx=64, Ny=48, H=8, grid="latlon", topo=("periodic", "bounded"), substeps=14, random_uv=0.05)
    data = forcing()
    with dynamics_hook(regrid_hook(data, True, csi.Cyclical(1200.0), csi.InMemory(2))):
        whole = _tile_run(cases.csi_model(c, **KW), c)

        def tile(rank, group):
            m = cases.csi_model(c, tile=(1, 2, rank), local_group=group, **KW)
            assert len(m._series) == 4 and m.ctx.regrid_stats()[1] == 4
            m.set_exchange_interval(0)
            res = _tile_run(m, c)
            res["offsets"] = (m.grid.i_off, m.grid.j_off, m.grid.Nx, m.grid.Ny)
            del m
            return res
        tiles = run_tile_threads(2, tile)
    for rank, d in enumerate(tiles):
        i0, j0, nx, ny = d["offsets"]
        for k, want in whole.items():
            got, w = d[k][:ny, :nx], want[j0:j0 + ny, i0:i0 + nx]
            assert np.array_equal(got, w), (rank, k, np.abs(got - w).max())


def test_a_model_without_regridded_series_never_launches_the_kernel():
    c = cases.make_case(Nx=48, Ny=32, substeps=8, wind_drag="arrays", field_forcing=True)
    m = cases.csi_model(c, **KW)
    csi.time_step(m, c["dt"])
    m.ctx.time_series_update(12.0)
    m.synchronize()
    assert m.ctx.regrid_stats() == (0, 0) and not m._regrid_maps
    # ... nor does one whose series all live on the model grid
    g = c["g"]
    fts = csi.FieldTimeSeries(g, CC, [0.0, 1.0], np.zeros((2, 32, 48)))
    m2 = csi.SeaIceModel(g, ice_thermodynamics=csi.SlabThermodynamics(), top_heat_flux=fts, timestepper="ForwardEuler")
    csi.time_step(m2, 10.0)
    m2.synchronize()
    assert sorted(m2._series) == ["TOP_HEAT_FLUX"] and m2.ctx.regrid_stats() == (0, 0)
