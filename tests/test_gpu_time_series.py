"""Forcing time series interpolated at the model clock on the device (include/csi.h: csi_time_series_set / _update / _status;
csrc/time_series.hip, csrc/csi_time_series.hip; csi.FieldTimeSeries).  The oracle is the NumPy restatement tests/time_series_ref.py;
EVERY comparison is bit for bit: the interpolation is two products and one sum in a stated order, and a series-driven array is, to
the kernels that read it, an array."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import time_series_ref as ref
from test_gpu_evp import EVP_FIELDS
from test_gpu_local_tiles import check as check_tiles, run_tile_threads

pytestmark = pytest.mark.gpu
L = csi._lib
KIND = {"clamp": (L.TIME_CLAMP, csi.Clamp), "cyclical": (L.TIME_CYCLICAL, csi.Cyclical), "linear": (L.TIME_LINEAR, csi.Linear)}
LOC = {"fc": (csi.Face, csi.Center), "cf": (csi.Center, csi.Face), "cc": (csi.Center, csi.Center)}
SLOT_LOC = dict(TOP_U="fc", TOP_V="cf", BOT_U="fc", BOT_V="cf", FORCING_U="fc", FORCING_V="cf", FREE_DRIFT_U="fc", FREE_DRIFT_V="cf",
                TOP_HEAT_FLUX="cc", BOTTOM_HEAT_FLUX="cc", SNOWFALL="cc")
NONUNIFORM = np.array([3.0, 10.0, 11.0, 40.0, 41.5])


# ---- the ABI driven directly: a bare context (a model without dynamics), fields bound by hand ------------------------------------------
class Driver:
    def __init__(self, Nx=48, Ny=32, topo=(csi.Bounded, csi.Periodic), mode="fast"):
        self.g = csi.RectilinearGrid((Nx, Ny), x=(0.0, Nx * 1e3), y=(0.0, Ny * 1e3), topology=topo, halo=(4, 4))
        self.m = csi.SeaIceModel(self.g, dynamics=None, advection=None, timestepper="ForwardEuler", mode=mode)
        self.fields, self.keep, self.spec = {}, [], {}

    def add(self, slot, times, data, kind, period=0.0, backend="device", window=3, pad=0):
        """Bind a field to `slot` and set a series on it.  pad: extra doubles per row (and `pad` extra rows per slice) of the series'
        own layout, so that ld / slice_stride differ from the packed ones."""
        fld = csi.Field(LOC[SLOT_LOC[slot]], self.g, self.m.device, slot.lower())
        fld.fill_parent(-777.0)                                       # the halo must stay untouched
        self.m._bind(slot, fld)
        nt, ny, nx = data.shape
        lay = np.full((nt, ny + pad, nx + pad), np.nan)
        lay[:, :ny, :nx] = data
        times = np.ascontiguousarray(times, dtype=np.float64)
        if backend == "device":
            held = torch.from_numpy(lay).to(self.m.device)
            ptr = held.data_ptr()
        else:
            held = lay
            ptr = lay.ctypes.data
        st = L.TimeSeries(nt, kind, L.SERIES_DEVICE if backend == "device" else L.SERIES_HOST, window, period,
                          times.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(ptr), nx + pad, (ny + pad) * (nx + pad))
        torch.cuda.synchronize()
        self.m.ctx.call("csi_time_series_set", L.F[slot], C.byref(st))
        self.keep += [held, times, st]
        self.fields[slot] = fld
        self.spec[slot] = (times, data, kind, period, window if backend == "host" else 0)
        return fld

    def update(self, t):
        self.m.ctx.time_series_update(t)
        self.m.synchronize()

    def check(self, t, what=()):
        for slot, (times, data, kind, period, _) in self.spec.items():
            want = ref.at(times, data, kind, period, t)
            got = self.fields[slot].interior_numpy()
            assert got.shape == want.shape, (slot, got.shape, want.shape)
            assert np.array_equal(got, want), (what, slot, t, ref.plan(times, kind, period, t), np.abs(got - want).max(),
                                               np.argwhere(got != want)[:4].tolist())

    def status(self, slot):
        return self.m.ctx.time_series_status(slot, self.spec[slot][4])


def _data(rng, nt, g, loc):
    nx, ny = g.interior_size(*LOC[loc])
    return rng.standard_normal((nt, ny, nx)) * 10.0 ** rng.integers(-3, 3, size=(nt, 1, 1))


def _probe(times, period):
    span, step = times[-1] - times[0], times[-1] - times[-2]
    t = list(times) + [0.5 * (a + b) for a, b in zip(times[:-1], times[1:])] + [times[0] + 0.37 * step, times[1] - 1e-9]
    t += [times[0] - 0.25 * step, times[0] - 2.6 * span, times[-1] + 0.25 * step, times[-1] + 0.6 * step, times[-1] + 1.3 * span]
    t += [times[-1] + 0.5 * (period - span), times[0] + period, times[2] + 2 * period, times[0] - 0.3 * period]
    return [float(x) for x in t]


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("kind", ["clamp", "cyclical", "linear"])
@pytest.mark.parametrize("backend", ["device", "host"])
def test_interpolation_equals_the_restatement(backend, kind, mode):
    """One slot of each location on a Bounded x Periodic grid: the (Face, Center) field is one column wider, its rows (and the packed
    rows of the series) are an odd number of doubles long, so aligned and unaligned rows, lone first / last points and 16-byte pairs
    all occur.  About twenty times: every node, between nodes, before and after the ends, the cyclical gap and whole periods later."""
    d = Driver(mode=mode)
    rng = np.random.default_rng(11)
    period = 45.0 if kind == "cyclical" else 0.0
    for slot, pad in (("TOP_U", 0), ("TOP_V", 0), ("SNOWFALL", 3)):
        d.add(slot, NONUNIFORM, _data(rng, NONUNIFORM.size, d.g, SLOT_LOC[slot]), KIND[kind][0], period, backend, window=3, pad=pad)
    assert d.fields["TOP_U"].interior_numpy().shape == (32, 49)
    times = _probe(NONUNIFORM, period or ref.inferred_period(NONUNIFORM))
    assert len(times) >= 20
    for t in times:
        d.update(t)
        d.check(t, (backend, kind, mode))
    for slot, fld in d.fields.items():                            # nothing but the interior was written
        full = fld.numpy().copy()
        ny, nx = fld.interior_numpy().shape
        full[4:4 + ny, 4:4 + nx] = -777.0
        assert np.all(full == -777.0), slot


@pytest.mark.parametrize("backend", ["device", "host"])
def test_all_eleven_slots_in_one_launch(backend):
    """Every eligible slot driven at once, each with its own number of slices, times, indexing kind and (so) weight."""
    d = Driver(Nx=64, Ny=48, topo=(csi.Bounded, csi.Bounded))
    rng = np.random.default_rng(5)
    kinds = [L.TIME_LINEAR, L.TIME_CYCLICAL, L.TIME_CLAMP]
    for k, slot in enumerate(L.SERIES_SLOTS):
        nt = 2 + k % 5
        times = np.cumsum(0.5 + rng.random(nt)) * (1.0 + k) - 3.0
        d.add(slot, times, _data(rng, nt, d.g, SLOT_LOC[slot]), kinds[k % 3], 0.0, backend, window=2 + k % 2, pad=k % 2)
    for t in (-5.0, 0.0, 1.234, 7.5, 19.0, 64.0):
        d.update(t)
        d.check(t, backend)
    weights = {ref.plan(*d.spec[s][:1], d.spec[s][2], d.spec[s][3], 7.5)[2] for s in d.spec}
    assert len(weights) >= 6                                      # (genuinely different descriptors)


def test_slots_that_no_series_can_drive_are_refused_by_name():
    d = Driver()
    st = L.TimeSeries()
    for slot in ("U", "H", "S11", "GH", "MASS_FLUX", "TU"):
        with pytest.raises(csi.CsiError, match="not one a series may drive") as e:
            d.m.ctx.call("csi_time_series_set", L.F[slot], C.byref(st))
        assert e.value.code == -1
    with pytest.raises(csi.CsiError, match="bind field snowfall first") as e:
        d.m.ctx.call("csi_time_series_set", L.F["SNOWFALL"], C.byref(st))
    assert e.value.code == -2
    fld = d.add("SNOWFALL", [0.0, 1.0], np.zeros((2, 32, 48)), L.TIME_CLAMP)
    bad = L.TimeSeries(2, L.TIME_CYCLICAL, L.SERIES_DEVICE, 0, 0.5, d.keep[1].ctypes.data_as(C.POINTER(C.c_double)),
                       C.c_void_p(d.keep[0].data_ptr()), 48, 48 * 32)
    with pytest.raises(csi.CsiError, match="period longer"):
        d.m.ctx.call("csi_time_series_set", L.F["SNOWFALL"], C.byref(bad))
    d.m.ctx.call("csi_time_series_set", L.F["SNOWFALL"], None)       # NULL removes
    with pytest.raises(csi.CsiError, match="no series"):
        d.m.ctx.time_series_status("SNOWFALL", 0)
    d.m.ctx.time_series_update(0.5)                                  # nothing set: nothing launched, CSI_OK
    assert fld is not None


# ---- the device window of a host-resident series ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,window", [(10, 3), (9, 2)], ids=["nt10_window3", "nt9_window2"])
def test_window_residency_and_upload_counts(nt, window):
    """nt = 10, window = 3: slice mod window would put the cyclical wrap pair (9, 0) into one slot.  nt = 9, window = 2: no room to
    look ahead.  A walk of 40 times through two and a half periods, then jumps forward by five slices, backward by seven and back to
    the first time."""
    d = Driver()
    rng = np.random.default_rng(nt)
    times = np.arange(nt) * 1.0
    period = float(nt)                                              # (what Cyclical infers)
    d.add("TOP_U", times, _data(rng, nt, d.g, "fc"), L.TIME_CYCLICAL, 0.0, "host", window=window)
    assert d.status("TOP_U") == ([-1] * window, 0)
    walk = [0.3 + k * (2.5 * period / 40.0) for k in range(40)]
    entries, prev = 0, None
    for k, t in enumerate(walk):
        n1, n2, _ = ref.plan(times, L.TIME_CYCLICAL, 0.0, t)
        assert n1 != n2
        d.update(t)
        d.check(t, (nt, window, k))
        resident, uploads = d.status("TOP_U")
        assert n1 in resident and n2 in resident, (k, t, (n1, n2), resident)
        assert len(set(r for r in resident if r >= 0)) == len([r for r in resident if r >= 0])
        nxt = (n2 + 1) % nt
        if window == 3:
            assert nxt in resident, (k, t, nxt, resident)           # already there before the walk reaches it
        # slices entering the window: the first call brings its pair (and, with room, the next slice); every later change of
        # interval brings exactly one slice -- never one per step
        if prev is None:
            entries = 3 if window == 3 else 2
        elif (n1, n2) != prev:
            assert n1 == prev[1]                                    # (the walk skips no interval)
            entries += 1
        assert uploads == entries, (k, t, uploads, entries)
        prev = (n1, n2)
    assert entries < len(walk)
    first = walk[0]
    for t in (walk[-1] + 5.0, walk[-1] + 5.0 - 7.0, first):
        n1, n2, _ = ref.plan(times, L.TIME_CYCLICAL, 0.0, t)
        d.update(t)
        d.check(t, (nt, window, "jump", t))
        resident, _ = d.status("TOP_U")
        assert n1 in resident and n2 in resident, (t, (n1, n2), resident)


def test_window_at_nodes_and_with_clamped_ends():
    """n1 == n2 (a node, a clamped end): one slice suffices, the look-ahead still runs; beyond a clamped end there is nothing to fetch."""
    d = Driver()
    rng = np.random.default_rng(3)
    times = np.array([0.0, 2.0, 3.0, 7.0, 8.0, 12.0])
    d.add("SNOWFALL", times, _data(rng, 6, d.g, "cc"), L.TIME_CLAMP, 0.0, "host", window=2)
    for t, want_resident in ((-1.0, {0, 1}), (2.0, {1, 2}), (2.5, {1, 2}), (7.0, {3, 4}), (12.0, {5}), (50.0, {5}), (0.5, {0, 1})):
        d.update(t)
        d.check(t, t)
        resident, _ = d.status("SNOWFALL")
        assert want_resident <= set(resident), (t, resident)


# ---- models: a series-driven run equals the run whose arrays the test updates by hand ----------------------------------------------------
TIMES = np.array([-50.0, 250.0, 400.0, 1000.0])                     # steps of 120 s from t = 0 cross the node at 250


def forcing_data(g, seed=7):
    """Global-grid series for the six velocity-point arrays of an OMIP-style case: air velocities (wind drag), ocean velocities
    (bottom drag) and prescribed free-drift velocities."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, loc, scale in (("ua", "fc", 6.0), ("va", "cf", 4.0), ("uo", "fc", 0.05), ("vo", "cf", 0.05), ("fdu", "fc", 0.03), ("fdv", "cf", 0.03),
                             ("tu", "fc", 0.02), ("tv", "cf", 0.02)):
        nx, ny = g.interior_size(*LOC[loc])
        x, y = np.linspace(0, 1, nx)[None, None, :], np.linspace(0, 1, ny)[None, :, None]
        phase = np.arange(TIMES.size)[:, None, None]
        out[name] = (loc, scale * (np.cos(2 * np.pi * (y + 0.1 * phase)) * np.sin(2 * np.pi * (x - 0.07 * phase)) + 0.2 * rng.standard_normal((TIMES.size, ny, nx))))
    return out


def _local(g, arr, loc):
    return g.local_interior(arr, *LOC[loc]) if isinstance(g, csi.TileGrid) else arr


def forcing_values(g, data, series, t0=0.0, indexing=None, backend=None):
    """name -> what the model is given: a FieldTimeSeries on g (global data, cut per tile) or the restatement's array at t0."""
    indexing = indexing or csi.Linear()
    if series:
        return {k: csi.FieldTimeSeries(g, LOC[loc], TIMES, a, time_indexing=indexing, backend=backend or csi.InMemory()) for k, (loc, a) in data.items()}
    return {k: _local(g, ref.at(TIMES, a, indexing.kind, indexing.period, t0), loc) for k, (loc, a) in data.items()}


@contextmanager
def dynamics_hook(make):
    """cases.csi_model builds its dynamics with csi.SeaIceMomentumEquation(g, ...): make(g, keywords) replaces keywords (stresses,
    free_drift, rheology, solver) or returns another dynamics object."""
    orig = csi.SeaIceMomentumEquation

    def dynamics(g, **k):
        got = make(g, k)
        return got if got is not None else orig(g, **k)
    csi.SeaIceMomentumEquation = dynamics
    try:
        yield
    finally:
        csi.SeaIceMomentumEquation = orig


# The pair kernel has instantiations for stress arrays + ocean velocities + free-drift fields and for wind drag + ocean velocities,
# none for wind drag together with free-drift fields (three kernels then): all three are run.
CONFIGS = {"stress_ocean_freedrift": (("tu", "tv"), True, 2), "wind_ocean": (("ua", "va"), False, 2), "wind_ocean_freedrift": (("ua", "va"), True, 0)}


def omip_hook(data, series, holder, config="stress_ocean_freedrift", **kw):
    (top_u, top_v), free_drift, _ = CONFIGS[config]
    used = {k: data[k] for k in (top_u, top_v, "uo", "vo") + (("fdu", "fdv") if free_drift else ())}

    def make(g, k):
        v = forcing_values(g, used, series, **kw)
        holder.append(v)
        k["top_momentum_stress"] = (v["tu"], v["tv"]) if top_u == "tu" else csi.SemiImplicitStress(ue=v["ua"], ve=v["va"], rho_e=1.3, Cd=1.2e-3)
        k["bottom_momentum_stress"] = csi.SemiImplicitStress(ue=v["uo"], ve=v["vo"])
        if free_drift:
            k["free_drift"] = dict(u=v["fdu"], v=v["fdv"])
    return make


def write_omip_arrays(m, data, t, config="stress_ocean_freedrift", indexing=None):
    (top_u, top_v), free_drift, _ = CONFIGS[config]
    indexing = indexing or csi.Linear()
    at = lambda k: _local(m.grid, ref.at(TIMES, data[k][1], indexing.kind, indexing.period, t), data[k][0])
    m.synchronize()
    m.external_stress_field("TOP", "U").set(at(top_u)); m.external_stress_field("TOP", "V").set(at(top_v))
    m.external_stress_field("BOT", "U").set(at("uo")); m.external_stress_field("BOT", "V").set(at("vo"))
    if free_drift:
        m.free_drift_field("u").set(at("fdu")); m.free_drift_field("v").set(at("fdv"))


def state_of(m, names):
    m.synchronize()
    return {k: EVP_FIELDS[k](m).numpy().copy() for k in names}


STATE = ("u", "v", "s11", "s22", "s12", "h", "a")
EVP_FIELDS = dict(EVP_FIELDS, h=lambda m: m.ice_thickness, a=lambda m: m.ice_concentration)


def assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, np.abs(a[k] - b[k]).max(), np.argwhere(a[k] != b[k])[:4].tolist())


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("backend", ["device", "host"])
def test_series_driven_evp_run_equals_hand_updated_run(backend, config):
    """RK3, WENO7, the EVP pair kernel at fusion level 2: wind-drag arrays, ocean-velocity arrays and prescribed free-drift fields
    driven by six series (model A) against the same model with plain arrays that the test rewrites before every step (model B)."""
    c = cases.make_case(Nx=64, Ny=48, topo=("periodic", "bounded"), substeps=12, random_uv=0.05, land=0.15)
    data = forcing_data(c["g"])
    kw = dict(mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7))
    held = []
    with dynamics_hook(omip_hook(data, True, held, config, backend=csi.InMemory() if backend == "device" else csi.InMemory(3))):
        A = cases.csi_model(c, **kw)
    with dynamics_hook(omip_hook(data, False, held, config)):
        B = cases.csi_model(c, **kw)
    fd = CONFIGS[config][1]
    assert sorted(A._series) == ["BOT_U", "BOT_V"] + (["FREE_DRIFT_U", "FREE_DRIFT_V"] if fd else []) + ["TOP_U", "TOP_V"] and not B._series
    crossed = set()
    for n in range(5):
        crossed.add(ref.plan(TIMES, L.TIME_LINEAR, 0.0, A.clock.time)[:2])
        write_omip_arrays(B, data, B.clock.time, config)
        csi.time_step(A, c["dt"])
        csi.time_step(B, c["dt"])
        assert_same(state_of(A, STATE), state_of(B, STATE), (backend, "step", n))
        assert A.ctx.last_path() == B.ctx.last_path() and A.ctx.last_launches() == B.ctx.last_launches()
        assert A.ctx.last_path()["level"] == CONFIGS[config][2], A.ctx.last_path()
    assert len(crossed) >= 2                                        # the steps crossed a slice boundary
    assert A.clock.time == B.clock.time == 5 * c["dt"]
    # the entries that are called on their own read the clock too
    A.clock.time = B.clock.time = 777.0
    write_omip_arrays(B, data, 777.0, config)
    for step in (lambda m: csi.time_step_momentum(m, c["dt"]), csi.update_state):
        step(A); step(B)
    assert_same(state_of(A, STATE), state_of(B, STATE), (backend, "momentum step on its own"))
    for slot in ("TOP", "BOT"):                                     # halos included
        assert np.array_equal(A.external_stress_field(slot, "U").numpy(), B.external_stress_field(slot, "U").numpy())


@pytest.mark.parametrize("variant", ["viscous", "explicit"])
def test_model_forcing_series_on_the_viscous_and_explicit_paths(variant):
    c = cases.make_case(Nx=48, Ny=32, topo=("bounded", "periodic"), substeps=8, random_uv=0.05)
    g = c["g"]
    rng = np.random.default_rng(2)
    data = {"fu": ("fc", 3e-6 * rng.standard_normal((TIMES.size,) + tuple(reversed(g.interior_size(*LOC["fc"]))))),
            "fv": ("cf", 3e-6 * rng.standard_normal((TIMES.size,) + tuple(reversed(g.interior_size(*LOC["cf"])))))}
    extra = dict(rheology=csi.ViscousRheology(nu=500.0)) if variant == "viscous" else dict(solver=csi.ExplicitSolver())

    def make(g_, k):
        k.update(extra)
    ind = csi.Cyclical()
    models = []
    for series in (True, False):
        v = forcing_values(g, data, series, indexing=ind, backend=csi.InMemory(2))
        with dynamics_hook(make):
            models.append(cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), forcing=dict(u=v["fu"], v=v["fv"])))
    A, B = models
    assert sorted(A._series) == ["FORCING_U", "FORCING_V"]
    for n in range(5):
        t = B.clock.time
        B.synchronize()
        B.forcing_fields.u.set(ref.at(TIMES, data["fu"][1], ind.kind, ind.period, t)); B.forcing_fields.v.set(ref.at(TIMES, data["fv"][1], ind.kind, ind.period, t))
        csi.time_step(A, c["dt"]); csi.time_step(B, c["dt"])
        assert_same(state_of(A, ("u", "v", "h", "a")), state_of(B, ("u", "v", "h", "a")), (variant, n))
        assert A.ctx.last_launches() == B.ctx.last_launches()
    if variant == "explicit":                                       # compute_momentum_tendencies on its own reads the clock too
        A.clock.time = B.clock.time = 333.0
        B.synchronize()
        B.forcing_fields.u.set(ref.at(TIMES, data["fu"][1], ind.kind, ind.period, 333.0)); B.forcing_fields.v.set(ref.at(TIMES, data["fv"][1], ind.kind, ind.period, 333.0))
        for m in (A, B):
            csi.compute_momentum_tendencies(m, c["dt"])
            m.synchronize()
        assert np.array_equal(A.timestepper.Gn.u.interior_numpy(), B.timestepper.Gn.u.interior_numpy())


def test_stress_series_under_free_drift_dynamics():
    """dynamics = StressBalanceFreeDrift(top = a pair of stress-array series, bottom = SemiImplicitStress(ocean-velocity series))."""
    c = cases.make_case(Nx=48, Ny=32, topo=("periodic", "bounded"), random_uv=0.05)
    data = forcing_data(c["g"])
    data = {"ua": (data["ua"][0], 0.02 * data["ua"][1]), "va": (data["va"][0], 0.02 * data["va"][1]), "uo": data["uo"], "vo": data["vo"]}
    models = []
    for series in (True, False):
        def make(g, k, series=series):
            v = forcing_values(g, data, series, indexing=csi.Clamp())
            return csi.StressBalanceFreeDrift(top_momentum_stress=(v["ua"], v["va"]), bottom_momentum_stress=csi.SemiImplicitStress(ue=v["uo"], ve=v["vo"]))
        with dynamics_hook(make):
            models.append(cases.csi_model(c, mode="strict", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7)))
    A, B = models
    assert sorted(A._series) == ["BOT_U", "BOT_V", "TOP_U", "TOP_V"]
    for n in range(5):
        at = lambda k: ref.at(TIMES, data[k][1], L.TIME_CLAMP, 0.0, B.clock.time)
        B.synchronize()
        B.external_stress_field("TOP", "U").set(at("ua")); B.external_stress_field("TOP", "V").set(at("va"))
        B.external_stress_field("BOT", "U").set(at("uo")); B.external_stress_field("BOT", "V").set(at("vo"))
        csi.time_step(A, c["dt"]); csi.time_step(B, c["dt"])
        assert_same(state_of(A, ("u", "v", "h", "a")), state_of(B, ("u", "v", "h", "a")), n)
        assert A.ctx.last_launches() == B.ctx.last_launches() == (1, 1)


@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_heat_flux_and_snowfall_series_in_the_thermodynamics(snow):
    """A top heat-flux series beside RadiativeEmission (the secant solve reads the interpolated array) and, on the layered step, a
    snowfall series: h, hs, aice, Tu and the mass fluxes equal those of the hand-updated run."""
    Nx, Ny, DT = 48, 32, 600.0
    g = csi.RectilinearGrid((Nx, Ny), x=(0.0, 48e3), y=(0.0, 32e3), topology=(csi.Periodic, csi.Bounded), halo=(4, 4))
    rng = np.random.default_rng(9)
    times = np.array([0.0, 900.0, 1500.0, 4000.0])
    q = 250.0 + 60.0 * rng.standard_normal((4, Ny, Nx))
    sf = 3e-5 * (1.0 + rng.random((4, Ny, Nx)))
    h0, a0 = 0.5 + rng.random((Ny, Nx)), 0.3 + 0.7 * rng.random((Ny, Nx))
    h0[:4, :6] = 0.0; a0[:4, :6] = 0.0
    h0[8:10, :] = 0.02                                              # unconsolidated cells
    models = []
    for series in (True, False):
        top = csi.FieldTimeSeries(g, (csi.Center, csi.Center), times, q, time_indexing=csi.Clamp(), backend=csi.InMemory(2)) if series else q[0].copy()
        fall = csi.FieldTimeSeries(g, (csi.Center, csi.Center, None), times, sf, time_indexing=csi.Linear()) if series else sf[0].copy()
        ice = csi.SlabThermodynamics(bottom_salinity=30.0, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        kw = dict(ice_thermodynamics=ice, top_heat_flux=(csi.RadiativeEmission(), top, -20.0), bottom_heat_flux=4.0, timestepper="ForwardEuler", mode="strict")
        if snow:
            kw.update(snow_thermodynamics=csi.snow_slab_thermodynamics(), snowfall=fall)
        m = csi.SeaIceModel(g, **kw)
        csi.set_(m, h=h0, aice=a0, **(dict(hs=0.1 * a0) if snow else {}))
        models.append(m)
    A, B = models
    assert sorted(A._series) == (["SNOWFALL", "TOP_HEAT_FLUX"] if snow else ["TOP_HEAT_FLUX"])
    names = dict(h=lambda m: m.ice_thickness, a=lambda m: m.ice_concentration, Tu=lambda m: m.ice_top_temperature)
    if snow:
        names.update(hs=lambda m: m.snow_thickness, Tus=lambda m: m.snow_top_temperature, mf_ice=lambda m: m.mass_fluxes.thermodynamics.ice,
                     mf_snow=lambda m: m.mass_fluxes.thermodynamics.snow, mf_int=lambda m: m.mass_fluxes.intercepted_snowfall)
    for n in range(5):
        t = B.clock.time
        B.synchronize()
        B.external_heat_fluxes.top.set(ref.at(times, q, L.TIME_CLAMP, 0.0, t))
        if snow:
            B.snowfall.set(ref.at(times, sf, L.TIME_LINEAR, 0.0, t))
        csi.time_step(A, DT); csi.time_step(B, DT)
        A.synchronize(); B.synchronize()
        for k, f in names.items():
            x, y = f(A).interior_numpy(), f(B).interior_numpy()
            assert np.array_equal(x, y), (snow, n, k, np.abs(x - y).max())
    assert np.abs(A.ice_thickness.interior_numpy() - h0).max() > 1e-4


# ---- tiles and the north fold -------------------------------------------------------------------------------------------------------------
# (three rows of tests/test_gpu_local_tiles.py's table, as data)
DECOMPOSITIONS = {
    "2x2_channel_land_arrays": (2, 2, dict(Nx=256, Ny=192, topo=("periodic", "bounded"), land=0.2)),
    "2x1_bounded_x": (2, 1, dict(Nx=256, Ny=96, topo=("bounded", "periodic"))),
    "1x2_fold": (1, 2, dict(Nx=192, Ny=192, topo=("periodic", "folded"))),
}


def _tile_run(m, c):
    res = {}
    m.clock.time = 100.0
    csi.time_step_momentum(m, c["dt"])
    csi.time_step_momentum(m, c["dt"])
    m.synchronize()
    res.update({f"mom_{f}": EVP_FIELDS[f](m).interior_numpy().copy() for f in ("u", "v", "s11", "s22", "s12")})
    m.clock.time = 330.0
    csi.time_step(m, c["dt"])
    m.synchronize()
    res.update({f"step_{f}": EVP_FIELDS[f](m).interior_numpy().copy() for f in ("u", "v", "h", "a")})
    res["transport"] = m.ctx.halo_transport() if isinstance(m.grid, csi.TileGrid) else None
    return res


@pytest.mark.parametrize("transport", ["peer", "rccl"])
@pytest.mark.parametrize("name", sorted(DECOMPOSITIONS))
def test_tiled_series_run_equals_untiled(name, transport):
    """Global-shape series cut per tile, on an in-process tile group: two momentum steps and one whole step, at two clock times."""
    Rx, Ry, kw = DECOMPOSITIONS[name]
    c = cases.make_case(H=8, substeps=14, patches=True, random_uv=0.05, **kw)
    data = forcing_data(c["g"])
    mk = dict(mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7))
    held = []
    with dynamics_hook(omip_hook(data, True, held, indexing=csi.Cyclical(1200.0), backend=csi.InMemory(2))):
        whole = _tile_run(cases.csi_model(c, **mk), c)

        def tile(rank, group):
            m = cases.csi_model(c, tile=(Rx, Ry, rank), local_group=group, **mk)
            assert len(m._series) == 6
            m.set_exchange_interval(0)
            if transport == "rccl":
                m.set_halo_transport("rccl")
            res = _tile_run(m, c)
            res["offsets"] = (m.grid.i_off, m.grid.j_off, m.grid.Nx, m.grid.Ny)
            del m
            return res
        tiles = run_tile_threads(Rx * Ry, tile)
    assert all(d["transport"] == transport for d in tiles), [d["transport"] for d in tiles]
    check_tiles(tiles, {f: whole[f"mom_{f}"] for f in ("u", "v", "s11", "s22", "s12")}, {f: whole[f"step_{f}"] for f in ("u", "v", "h", "a")},
                (name, transport))


# ---- checkpoint ---------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_restores_into_a_fresh_model_with_the_same_series():
    c = cases.make_case(Nx=48, Ny=32, topo=("periodic", "bounded"), substeps=8, random_uv=0.05)
    data = forcing_data(c["g"])
    kw = dict(mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7))
    held = []

    def build():
        with dynamics_hook(omip_hook(data, True, held, backend=csi.InMemory(3))):
            return cases.csi_model(c, **kw)
    m = build()
    for _ in range(3):
        csi.time_step(m, c["dt"])
    saved = csi.prognostic_state(m)
    for _ in range(3):
        csi.time_step(m, c["dt"])
    first = csi.prognostic_state(m)
    m2 = build()
    # a fresh model has interpolated its series at ITS clock (t = 0: the constructor and set!'s update_state!), so its window holds
    # that time's pair and the slice after it -- nothing of the run that was saved
    resident, uploads = m2.time_series_status("TOP_U")
    assert sorted(resident) == [0, 1, 2] and uploads == 3, (resident, uploads)
    csi.restore_prognostic_state(m2, saved)
    assert m2.clock.time == 3 * c["dt"]
    csi.time_step(m2, c["dt"])
    n1, n2, _ = ref.plan(TIMES, L.TIME_LINEAR, 0.0, 3 * c["dt"])
    resident, uploads = m2.time_series_status("TOP_U")
    assert (n1, n2) == (1, 2) and sorted(resident) == [1, 2, 3] and uploads == 4, (resident, uploads)      # the restored clock's pair + the next slice
    for _ in range(2):
        csi.time_step(m2, c["dt"])
    second = csi.prognostic_state(m2)
    assert second["clock"] == first["clock"]
    for k in first:
        if k != "clock":
            assert np.array_equal(first[k], second[k]), k


# ---- no series, no change -------------------------------------------------------------------------------------------------------------------
def test_a_model_without_series_never_calls_the_update():
    c = cases.make_case(Nx=48, Ny=32, substeps=8, wind_drag="arrays", field_forcing=True)
    m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7))
    assert not m._series
    calls, call = [], m.ctx.call
    m.ctx.call = lambda name, *a: (calls.append(name), call(name, *a))[1]
    csi.time_step(m, c["dt"])
    csi.time_step_momentum(m, c["dt"])
    csi.compute_momentum_tendencies(m, c["dt"])
    csi.update_state(m)
    m.synchronize()
    assert "csi_time_step_rk3" in calls and not [n for n in calls if "time_series" in n], calls
    before = (m.ctx.last_path(), m.ctx.last_launches())
    m.ctx.time_series_update(12.0)                                   # on such a context: CSI_OK, nothing launched
    assert (m.ctx.last_path(), m.ctx.last_launches()) == before and before[0]["level"] == 2
