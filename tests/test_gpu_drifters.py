"""GPU tests of the Lagrangian ice drifters (include/csi.h, "Lagrangian ice drifters"; csrc/drifters.hip): csi_drifters_advance and
csi_drifters_sample bit for bit against the NumPy restatement tests/drifters_ref.py, in both modes.  The velocity parents are poisoned
(NaN and 1e300) in every element outside the one halo ring the header names, so a read beyond it shows in the positions."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import drifters_cases as dc
import drifters_ref as ref

pytestmark = pytest.mark.gpu
L = csi._lib
SIZES = [(37, 29), (64, 16), (130, 33)]
_models = {}


def bare_model(Nx, Ny, topo, kind, land=False, snow=False):
    """A model without dynamics (u, v, h, aice are bound; nothing steps them) whose velocity parents are dc.parents' arrays, copied whole:
    what the kernels read is exactly what the restatement reads.  Cached: the tests only read it."""
    key = (Nx, Ny, topo, kind, land, snow)
    if key not in _models:
        g = dc.make_grid(Nx, Ny, topo, kind)
        kw = {}
        if snow:
            kw = dict(ice_thermodynamics=csi.SlabThermodynamics(top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance(), top_heat_flux=-70.0,
                                                                bottom_heat_flux=5.0, bottom_salinity=30.0),
                      snow_thermodynamics=csi.snow_slab_thermodynamics(), snowfall=2e-5)
        m = csi.SeaIceModel(g, timestepper="ForwardEuler", **kw)
        u, v = dc.parents(g, seed=Nx + len(topo) + len(kind))
        m.copy_to_field(m.velocities.u, u)
        m.copy_to_field(m.velocities.v, v)
        rng = np.random.default_rng(Nx)
        fields = {"u": u, "v": v}
        for name, f in (("h", m.ice_thickness), ("aice", m.ice_concentration), ("hs", m.snow_thickness)):
            if f is not None:
                fields[name] = rng.random(tuple(f.data.shape))
                m.copy_to_field(f, fields[name])
        active = dc.land(g, seed=Nx) if land else None
        if land:
            m.set_mask(active)
        _models[key] = (m, dc.ref_grid(g, active), fields)
    return _models[key]


def run_advance(m, g, xi, eta, dt, substeps):
    d = csi.Drifters(g, xi, eta, device=m.device)
    d.advance(m, dt, substeps)
    return d.numpy(m)


def check_advance(m, G, fields, xi, eta, dt, substeps, what):
    want = ref.advance(G, fields["u"], fields["v"], xi, eta, dt, substeps)
    got = run_advance(m, m.grid, xi, eta, dt, substeps)
    assert dc.same_bits(got[0], want[0]) and dc.same_bits(got[1], want[1]), what
    assert np.array_equal(got[2], want[2]), what
    return want


@pytest.mark.parametrize("topo", ["pp", "bb", "pb"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_advance_and_sample_match_the_restatement(size, topo):
    """Three metric kinds, with and without land, STRICT and FAST; 1000 drifters, 2 sub-steps that move them up to a few cells (walls are
    hit, land holds)."""
    for kind in dc.KINDS:
        for land in (False, True):
            m, G, fields = bare_model(*size, topo, kind, land)
            xi, eta = dc.positions(m.grid, 1000, seed=size[0])
            for mode in ("strict", "fast"):
                m.set_mode(mode)
                want = check_advance(m, G, fields, xi, eta, 5000.0, 2, (kind, land, mode))
                d = csi.Drifters(m.grid, want[0], want[1], device=m.device)
                got = d.sample(m, "xi", "eta", "u", "v", "h", "aice")
                m.synchronize()
                assert dc.same_bits(got.cpu().numpy(), ref.sample(G, fields, want[0], want[1], ref.COLUMNS[:6])), (kind, land, mode)
            moved = np.abs(want[0] - xi)
            assert np.nanmax(moved) > 1.0
            if land:
                assert ((want[2] & ref.HELD) != 0).any()
            if topo == "bb":
                assert ((want[2] & ref.CLAMPED_X) != 0).any()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_every_list_length_around_the_wave_and_the_block(n):
    m, G, fields = bare_model(37, 29, "pb", "full", True)
    before = m.ctx.drifters_stats()
    xi, eta = dc.positions(m.grid, n, seed=n)
    check_advance(m, G, fields, xi, eta, 3000.0, 1, n)
    assert m.ctx.drifters_stats() - before == (0 if n == 0 else 1)          # n == 0: a no-op without a launch
    d = csi.Drifters(m.grid, xi, eta, device=m.device)
    out = d.sample(m, "u", "xi")
    m.synchronize()
    assert out.shape == (2, n) and dc.same_bits(out.cpu().numpy(), ref.sample(G, fields, xi, eta, ("xi", "u")))
    assert m.ctx.drifters_stats() - before == (0 if n == 0 else 2)


@pytest.mark.parametrize("msub", [1, 2, 5])
def test_substeps_in_one_launch_equal_separate_advances(msub):
    m, G, fields = bare_model(64, 16, "bb", "per_j", True)
    xi, eta = dc.positions(m.grid, 300, seed=7)
    dt = 4321.0
    want = check_advance(m, G, fields, xi, eta, dt, msub, msub)
    d = csi.Drifters(m.grid, xi, eta, device=m.device)
    for _ in range(msub):
        d.advance(m, dt / msub, 1)
    x, y, _ = d.numpy(m)
    assert dc.same_bits(x, want[0]) and dc.same_bits(y, want[1])


@pytest.mark.parametrize("topo", ["pp", "bb", "pb"])
def test_edge_table_positions_and_the_status_they_must_get(topo):
    """The CPU suite's table as drifter positions: on and beyond every boundary, NaN, +-Inf, 1e300.  Safe by the clamp contract (every
    index is clamped as a double before the conversion); the NaN / Inf rows must come back untouched with INACTIVE, every other row inside
    the domain, held, or lost as (NaN, NaN)."""
    for kind in ("uniform", "full"):
        m, G, fields = bare_model(37, 29, topo, kind, True)
        xi, eta = ref.edge_positions(37, 29)
        for dt, msub in ((2500.0, 1), (-4000.0, 2), (0.0, 1)):
            want = check_advance(m, G, fields, xi, eta, dt, msub, (kind, dt))
            x, y, st = run_advance(m, m.grid, xi, eta, dt, msub)
            inactive = ~(np.isfinite(xi) & np.isfinite(eta))
            assert inactive.sum() > 50 and np.all(st[inactive] == ref.INACTIVE) and dc.same_bits(x[inactive], xi[inactive]) and dc.same_bits(y[inactive], eta[inactive])
            act = ~inactive
            lost, held = (st & ref.LOST) != 0, (st & ref.HELD) != 0
            inside = (x >= 0) & (x <= 37) & (y >= 0) & (y <= 29)
            assert np.all(inside[act] | held[act] | (lost[act] & np.isnan(x[act]) & np.isnan(y[act])))
            assert lost[act].any()                      # the 1e300 rows
        s = csi.Drifters(m.grid, xi, eta, device=m.device).sample(m, *ref.COLUMNS[:6])
        m.synchronize()
        s = s.cpu().numpy()
        assert dc.same_bits(s, ref.sample(G, fields, xi, eta, ref.COLUMNS[:6])) and np.isnan(s[:, inactive]).all()


def test_drifters_are_held_at_land_and_clamped_at_walls():
    g = csi.RectilinearGrid((8, 6), x=(0.0, 8000.0), y=(0.0, 6000.0), topology=(csi.Bounded, csi.Bounded), halo=(2, 2))
    m = csi.SeaIceModel(g, timestepper="ForwardEuler")
    active = np.ones((6, 8), dtype=bool)
    active[2, 4] = False
    m.set_mask(active)
    m.copy_to_field(m.velocities.u, np.ones(tuple(m.velocities.u.data.shape)))
    xi, eta = np.array([3.5, 3.5, 7.5, 0.25]), np.array([2.5, 3.5, 1.0, 5.0])
    x, y, st = run_advance(m, g, xi, eta, 1000.0, 1)
    assert list(x) == [3.5, 4.5, 8.0, 1.25] and list(y) == list(eta) and list(st) == [ref.HELD, 0, ref.CLAMPED_X, 0]
    x, y, st = run_advance(m, g, xi, eta, 1000.0, 2)
    assert x[0] == 3.5 and st[0] == ref.HELD
    x, y, st = run_advance(m, g, xi[:1], eta[:1], 2000.0, 1)
    assert x[0] == 5.5 and st[0] == 0
    d = csi.Drifters(g, xi, eta, device=m.device).advance(m, 1000.0)
    assert d.status_counts(m) == dict(free=2, clamped_x=1, clamped_y=0, held=1, lost=0, inactive=0)


def _stepped_model(timestepper="SplitRungeKutta3", **kw):
    c = cases.make_case(substeps=10, patches=True, random_uv=0.03, **kw)
    return c, cases.csi_model(c, mode="fast", timestepper=timestepper, advection=csi.WENO(order=5))


def _ref_of_model(m, c):
    return dc.ref_grid(m.grid, c.get("mask"))


def test_no_slip_wall():
    """A channel with ValueBoundaryCondition(0) on the tangential velocity: the first halo row of u holds -u of the first interior row, so
    the interpolated rate falls to zero ON the wall; drifters seeded on and next to the walls against the restatement fed the model's
    fields, and those on the wall do not move along it."""
    c, m = _stepped_model(Nx=48, Ny=24, topo=("periodic", "bounded"), noslip=True)
    csi.time_step(m, c["dt"])
    m.synchronize()
    G = _ref_of_model(m, c)
    u, v = m.velocities.u.numpy(), m.velocities.v.numpy()
    xs = np.linspace(0.3, 47.6, 40)
    xi = np.concatenate([xs, xs, xs, xs])
    eta = np.concatenate([np.zeros(40), np.full(40, 24.0), np.full(40, 0.3), np.full(40, 23.6)])
    want = ref.advance(G, u, v, xi, eta, 50 * c["dt"], 2)
    got = run_advance(m, m.grid, xi, eta, 50 * c["dt"], 2)
    assert dc.same_bits(got[0], want[0]) and dc.same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])
    a, _ = ref.rate(G, u, v, xi[:80], eta[:80])
    assert np.all(a == 0.0) and np.abs(ref.rate(G, u, v, xi[80:], eta[80:])[0]).max() > 0.0


def test_model_stepped_three_rk3_steps_with_drifters_set():
    """model.drifters: time_step advances them after each step with the step's dt and the velocities it leaves."""
    for kw in (dict(Nx=40, Ny=32, topo=("periodic", "periodic")), dict(Nx=37, Ny=29, topo=("bounded", "bounded"), grid="latlon", land=0.2)):
        c, m = _stepped_model(**kw)
        G = _ref_of_model(m, c)
        before = m.ctx.drifters_stats()
        m.drifters = csi.Drifters.at_cell_centers(m.grid, stride=2, substeps=2)
        xi, eta, _ = m.drifters.numpy()
        for step in range(3):
            csi.time_step(m, 20 * c["dt"])
            got = m.drifters.numpy(m)                       # (waits for the model's stream: the fields below are the step's)
            want = ref.advance(G, m.velocities.u.numpy(), m.velocities.v.numpy(), xi, eta, 20 * c["dt"], 2)
            assert dc.same_bits(got[0], want[0]) and dc.same_bits(got[1], want[1]) and np.array_equal(got[2], want[2]), (kw, step)
            assert not np.array_equal(got[0], xi)
            xi, eta = want[0], want[1]
        assert m.ctx.drifters_stats() - before == 3


@pytest.mark.parametrize("snow", [False, True])
def test_sampling_every_column_alone_and_all_together(snow):
    m, G, fields = bare_model(37, 29, "pb", "uniform", False, snow)
    xi, eta = dc.positions(m.grid, 257, seed=3)
    xi[5], eta[9] = np.nan, np.inf
    d = csi.Drifters(m.grid, xi, eta, device=m.device)
    names = ref.COLUMNS if snow else ref.COLUMNS[:6]
    for cols in [(n,) for n in names] + [names, names[::-1], ("v", "xi")]:
        out = d.sample(m, *cols)
        m.synchronize()
        want = ref.sample(G, fields, xi, eta, cols)
        assert out.shape == want.shape and dc.same_bits(out.cpu().numpy(), want), cols
    assert np.isnan(want[:, 5]).all() and np.isnan(want[:, 9]).all()
    if not snow:
        with pytest.raises(ValueError, match="snow layer"):
            d.sample(m, "hs")
        with pytest.raises(csi.CsiError, match="field hs is requested") as e:          # ... and by the library, by name
            m.ctx.drifters_sample(d._struct(), L.DRIFTER_COL_HS, d.xi.data_ptr(), d.n)
        assert e.value.code == -2


def test_checkpoint_round_trip_mid_run():
    c = cases.make_case(Nx=40, Ny=32, substeps=10, patches=True, random_uv=0.03)

    def build(stride):
        m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
        m.drifters = csi.Drifters.at_cell_centers(m.grid, stride=stride, substeps=1)
        return m
    a = build(4)
    for _ in range(2):
        csi.time_step(a, 30 * c["dt"])
    ckpt = csi.prognostic_state(a)
    for _ in range(2):
        csi.time_step(a, 30 * c["dt"])
    want = csi.prognostic_state(a)
    b = build(4)
    csi.time_step(b, 7 * c["dt"])
    csi.restore_prognostic_state(b, ckpt)
    for _ in range(2):
        csi.time_step(b, 30 * c["dt"])
    got = csi.prognostic_state(b)
    assert {"drifters.xi", "drifters.eta", "drifters.status"} <= set(got) and set(got) == set(want)
    for k in ("drifters.xi", "drifters.eta", "drifters.status", "u", "h"):
        assert dc.same_bits(got[k], want[k]), k
    assert not np.array_equal(ckpt["drifters.xi"], want["drifters.xi"])


def test_writer_records_tracks(tmp_path):
    c, m = _stepped_model(Nx=40, Ny=32, topo=("periodic", "bounded"))
    G = _ref_of_model(m, c)
    m.drifters = csi.Drifters.at_cell_centers(m.grid, stride=4)
    m.output_writers["tracks"] = csi.DrifterWriter(m.drifters, csi.IterationInterval(1), str(tmp_path / "tracks"), columns=("xi", "eta", "u", "aice"))
    want = [m.drifters.numpy(m)]
    sampled = []
    for _ in range(3):
        csi.time_step(m, 25 * c["dt"])
        want.append(m.drifters.numpy(m))
        fields = {"u": m.velocities.u.numpy(), "v": m.velocities.v.numpy(), "aice": m.ice_concentration.numpy()}
        sampled.append(ref.sample(G, fields, want[-1][0], want[-1][1], ("u", "aice")))
    m.output_writers["tracks"].close()
    out = csi.load_tracks(str(tmp_path / "tracks"))
    assert out["xi"].shape == (4, m.drifters.n) and list(out["iteration"]) == [0, 1, 2, 3]
    for k in range(4):
        assert dc.same_bits(out["xi"][k], want[k][0]) and dc.same_bits(out["eta"][k], want[k][1]) and np.array_equal(out["status"][k], want[k][2])
    for k in range(3):
        assert dc.same_bits(out["u"][k + 1], sampled[k][0]) and dc.same_bits(out["aice"][k + 1], sampled[k][1])


def _raw_context(topo_x, topo_y, bind=True):
    ctx = csi.Context(0)
    met = L.Metrics()
    met.dx, met.dy = 1000.0, 1000.0
    ctx.call("csi_grid_set", 16, 12, 4, 4, topo_x, topo_y, L.METRIC_UNIFORM, C.byref(met))
    wall = lambda t: int(t in (L.BOUNDED, L.LEFT_CONNECTED))      # noqa: E731  (a Face field has one more point on a high wall)
    keep = [torch.zeros((12 + 8 + ey, 16 + 8 + ex), dtype=torch.float64, device="cuda:0") for ex, ey in ((wall(topo_x), 0), (0, wall(topo_y)))]
    if bind:
        for slot, t in zip(("U", "V"), keep):
            ctx.call("csi_field_bind", L.slot_id(slot), C.c_void_p(t.data_ptr()), t.shape[1], t.shape[1], t.shape[0])
    torch.cuda.synchronize()
    return ctx, keep


def test_tiled_and_folded_contexts_and_bad_arguments_refuse_by_name():
    xi = torch.full((4,), 2.5, dtype=torch.float64, device="cuda:0")
    eta = torch.full((4,), 3.25, dtype=torch.float64, device="cuda:0")
    st = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    out = torch.zeros((2, 4), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    d = L.Drifters(4, xi.data_ptr(), eta.data_ptr(), st.data_ptr())

    def refused(ctx, code, text, fn, *args):
        with pytest.raises(csi.CsiError, match=text) as e:
            fn(*args)
        assert e.value.code == code
        assert ctx.drifters_stats() == 0

    for tx, ty, text in ((L.FULLY_CONNECTED, L.PERIODIC, "tiled context"), (L.PERIODIC, L.LEFT_CONNECTED, "tiled context"),
                         (L.PERIODIC, L.RIGHT_FOLDED, "RIGHT_FOLDED"), (L.PERIODIC, L.LEFT_CONNECTED_RIGHT_FOLDED, "tiled context")):
        ctx, keep = _raw_context(tx, ty)
        refused(ctx, -4, text, ctx.drifters_advance, d, 10.0, 1)
        refused(ctx, -4, text, ctx.drifters_sample, d, 3, out.data_ptr(), 4)
        ctx.close()
    ctx, keep = _raw_context(L.PERIODIC, L.BOUNDED, bind=False)
    refused(ctx, -2, "field u", ctx.drifters_advance, d, 10.0, 1)
    ctx.close()
    ctx, keep = _raw_context(L.PERIODIC, L.BOUNDED)
    refused(ctx, -1, "dt is not finite", ctx.drifters_advance, d, float("nan"), 1)
    refused(ctx, -1, "substeps < 1", ctx.drifters_advance, d, 10.0, 0)
    refused(ctx, -1, "n < 0", ctx.drifters_advance, L.Drifters(-1, xi.data_ptr(), eta.data_ptr(), st.data_ptr()), 10.0, 1)
    refused(ctx, -1, "NULL with n > 0", ctx.drifters_advance, L.Drifters(4, None, eta.data_ptr(), st.data_ptr()), 10.0, 1)
    refused(ctx, -1, "unknown bit", ctx.drifters_sample, d, 128, out.data_ptr(), 4)
    refused(ctx, -1, "unknown bit", ctx.drifters_sample, d, 0, out.data_ptr(), 4)
    refused(ctx, -1, "ld < n", ctx.drifters_sample, d, 3, out.data_ptr(), 3)
    refused(ctx, -1, "dev_out == NULL", ctx.drifters_sample, d, 3, None, 4)
    refused(ctx, -2, "field h is requested", ctx.drifters_sample, d, L.DRIFTER_COL_H, out.data_ptr(), 4)
    ctx.drifters_advance(L.Drifters(0, None, None, None), 10.0, 1)      # n == 0: accepted, nothing launched
    assert ctx.drifters_stats() == 0
    ctx.drifters_advance(d, 10.0, 3)
    ctx.call("csi_sync")
    assert ctx.drifters_stats() == 1 and xi.cpu().tolist() == [2.5] * 4 and eta.cpu().tolist() == [3.25] * 4 and st.cpu().tolist() == [0] * 4      # u = v = 0: nobody moves
    ctx.close()


def test_a_model_that_never_sets_drifters_launches_none():
    c, m = _stepped_model(Nx=40, Ny=32)
    assert m.drifters is None
    for _ in range(2):
        csi.time_step(m, c["dt"])
    m.synchronize()
    assert m.ctx.drifters_stats() == 0 and not any(k.startswith("drifters") for k in csi.prognostic_state(m))
