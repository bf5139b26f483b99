"""GPU tests of csi_derived_compute / csi_budget_compute (include/csi.h): the seven derived fields and the three energy budget sums, bit for
bit against the NumPy restatement (tests/derived_ref.py) in both modes, at the block edges of the two kernels, on every topology and
metric kind, with and without land, with NaN in every halo element the contract says is not read; the errors by name; the state after
real RK3 steps; the reference's adjoint identity; tiles; the output writer's hook; and a model that never asks for any of it."""
import math

import numpy as np
import pytest
import torch

import cases
import climaseaice_jl_amd as csi
import derived_ref as ref
import diagnostics_ref as dref
import output_ref

pytestmark = pytest.mark.gpu
L = csi._lib
SENTINEL = 7.25


def case_of(shape, topo, metrics, **kw):
    """The grids of derived_ref.grid_of through cases.make_case (the same constructors and numbers)."""
    rect = metrics in ("uniform", "distorted_rectilinear")
    return cases.make_case(Nx=shape[0], Ny=shape[1], topo=ref.TOPOS[topo], grid="rectilinear" if rect else "latlon",
                           curvilinear=0.05 if metrics in ("curvilinear", "distorted_rectilinear") else None, substeps=4, patches=False, **kw)


def state_fields(m):
    f = m.dynamics.auxiliaries.fields
    return {"u": m.velocities.u, "v": m.velocities.v, "s11": f.s11, "s22": f.s22, "s12": f.s12, "P": f.P, "h": m.ice_thickness,
            "a": m.ice_concentration}


def load(m, par):
    for k, fld in state_fields(m).items():
        m.copy_to_field(fld, par[k])


def download(m):
    m.synchronize()
    return {k: fld.numpy().copy() for k, fld in state_fields(m).items()}


def set_land(m, wet):
    """The model's mask from (Ny, Nx) wet cells (None: no mask); returns the mask's parent as the library reads it."""
    if wet is None:
        m.ctx.call("csi_mask_set", None, 0)
        return None
    m.set_mask(wet)
    return m.mask.cpu().numpy()


def budget_bits(b, want):
    return [k for k in want if not dref.same_bits(getattr(b, k), want[k])]


# ---- every shape x topology x metric kind, with and without land, both modes ---------------------------------------------------------------
@pytest.mark.parametrize("metrics", ref.METRICS)
@pytest.mark.parametrize("topo", list(ref.TOPOS))
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fields_and_budget_equal_the_restatement_bitwise(shape, topo, metrics):
    c = case_of(shape, topo, metrics)
    g = c["g"]
    m = cases.csi_model(c, mode="fast")
    names = ref.NAMES
    for land in (False, True):
        # derived fields: NaN in every element outside "HALO ELEMENTS READ"; P == 0 in a patch and in the last cell
        par, wet = ref.white_noise(g, seed=11 + land, land=land, poison="derived")
        mask = set_land(m, wet)
        load(m, par)
        want = ref.Ref(g, par, mask).fields()
        assert np.all(want["sigma_I"][par["P"][g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx] == 0] == 0.0)
        for mode in ("strict", "fast"):
            m.set_mode(mode)
            fields = m.compute_derived(*names)            # all seven in one call
            m.synchronize()
            for n, fld in zip(names, fields):
                got = fld.interior_numpy()
                assert ref.same_bits(got, want[n]), (n, mode, land, np.argwhere(got != want[n])[:4])
                assert np.all(np.isfinite(got))
        for fld in fields:
            fld.fill_parent(SENTINEL)
        for n in names:                                   # every field alone: that interior and nothing else is written
            m.compute_derived(n)
            m.synchronize()
            for k, fld in zip(names, fields):
                parent = fld.numpy()
                inner = parent[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx]
                if k == n:
                    assert ref.same_bits(inner, want[n]), (n, "alone", land)
                    outer = parent.copy()
                    outer[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx] = SENTINEL
                    assert np.all(outer == SENTINEL), (n, "halo written")
                else:
                    assert np.all(parent == SENTINEL), (k, "written by a call for", n)
            m.derived_field(n).fill_parent(SENTINEL)
        # the budget: its own (larger) set of elements
        par, _ = ref.white_noise(g, seed=11 + land, land=land, poison="budget")
        load(m, par)
        sums = ref.Ref(g, par, mask, rho=m.sea_ice_density).budget()
        assert all(math.isfinite(v) for v in sums.values())
        for mode in ("strict", "fast"):
            m.set_mode(mode)
            assert budget_bits(m.energy_budget(), sums) == [], (mode, land)
        b = m.energy_budget("stress")
        assert budget_bits(b, {k: sums[k] for k in ("internal_work", "stress_power")}) == [] and b.kinetic_energy is None
        b = m.energy_budget("kinetic")
        assert budget_bits(b, {"kinetic_energy": sums["kinetic_energy"]}) == [] and b.internal_work is None and b.imbalance is None
    assert m.ctx.derived_stats() == (2 * (2 + 7), 2 * 4)


def test_budget_with_more_records_than_the_finishing_block_has_threads():
    """1030 x 961 cells are 17 x 16 = 272 records (the last block column six cells wide, the last block row one cell high): threads
    0 .. 15 of the finishing block add two records each, the strided part of the order that no smaller grid reaches.  Uniform metrics,
    doubly periodic, both groups, one call per mode, bit for bit against the restatement."""
    c = case_of((1030, 961), "periodic", "uniform")
    g = c["g"]
    assert -(-g.Nx // 64) * -(-g.Ny // 64) == 272
    m = cases.csi_model(c, mode="strict")
    par, _ = ref.white_noise(g, seed=17, land=False, poison="budget")
    set_land(m, None)
    load(m, par)
    sums = ref.Ref(g, par, None, rho=m.sea_ice_density).budget()
    assert all(math.isfinite(v) for v in sums.values())
    for mode in ("strict", "fast"):
        m.set_mode(mode)
        assert budget_bits(m.energy_budget(), sums) == [], mode


# ---- errors by name ----------------------------------------------------------------------------------------------------------------------------
def test_errors_by_name():
    c = case_of((37, 29), "periodic", "uniform")
    m = cases.csi_model(c)
    with pytest.raises(csi.CsiError, match="shear") as e:          # the slot is not bound
        m.ctx.derived_compute(2)
    assert e.value.code == -2
    m.derived_field("shear")
    m.ctx.derived_compute(2)
    with pytest.raises(csi.CsiError, match="divergence") as e:
        m.ctx.derived_compute(3)
    assert e.value.code == -2
    for mask in (0, 128, -1):
        with pytest.raises(csi.CsiError, match="mask") as e:
            m.ctx.derived_compute(mask)
        assert e.value.code == -1
    for what in (0, 4):
        with pytest.raises(csi.CsiError, match="what") as e:
            m.ctx.budget_compute(what)
        assert e.value.code == -1
    with pytest.raises(ValueError, match="divergence, shear"):
        m.compute_derived("vorticity")
    # a viscous model has no stress fields: the stress group is refused naming sigma11, the strain group works
    g = c["g"]
    dyn = csi.SeaIceMomentumEquation(g, rheology=csi.ViscousRheology(nu=1000.0), solver=csi.SplitExplicitSolver(substeps=4), device="cuda:0")
    v = csi.SeaIceModel(g, dynamics=dyn, timestepper="ForwardEuler")
    csi.set_(v, h=c["h"], aice=c["a"], u=c["u"], v=c["v"])
    for call in (lambda: v.compute_derived("sigma_I"), lambda: v.compute_derived("shear", "stress_power"), lambda: v.energy_budget("stress"),
                 lambda: v.energy_budget()):
        with pytest.raises(csi.CsiError, match="sigma11") as e:
            call()
        assert e.value.code == -2
    shear, = v.compute_derived("shear")
    v.synchronize()
    par = {"u": v.velocities.u.numpy(), "v": v.velocities.v.numpy()}
    assert ref.same_bits(shear.interior_numpy(), ref.Ref(g, par).fields(("shear",))["shear"])
    assert v.energy_budget("kinetic").kinetic_energy > 0.0
    # a model without dynamics binds u, v (prescribed velocities): the strain group works, the stress group names sigma11
    n = csi.SeaIceModel(g, dynamics=None, advection=None, timestepper="ForwardEuler")
    with pytest.raises(csi.CsiError, match="sigma11"):
        n.compute_derived("sigma_II")
    assert "shear" not in csi.bound_fields(n)
    n.compute_derived("speed")
    assert "speed" in csi.bound_fields(n) and csi.bound_fields(n)["speed"][1] == "D_SPEED"


# ---- after real steps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "strict"])
@pytest.mark.parametrize("config", ["bounded_latlon_land", "periodic_uniform", "channel_curvilinear"])
def test_after_three_rk3_steps(config, mode):
    """The halo elements the entry points read are the ones the step entry points leave valid: fields and budget of the stepped state
    against the restatement fed the DOWNLOADED parents, halos included."""
    topo, metrics, land = {"bounded_latlon_land": ("bounded", "latlon", 0.2), "periodic_uniform": ("periodic", "uniform", 0.0),
                           "channel_curvilinear": ("channel", "curvilinear", 0.0)}[config]
    c = case_of((65, 65), topo, metrics, land=land, random_uv=0.02)
    c["substeps"] = 12
    m = cases.csi_model(c, mode=mode, timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    for _ in range(3):
        csi.time_step(m, c["dt"])
    fields = m.compute_derived(*ref.NAMES)
    b = m.energy_budget()
    par = download(m)
    mask = m.mask.cpu().numpy() if land else None
    r = ref.Ref(c["g"], par, mask, rho=m.sea_ice_density)
    want = r.fields()
    for n, fld in zip(ref.NAMES, fields):
        got = fld.interior_numpy()
        assert np.all(np.isfinite(got)) and ref.same_bits(got, want[n]), (n, np.argwhere(got != want[n])[:4])
    assert np.abs(want["shear"]).max() > 0.0 and np.abs(want["sigma_II"]).max() > 0.0
    assert budget_bits(b, r.budget()) == []
    assert b.kinetic_energy > 0.0 and b.imbalance == ref.imbalance(b.internal_work, b.stress_power)


# ---- the reference's identity on the device ---------------------------------------------------------------------------------------------------
IDENTITY = {"latlon_bounded_40": ((40, 40), "bounded", "latlon"), "rectilinear_periodic": ((37, 29), "periodic", "uniform"),
            "curvilinear_periodic": ((37, 29), "periodic", "distorted_rectilinear"), "latlon_channel": ((64, 33), "channel", "latlon")}


@pytest.mark.parametrize("name", list(IDENTITY))
def test_energy_identity(name):
    """imbalance < 1e-10, the reference's own bound (test/test_rheology_energy_budget.jl:117), on unmasked grids with unit white noise
    in u, v, sigma that vanishes on and beyond the walls (two-cell margin) or is periodic."""
    shape, topo, metrics = IDENTITY[name]
    c = case_of(shape, topo, metrics)
    m = cases.csi_model(c)
    par, _ = ref.white_noise(c["g"], seed=21, margin=2, zero_P=False, unit=True)
    load(m, par)
    b = m.energy_budget("stress")
    print(name, "W", b.internal_work, "D", b.stress_power, "imbalance", b.imbalance)
    assert abs(b.stress_power) > 0.0
    assert b.imbalance < 1e-10
    assert budget_bits(b, ref.Ref(c["g"], par).budget(("internal_work", "stress_power"))) == []


# ---- tiles --------------------------------------------------------------------------------------------------------------------------------------
TILES = {"2x1_bounded_x": (2, 1, dict(Nx=128, Ny=64, topo=("bounded", "periodic"))),
         "1x2_fold": (1, 2, dict(Nx=192, Ny=192, topo=("periodic", "folded")))}


@pytest.mark.parametrize("name", list(TILES))
def test_tiles(name):
    """Derived fields of the tiles, reassembled, equal the untiled run bit for bit (rank-local, no communication; on the fold the halo
    images carry the sign); the budget sums are equal on all ranks and within rounding of the untiled run's."""
    from test_gpu_local_tiles import run_tile_threads
    Rx, Ry, kw = TILES[name]
    c = cases.make_case(substeps=8, random_uv=0.02, **kw)

    def run(m):
        for _ in range(2):
            csi.time_step(m, c["dt"])
        fields = m.compute_derived(*ref.NAMES)
        b = m.energy_budget()
        m.synchronize()
        return {n: f.interior_numpy().copy() for n, f in zip(ref.NAMES, fields)}, b

    def tile(rank, group):
        m = cases.csi_model(c, timestepper="SplitRungeKutta3", advection=csi.WENO(order=5), tile=(Rx, Ry, rank), local_group=group)
        out = run(m)
        g = m.grid
        return out + ((g.i_off, g.j_off),)

    whole = cases.csi_model(c, timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    want, bw = run(whole)
    parts = run_tile_threads(Rx * Ry, tile)
    for n in ref.NAMES:
        got = np.full_like(want[n], np.nan)
        for fields, _, (i0, j0) in parts:
            a = fields[n]
            got[j0:j0 + a.shape[0], i0:i0 + a.shape[1]] = a
        assert ref.same_bits(got, want[n]), (n, np.argwhere(got != want[n])[:4])
    # the same terms in another tree: each sum within the order-independent bound of the exact sum, so within twice it of each other
    terms = ref.Ref(c["g"], download(whole), None, rho=whole.sea_ice_density).terms()
    for k in ref.SUMS:
        vals = [getattr(b, k) for _, b, _ in parts]
        assert all(dref.same_bits(v, vals[0]) for v in vals), k
        _, bound = dref.fsum_bound(terms[k])
        print(name, k, "tiled", vals[0], "untiled", getattr(bw, k), "difference", vals[0] - getattr(bw, k), "bound", 2 * bound)
        assert abs(vals[0] - getattr(bw, k)) <= 2 * bound, k


# ---- the output writer ------------------------------------------------------------------------------------------------------------------------
def test_writer_with_derived_outputs(tmp_path):
    """["h", "shear", "divergence"], snapshots and time averages: the records equal the stand-in's arithmetic on the restatement's
    fields of a twin's downloaded states."""
    c = case_of((65, 65), "bounded", "latlon", random_uv=0.02)
    c["substeps"] = 8
    dt, names = c["dt"], ["h", "shear", "divergence"]
    mk = lambda: cases.csi_model(c, timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    twin, states = mk(), []

    def state():
        par = download(twin)
        f = ref.Ref(c["g"], par).fields(("shear", "divergence"))
        f["h"] = output_ref.interior(par["h"], 4, 4).copy()
        return f
    states.append(state())
    for _ in range(4):
        csi.time_step(twin, dt)
        states.append(state())
    m = mk()
    m.output_writers["snap"] = csi.OutputWriter(m, names, csi.IterationInterval(2), str(tmp_path / "snap"), dtype="f64")
    m.output_writers["avg"] = csi.OutputWriter(m, names, csi.AveragedTimeInterval(2 * dt), str(tmp_path / "avg"), dtype="f32")
    assert m.output_writers["snap"].derived == ("shear", "divergence")
    for _ in range(4):
        csi.time_step(m, dt)
    for w in m.output_writers.values():
        w.close()
    snap, avg = csi.load_output(str(tmp_path / "snap")), csi.load_output(str(tmp_path / "avg"))
    assert list(snap["iteration"]) == [0, 2, 4] and list(avg["time"]) == [2 * dt, 4 * dt]
    for n in names:
        for r, it in enumerate((0, 2, 4)):
            assert output_ref.same_bits(snap[n][r], states[it][n]), ("snap", n, it)
        for r in range(2):
            want = output_ref.element(output_ref.averaged([states[2 * r + k][n] for k in (1, 2)], [dt] * 2), "f32")
            assert output_ref.same_bits(avg[n][r], want), ("avg", n, r)
    # snapshots: 3 records; averages: 4 accumulates + 2 records -- one launch each, for either writer
    assert m.ctx.derived_stats() == (3 + 6, 0)


def test_a_model_that_never_asks_makes_none_of_the_new_calls(tmp_path, monkeypatch):
    c = case_of((65, 65), "bounded", "latlon", random_uv=0.02)
    m = cases.csi_model(c, timestepper="SplitRungeKutta3", advection=csi.WENO(order=5))
    called = []
    for name in ("derived_compute", "budget_compute"):
        monkeypatch.setattr(type(m.ctx), name, lambda self, *a, _n=name: called.append(_n))
    with csi.OutputWriter(m, ["h", "u", "sigma12"], csi.IterationInterval(1), str(tmp_path / "w")) as w:
        m.output_writers["w"] = w
        assert w.derived == ()
        for _ in range(2):
            csi.time_step(m, c["dt"])
        m.diagnostics()
    monkeypatch.undo()
    assert called == [] and m.ctx.derived_stats() == (0, 0)
    assert m._derived_fields == {} and not any(n in csi.bound_fields(m) for n in csi.DERIVED_NAMES)
