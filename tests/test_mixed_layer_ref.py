"""The slab-ocean mixed layer without a GPU: the restatement tests/mixed_layer_ref.py against its own heat budget, its branches, the
RK3 stage restart and the ice step's energy closure; the layouts of include/csi.h as gcc, ctypes and the Julia stub see them; the
Python front end's checks, its series slots and the writer hook."""
import ctypes as C
import json
import os
import re
import subprocess
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest

import climaseaice_jl_amd as csi
import mixed_layer_ref as M
import output_ref
import thermo_linear_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = csi._lib

PAIRS = [(10.0, 600.0), (50.0, 3600.0), (2.0, 60.0), (200.0, 86400.0), (10.0, 3600.0)]      # (depth, dt)


def _budget(depth, dt, seed, variant=None, **kw):
    s = M.random_state(200_000, seed)
    r = M.step(s["To"], s["a"], dt, depth, Fo=s["Fo"], K=s["K"], Ta=s["Ta"], Qd=s["Qd"], Sb=s["Sb"], variant=variant, **kw)
    return s, r, M.budget_residual(s["To"], r, dt, s["Qd"]), M.budget_bound(s["To"], r, dt, s["Qd"])


@pytest.mark.parametrize("depth, dt", PAIRS)
def test_budget_holds_to_rounding(depth, dt):
    """C (To' - To) / dt = Qd - Qow - Qb per cell within 16 * 2^-53 * (C (|To| + |To'| + |Tf|) / dt + |Qow| + |Qd| + |Qio| + |Qfr|) on
    200 000 random cells around freezing.  Measured share of the bound, largest cell: 0.095 (10 m, 600 s), 0.097 (50 m, 3600 s),
    0.094 (2 m, 60 s), 0.092 (200 m, 86400 s), 0.087 (10 m, 3600 s); with gamma = 1e-2 (melt limited by the heat there is) 0.095, 0.097,
    0.094, 0.111, 0.096."""
    for gamma in (M.GAMMA, 1e-2):
        s, r, res, bound = _budget(depth, dt, seed=int(depth * 7 + dt), gamma=gamma)
        assert np.all(np.isfinite(res)) and (r["Qfr"] < 0).any() and (r["Qio"] > 0).any()
        share = (res / bound).max()
        print(f"budget depth={depth} dt={dt} gamma={gamma}: largest share of the bound {share:.3f}")
        assert np.all(res <= bound), share


@pytest.mark.parametrize("variant", ["frazil_sign", "no_open_water_weight"])
def test_the_budget_check_can_fail(variant):
    """With Qfr's sign flipped or the (1 - a) weight dropped the same check fails by orders of magnitude: the largest residual is
    4.8e14 (sign) / 8.7e12 (weight) times its bound at depth 10 m, dt 600 s."""
    s, r, res, bound = _budget(10.0, 600.0, seed=3, variant=variant)
    factor = (res / bound).max()
    print(f"{variant}: residual / bound = {factor:.2e}")
    assert factor > 1e9


def test_every_branch_has_cells_and_behaves():
    inp, kw = M.branch_state((8, 9))
    To, a = inp["To"], inp["a"]
    r = M.step(To, a, Fo=inp["Fo"], **kw)
    n = M.branch_counts(To, a, r, kw["dt"], kw["gamma"])
    assert kw["gamma"] * kw["dt"] >= kw["depth"]
    assert all(n[b] >= 6 for b in M.BRANCHES), n
    Tf, dT = r["Tf"], To - r["Tf"]
    fr = r["Qfr"] < 0
    assert np.array_equal(r["To"][fr], Tf[fr]) and np.all(r["To"][~fr] >= Tf[~fr]) and np.all(r["Qfr"][~fr] == 0)
    cap = (r["C"] * dT) / kw["dt"]
    free = ((kw["gamma"] * (M.RHO * M.CP)) * dT) * a
    lim = (dT > 0) & (a > 0) & (free >= cap)
    assert np.array_equal(r["Qio"][lim], cap[lim]) and np.array_equal(r["Qio"][(dT > 0) & (free < cap)], free[(dT > 0) & (free < cap)])
    assert np.all(r["Qio"][dT <= 0] == 0) and np.all(r["Qio"][a == 0] == 0) and np.all(r["Qio"] >= 0)
    assert np.all(r["Qow"][a == 1] == 0) and np.array_equal(r["Qow"][a == 0], inp["Fo"][a == 0])
    assert np.array_equal(r["Qb"], r["Qio"] + r["Qfr"])
    res, bound = M.budget_residual(To, r, kw["dt"], 0.0), M.budget_bound(To, r, kw["dt"], 0.0)
    assert np.all(res <= bound)


def test_absent_terms_are_not_added():
    s = M.random_state(5000, 5)
    base = dict(dt=600.0, depth=10.0, Qd=s["Qd"], Sb=s["Sb"])
    none = M.step(s["To"], s["a"], **base)
    assert np.all(none["Qow"] == 0) and not np.signbit(none["Qow"]).any()
    fo = M.step(s["To"], s["a"], Fo=s["Fo"], **base)
    assert np.array_equal(fo["Qow"], s["Fo"] * (1 - s["a"]))
    bulk = M.step(s["To"], s["a"], K=s["K"], Ta=s["Ta"], **base)
    assert np.array_equal(bulk["Qow"], (s["K"] * (s["To"] - s["Ta"])) * (1 - s["a"]))
    both = M.step(s["To"], s["a"], Fo=s["Fo"], K=s["K"], Ta=s["Ta"], **base)
    assert np.array_equal(both["Qow"], (s["Fo"] + (s["K"] * (s["To"] - s["Ta"]))) * (1 - s["a"]))
    # a zero surface flux that is PRESENT is added: -0.0 + 0.0 differs from -0.0 alone
    z = M.step(np.array([1.0]), np.array([0.5]), 600.0, 10.0, Fo=0.0, K=-0.0, Ta=1.0)
    assert z["Qow"][0] == 0 and not np.signbit(z["Qow"][0])


def test_three_stages_from_the_cache_equal_one_step():
    """RK3: every stage computes To from Psi^- with its own stage step; the last one (the whole step) is the result.  Chaining the
    stages instead advances To by 11/6 of the step."""
    s = M.random_state(4000, 9)
    rng = np.random.default_rng(10)
    a_stages = [np.clip(s["a"] + 0.01 * rng.standard_normal(s["a"].size), 0, 1) for _ in range(3)]
    kw = dict(Fo=s["Fo"], K=s["K"], Ta=s["Ta"], Qd=s["Qd"], Sb=s["Sb"])
    dt, depth = 1200.0, 20.0
    staged = M.rk3_stages(s["To"], a_stages, dt, depth, **kw)
    one = M.step(s["To"], a_stages[2], dt, depth, **kw)
    assert all(np.array_equal(staged[k], one[k]) for k in ("To", "Qb", "Qow"))
    To = s["To"]
    for beta, a in zip((3, 2, 1), a_stages):
        To = M.step(To, a, dt / beta, depth, **kw)["To"]
    warm = (one["Qfr"] == 0) & (one["Qio"] == 0)          # (cells that neither freeze nor melt: their change is linear in the step)
    assert warm.sum() > 100 and not np.array_equal(To, one["To"])
    ratio = (To - s["To"])[warm] / (one["To"] - s["To"])[warm]
    assert np.median(ratio) > 1.5


# ---- coupled closure: ice plus ocean (test/test_energy_conservation.jl per cell, with q_bottom = Qb) -----------------------------------

def _coupled_run(snow, nsteps=200, dt=600.0, depth=10.0):
    st = T.closure_state(partial=True, snow=snow, melting=False)
    n = st["h"].size
    rng = np.random.default_rng(21)
    Sb = 0.0         # (the reference's test: fresh water, so that the latent heat at Tb is L0 and E = -aice L0 (rho h + rho_s hs) is the energy)
    Tf = T.PHASE["liq_T0"] - T.PHASE["liq_slope"] * Sb
    ocean = dict(To=Tf + np.where(np.arange(n) % 2 == 0, 0.05 * rng.random(n), 0.0))      # half the cells start above freezing
    K = 1e-3 * 1.225 * 1004 * 5
    seen = dict(frazil=0, melt=0, out=0, Qb=[])

    def step(s, top, bottom, Ps):
        o = M.step(ocean["To"], s["a"], dt, depth, K=K, Ta=st["Ta"], Qd=2.0, Sb=Sb)
        ocean["To"] = o["To"]
        seen["frazil"] += int((o["Qfr"] < 0).sum())
        seen["melt"] += int((o["Qio"] > 0).sum())
        if snow:
            r = T.layered_step(s["h"], s["a"], s["hs"], s["Tu"], dt, top, [o["Qb"]], Ps, S=Sb)
            r["Tu"] = r["tu_snow"]
        else:
            r = T.slab_step(s["h"], s["a"], s["Tu"], dt, top, [o["Qb"]], S=Sb)
            r.update(hs=np.zeros_like(s["h"]), mf_int=np.zeros_like(s["h"]))
        assert np.array_equal(r["q_bottom"], o["Qb"])
        seen["out"] += int(((r["h"] <= 0) | (r["aice"] <= 0)).sum())
        return r
    worst = T.closure_run(st, snow, False, nsteps, dt=dt, K=K, step=step)
    return worst, seen


@pytest.mark.parametrize("snow", [False, True])
def test_coupled_energy_closure(snow):
    """The ice's energy closes against the fluxes the step used when the bottom flux is the mixed layer's Qb (LinearHeatFlux top,
    partial concentrations: the reference's bound at aice < 1, 1e-13).  No cell melts out -- asserted first, so no cell is excluded.
    Measured: 6.0e-16 (bare ice), 5.9e-16 (snow)."""
    worst, seen = _coupled_run(snow)
    assert seen["out"] == 0, "a cell melted out: the closure would have to exclude it"
    assert seen["frazil"] > 0 and seen["melt"] > 0
    print(f"coupled closure snow={snow}: {worst.max():.2e}")
    assert worst.max() < 1e-13


# ---- the kernel's generated code (the build keeps the compiler's resource-usage remarks beside the object) ------------------------------

def test_kernel_has_sixteen_instantiations_without_scratch_or_spills():
    """csrc/mixed_layer.res: 16 instantiations of k_mixed_layer (surface array x bulk arrays x deep array x per-cell salinity), none
    with scratch, spilled registers or LDS.  Recorded: 44 VGPRs (numbers only) ... 78 (every array), 6-8 waves per SIMD."""
    csrc = os.path.join(ROOT, "climaseaice.jl_amd", "csrc")
    subprocess.check_call(["make", "-s", "-j8", "-C", csrc], stdout=subprocess.DEVNULL)      # (no-op when the library is up to date)
    blocks = open(os.path.join(csrc, "mixed_layer.res")).read().split("remark: Function Name: ")[1:]
    names = [b.split()[0] for b in blocks]
    assert len(names) == 16 and len(set(names)) == 16 and all("k_mixed_layer" in n for n in names)
    for b in blocks:
        g = lambda k: int(re.search(k + r"[^:]*: (\d+)", b).group(1))
        assert g("ScratchSize") == 0 and g("VGPRs Spill") == 0 and g("SGPRs Spill") == 0 and g("LDS Size") == 0, b.split()[0]
        assert g(r"    VGPRs") <= 96 and g("Occupancy") >= 5, b.split()[0]


# ---- layouts ------------------------------------------------------------------------------------------------------------------------

def _c_layout(tmp_path):
    exe = str(tmp_path / "mixed_layer_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "mixed_layer_layout.c"), "-o", exe])
    return json.loads(subprocess.check_output([exe]).decode())


FLAGS = ("CSI_ML_SURFACE_ARRAY", "CSI_ML_BULK_ARRAYS", "CSI_ML_DEEP_ARRAY", "CSI_ML_HAS_SURFACE", "CSI_ML_HAS_BULK")


def test_c_layout_matches_ctypes(tmp_path):
    got = _c_layout(tmp_path)
    assert got["sizeof_params"] == C.sizeof(L.MixedLayerParams) == 72
    for name, _ in L.MixedLayerParams._fields_:
        assert got[f"csi_mixed_layer_params.{name}"] == getattr(L.MixedLayerParams, name).offset, name
    assert tuple(got[f] for f in FLAGS) == (L.ML_SURFACE_ARRAY, L.ML_BULK_ARRAYS, L.ML_DEEP_ARRAY, L.ML_HAS_SURFACE, L.ML_HAS_BULK) == \
        (1, 2, 4, 8, 16)
    # every older id and count keeps its value; the seven new slots follow
    assert (got["CSI_F_COUNT"], got["CSI_F_COUNT_ALL"], got["CSI_F_COUNT_TOTAL"], got["CSI_F_COUNT_DERIVED"], got["CSI_F_COUNT_BINDABLE"],
            got["CSI_F_COUNT_THERMO"]) == (36, 39, 41, 48, 58, 63) and L.F_COUNT_THERMO == 63 and got["CSI_VERSION"] == 100
    for k, n in enumerate(L.MIXED_LAYER_FIELD_IDS):
        assert got["CSI_F_" + n] == L.F_MIXED_LAYER[n] == L.slot_id(n) == 63 + k
    assert got["CSI_F_COUNT_MIXED_LAYER"] == L.F_COUNT_MIXED_LAYER == 70
    assert len(L.SERIES_SLOTS) + len(L.THERMO_SERIES_SLOTS) + len(L.MIXED_LAYER_SERIES_SLOTS) == 18
    assert all(s in L.F_MIXED_LAYER for s in L.MIXED_LAYER_SERIES_SLOTS)
    assert all(s in L.SYMBOLS for s in ("csi_mixed_layer_set", "csi_mixed_layer_step", "csi_mixed_layer_stats"))


def test_c_layout_matches_julia_stub(tmp_path):
    got = _c_layout(tmp_path)
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    m = re.search(r"^const MIXED_LAYER = \((.*?)\)", stub, re.S | re.M)
    assert m, "const MIXED_LAYER is missing from the Julia stub"
    slots = {k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)", m.group(1))}
    assert slots == {n: got["CSI_F_" + n] for n in L.MIXED_LAYER_FIELD_IDS}
    for name in FLAGS:
        m = re.search(r"^const %s = (\d+)" % name, stub, re.M)
        assert m and int(m.group(1)) == got[name], name
    # struct CsiMixedLayerParams laid out by C's rules
    m = re.search(r"^struct\s+CsiMixedLayerParams\b[^\n]*\n(.*?)\nend", stub, re.S | re.M)
    assert m, "struct CsiMixedLayerParams is missing from the Julia stub"
    fields = re.findall(r"([A-Za-z_]\w*)::(\w+)", re.sub(r"#[^\n]*", "", m.group(1)))
    size_of = {"Cdouble": 8, "Float64": 8, "Int32": 4, "Cint": 4}
    off, offsets = 0, {}
    for name, t in fields:
        off = (off + size_of[t] - 1) // size_of[t] * size_of[t]
        offsets[name] = off
        off += size_of[t]
    assert offsets == {n: got[f"csi_mixed_layer_params.{n}"] for n, _ in L.MixedLayerParams._fields_} and (off + 7) // 8 * 8 == got["sizeof_params"]
    for fn in ("csi_mixed_layer_set", "csi_mixed_layer_step", "csi_mixed_layer_stats"):
        assert re.search(r"ccall\(\(:%s, " % fn, stub), fn
    assert "function attach_mixed_layer!" in stub
    assert re.search(r"CsiMixedLayerParams[^\n]*72", stub), "the static check does not carry the struct's size"


def test_header_is_the_definition():
    text = open(os.path.join(ROOT, "include", "csi.h"), encoding="utf-8").read()
    for words in ("C   = (rho * c) * depth", "Qs  = Fo + (K * (To - Ta))", "Qow = Qs * (1 - a)",
                  "Qio = dT > 0 ? min(((gamma * (rho * c)) * dT) * a, (C * dT) / dt) : 0", "T1  = To + (dt * ((Qd - Qow) - Qio)) / C",
                  "Qfr = T1 < Tf ? (C * (T1 - Tf)) / dt : 0", "To' = T1 < Tf ? Tf : T1", "Qb  = Qio + Qfr",
                  "CSI_F_ML_TEMPERATURE = CSI_F_COUNT_THERMO", "is lost where ice_volume_update clips", "11/6"):
        assert words in text, words


# ---- front end ------------------------------------------------------------------------------------------------------------------------

def grid():
    return csi.RectilinearGrid((4, 3), x=(0, 1), y=(0, 1), halo=(3, 3))


def series(g, nt=3):
    return csi.FieldTimeSeries(g, (csi.Center, csi.Center), np.arange(nt) * 10.0, np.zeros((nt, g.Ny, g.Nx)))


@pytest.mark.parametrize("make, err, words", [
    (lambda: dict(ocean=csi.SlabOceanMixedLayer(10.0), bottom_heat_flux=2.0), ValueError, "bottom_heat_flux is given beside ocean"),
    (lambda: dict(ocean=csi.SlabOceanMixedLayer(10.0), ice_thermodynamics=csi.SlabThermodynamics(bottom_heat_flux=np.zeros((3, 4)))),
     ValueError, "bottom_heat_flux is given beside ocean"),
    (lambda: dict(ocean=csi.SlabOceanMixedLayer(10.0), bottom_heat_flux="frazil"), ValueError, '"frazil" beside ocean'),
    (lambda: dict(ocean=csi.SlabOceanMixedLayer(10.0), ice_thermodynamics=None), ValueError, "needs ice_thermodynamics"),
    (lambda: dict(ocean=lambda i, j, grid, clock, fields: 0.0), TypeError, "a SlabOceanMixedLayer is needed.*closures"),
    (lambda: dict(ocean=csi.SlabOceanMixedLayer(10.0, surface_heat_flux=np.zeros((4, 4)))), ValueError, "SlabOceanMixedLayer.surface_heat_flux"),
    (lambda: dict(ocean=csi.SlabOceanMixedLayer(10.0, coefficient=np.zeros(5), atmosphere_temperature=0.0)), ValueError,
     "SlabOceanMixedLayer.coefficient"),
    (lambda: dict(ocean=csi.SlabOceanMixedLayer(10.0, temperature=np.zeros((2, 2)))), ValueError, "SlabOceanMixedLayer.temperature"),
])
def test_model_refusals_by_name(make, err, words):
    kw = dict(ice_thermodynamics=csi.SlabThermodynamics())
    kw.update(make())
    with pytest.raises(err, match=words):
        csi.SeaIceModel(grid(), **kw)


@pytest.mark.parametrize("kw, err, words", [
    (dict(depth=0.0), ValueError, "depth must be > 0"),
    (dict(depth=10.0, density=-1.0), ValueError, "density must be > 0"),
    (dict(depth=10.0, heat_capacity=0.0), ValueError, "heat_capacity must be > 0"),
    (dict(depth=float("nan")), ValueError, "depth: a finite number"),
    (dict(depth=10.0, ice_ocean_exchange_velocity=-1e-5), ValueError, "ice_ocean_exchange_velocity must be >= 0"),
    (dict(depth=10.0, deep_heat_flux=float("inf")), ValueError, "deep_heat_flux is not finite"),
    (dict(depth=10.0, coefficient=3.0), ValueError, "coefficient and atmosphere_temperature are given together"),
    (dict(depth=10.0, atmosphere_temperature=-5.0), ValueError, "coefficient and atmosphere_temperature are given together"),
    (dict(depth=10.0, surface_heat_flux=lambda i, j, grid, clock, fields: 0.0), NotImplementedError, "FluxFunction and other callables"),
    (dict(depth=10.0, deep_heat_flux="warm"), TypeError, "SlabOceanMixedLayer.deep_heat_flux"),
    (dict(depth=10.0, temperature=lambda x: x), ValueError, "SlabOceanMixedLayer.temperature"),
])
def test_layer_refusals_by_name(kw, err, words):
    with pytest.raises(err, match=words):
        csi.SlabOceanMixedLayer(**kw)


def test_flags_params_and_series_slots():
    g = grid()
    o = csi.SlabOceanMixedLayer(10.0)
    p = o.params()
    assert (p.density, p.heat_capacity, p.depth, p.exchange_velocity, p.flags, p.reserved) == (1026.0, 3991.0, 10.0, 6e-5, 0, 0)
    o = csi.SlabOceanMixedLayer(25.0, surface_heat_flux=-3.0, coefficient=6.5, atmosphere_temperature=-12.0, deep_heat_flux=2.0,
                                ice_ocean_exchange_velocity=0.0)
    p = o.params()
    assert p.flags == L.ML_HAS_SURFACE | L.ML_HAS_BULK and o.array_inputs() == []
    assert (p.surface_heat_flux, p.coefficient, p.reference_temperature, p.deep_heat_flux, p.exchange_velocity) == (-3.0, 6.5, -12.0, 2.0, 0.0)
    # one of the bulk pair per cell: both travel as arrays, the number is broadcast
    o = csi.SlabOceanMixedLayer(10.0, coefficient=6.5, atmosphere_temperature=np.zeros((3, 4)))
    assert o.flags() == L.ML_HAS_BULK | L.ML_BULK_ARRAYS and [s for _, s, _ in o.array_inputs()] == ["ML_COEFFICIENT", "ML_REFERENCE_TEMPERATURE"]
    assert o.params().coefficient == 0.0
    # what bulk_sensible_heat_flux returns carries K and Ta
    o = csi.SlabOceanMixedLayer(10.0, coefficient=csi.bulk_sensible_heat_flux(1e-3, 1.225, 1004, 5, -7.0))
    assert o.inputs["coefficient"] == 1e-3 * 1.225 * 1004 * 5 and o.inputs["atmosphere_temperature"] == -7.0
    # the four series slots, in the model's one table of series-driven per-cell inputs
    o = csi.SlabOceanMixedLayer(10.0, surface_heat_flux=series(g), coefficient=series(g), atmosphere_temperature=series(g),
                                deep_heat_flux=series(g))
    assert o.flags() == L.ML_HAS_SURFACE | L.ML_SURFACE_ARRAY | L.ML_HAS_BULK | L.ML_BULK_ARRAYS | L.ML_DEEP_ARRAY
    assert o.series_slots() == L.MIXED_LAYER_SERIES_SLOTS
    from climaseaice_jl_amd import model as model_module
    from climaseaice_jl_amd.ocean import INPUT_SLOTS
    table = model_module._SERIES_SLOT_OF
    assert [table[INPUT_SLOTS[n][1]] for n in ("surface_heat_flux", "coefficient", "atmosphere_temperature", "deep_heat_flux")] == \
        L.MIXED_LAYER_SERIES_SLOTS
    assert sorted(table.values()) == sorted(L.SERIES_SLOTS[8:] + L.THERMO_SERIES_SLOTS + L.MIXED_LAYER_SERIES_SLOTS)
    o.check(g, model_module._cell_shape_ok)
    with pytest.raises(ValueError, match="surface_flux_used needs a model"):
        o.surface_flux_used


def test_writer_takes_the_ocean_fields_by_name(tmp_path):
    """OutputWriter(model, ["ocean.temperature", "ocean.surface_flux_used"], ...): the second is allocated the first time it is asked
    for -- by the writer, before it looks the names up -- on the stand-in recorder."""
    g = csi.RectilinearGrid((8, 6), x=(0, 8), y=(0, 6), topology=(csi.Bounded, csi.Bounded), halo=(2, 2))
    fields = OrderedDict()
    fields["ocean.temperature"] = csi.CenterField(g, None, "ocean_temperature")
    fields["ocean.temperature"].data.fill_(-1.5)
    asked = []

    class Ocean:
        @property
        def surface_flux_used(self):
            asked.append(1)
            if "ocean.surface_flux_used" not in fields:
                fields["ocean.surface_flux_used"] = csi.CenterField(g, None, "ocean_surface_flux_used")
                fields["ocean.surface_flux_used"].data.fill_(7.0)
            return fields["ocean.surface_flux_used"]
    m = SimpleNamespace(grid=g, clock=SimpleNamespace(time=0.0, iteration=0), fields=fields, output_writers=OrderedDict(), ocean=Ocean())
    with pytest.raises(ValueError, match="'ocean.surface_flux_used' is not a field the model has bound"):
        csi.OutputWriter(SimpleNamespace(grid=g, clock=m.clock, fields=fields, output_writers=OrderedDict()),
                         ["ocean.surface_flux_used"], csi.IterationInterval(1), str(tmp_path / "none"), recorder=output_ref.RefRecorder)
    w = csi.OutputWriter(m, ["ocean.temperature", "ocean.surface_flux_used"], csi.IterationInterval(1), str(tmp_path / "o"), dtype="f64",
                         recorder=output_ref.RefRecorder)
    assert asked and w.names == ["ocean.temperature", "ocean.surface_flux_used"]
    w.write(m)
    w.close()
    out = csi.load_output(str(tmp_path / "o"))
    assert np.all(out["ocean.temperature"][0] == -1.5) and np.all(out["ocean.surface_flux_used"][0] == 7.0)
