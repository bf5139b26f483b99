"""Every instantiation of the flux-term kernels k_slab_flux / k_layered_flux (csrc/thermo_flux.hip) a configuration can select -- 864,
the 432 flux-balance-capable ones under both boundary conditions: 1296 cases of tests/thermo_flux_matrix.py -- on the GPU against the
NumPy restatement tests/thermo_shortwave_ref.py, bit for bit.  Each case asserts the kernel the library reports (csi_last_thermo)
against thermo_flux_matrix.expected_key before a number is compared.  One test per (step, shortwave, LIN, SB) group, looping over its
16 / 32 flux_bits values and both boundary conditions; FAST mode, one key per (step, shortwave) again in STRICT (the thermodynamics
is one code in both).  One 65 x 5 grid with halo 3 (both last blocks of the 64 x 4 block partial): the flags do not interact with the
shape, and test_gpu_heat_fluxes.py, test_gpu_thermo_linear.py and test_gpu_thermo_shortwave.py walk the shapes.

The configurations are set through the C ABI on one context (csi_heat_fluxes_set, csi_surface_solve_set, csi_shortwave_set,
csi_slab_thermo_step / csi_layered_thermo_step): the front end cannot express a bare number term beside nothing or a prescribed number
beside a shortwave term.  Every array slot stays bound throughout, so no kernel -- not even a wrongly selected one -- reads an unbound
array; the halos and the outputs hold NaN before every case."""
import ctypes as C

import numpy as np
import pytest
import torch

import climaseaice_jl_amd as csi
import thermo_flux_matrix as M
import thermo_shortwave_ref as S
from test_gpu_thermo_shortwave import SNOW_PAIR

pytestmark = pytest.mark.gpu

L = csi._lib
DEV = "cuda:0"
# the slots the steps update or write (reset before every case), then the inputs (written once)
STATE = ["H", "A", "HS", "TU", "TUS", "MASS_FLUX", "MASS_FLUX_SNOW", "SNOWFALL_INTERCEPTED", "TOP_HEAT_FLUX_USED", "BOTTOM_HEAT_FLUX_USED",
         "ALBEDO_USED"]
INPUTS = dict(BOTTOM_HEAT_FLUX="qb", SNOWFALL="ps", FLUX_COEFFICIENT="K", FLUX_REFERENCE_TEMPERATURE="Ta", BOTTOM_SALINITY="S", SHORTWAVE="F")
USED = ("TOP_HEAT_FLUX_USED", "BOTTOM_HEAT_FLUX_USED")
# restatement name -> slot, per step
SLAB_OUT = dict(h="H", aice="A", Tu="TU", mf="MASS_FLUX", q_top="TOP_HEAT_FLUX_USED", q_bottom="BOTTOM_HEAT_FLUX_USED", albedo="ALBEDO_USED")
LAYERED_OUT = dict(h="H", aice="A", hs="HS", tu_ice="TU", tu_snow="TUS", mf_ice="MASS_FLUX", mf_snow="MASS_FLUX_SNOW",
                   mf_int="SNOWFALL_INTERCEPTED", q_top="TOP_HEAT_FLUX_USED", q_bottom="BOTTOM_HEAT_FLUX_USED", albedo="ALBEDO_USED")
WEIGHT = {None: L.WEIGHT_NONE, "concentration": L.WEIGHT_CONCENTRATION, "ice_present": L.WEIGHT_ICE_PRESENT}


class Raw:
    """One context with the 65 x 5 grid and every slot of the thermodynamics bound to a plane of one tensor, without a model."""

    def __init__(self):
        self.ctx = L.Context(0)
        self.st = st = M.matrix_state()
        Nx, Ny, H = M.NX, M.NY, M.HALO
        self.ni, self.nj = Nx + 2 * H, Ny + 2 * H
        met = L.Metrics()
        met.dx = met.dy = 1000.0
        self.ctx.call("csi_grid_set", Nx, Ny, H, H, L.PERIODIC, L.PERIODIC, L.METRIC_UNIFORM, C.byref(met))
        self.inner = (slice(H, H + Ny), slice(H, H + Nx))

        def planes(arrays):
            full = np.full((len(arrays), self.nj, self.ni), np.nan)
            for k, x in enumerate(arrays):
                if x is not None:
                    full[(k,) + self.inner] = x
            return torch.from_numpy(full).to(DEV)

        # the state every case starts from (NaN in the halos and in the outputs), and the tensor the slots are bound to
        self.init = planes([st["h"], st["a"], st["hs"]] + [None] * (len(STATE) - 3))
        self.state = self.init.clone()
        self.inputs = planes([st[v] for v in INPUTS.values()])
        self.qtop = {off: planes([st["qt"] + off])[0] for off in (0.0, -200.0)}
        self.start = {k: planes([v])[0] for k, v in (("tu0", st["tu0"]), ("tp", st["tp"]), ("number", np.full((Ny, Nx), M.TP0)))}
        for k, name in enumerate(STATE):
            self.bind(name, self.state[k])
        for k, name in enumerate(INPUTS):
            self.bind(name, self.inputs[k])
        self.bind("TOP_HEAT_FLUX", self.qtop[0.0])
        torch.cuda.synchronize()

    def bind(self, name, plane):
        self.ctx.call("csi_field_bind", L.slot_id(name), C.c_void_p(plane.data_ptr()) if plane is not None else None, self.ni, self.ni, self.nj)

    def configure(self, cfg, mode):
        """The configuration through the C ABI: the mode, the shortwave setting, both tuples, the per-cell flags; returns the step call."""
        ctx = self.ctx
        ctx.call("csi_set_mode", L.MODE_STRICT if mode == "strict" else L.MODE_FAST)
        for name in USED:
            self.bind(name, self.state[STATE.index(name)] if cfg["used"] else None)
        if M.has(cfg["top"], "shortwave"):
            per_cell, weighting, pair = cfg["shortwave"]
            snow = SNOW_PAIR if pair else (0.0, 0.0, 0.0)
            ctx.call("csi_shortwave_set", C.byref(L.Shortwave(M.F0, *S.SEMTNER, *snow, WEIGHT[weighting], int(per_cell), int(pair), 0)))
        else:
            ctx.call("csi_shortwave_set", None)
        for side, code in (("top", L.HEAT_TOP), ("bottom", L.HEAT_BOTTOM)):
            terms = []
            for t in cfg[side]:
                if t[0] == "emission":
                    terms.append(L.HeatFluxTerm(L.FLUX_RADIATIVE_EMISSION, 0, M.EMISSION_VALUE, 1.0, 5.67e-8, 273.15))
                elif t[0] == "linear":
                    flags = WEIGHT[t[2]] | ((L.LINEAR_COEFFICIENT_ARRAY | L.LINEAR_REFERENCE_ARRAY) if t[1] else 0)
                    terms.append(L.HeatFluxTerm(L.FLUX_LINEAR, flags, M.K0, 0.0, 0.0, M.TA0))
                elif t[0] == "shortwave":
                    terms.append(L.HeatFluxTerm(L.FLUX_SHORTWAVE, 0, M.SHORTWAVE_VALUE, 0.0, 0.0, 0.0))
                elif t[0] == "array":
                    terms.append(L.HeatFluxTerm(L.FLUX_ARRAY, 0, 0.0, 0.0, 0.0, 0.0))
                    if side == "top":
                        self.bind("TOP_HEAT_FLUX", self.qtop[t[1]])
                    else:
                        assert t[1] == 0.0
                else:
                    terms.append(L.HeatFluxTerm(L.FLUX_CONSTANT, 0, float(t[1]), 0.0, 0.0, 0.0))
            ctx.call("csi_heat_fluxes_set", code, (L.HeatFluxTerm * len(terms))(*terms) if terms else None, len(terms))
        ctx.call("csi_surface_solve_set", C.byref(L.SurfaceSolve(1e-3, M.MAXITERS, int(cfg["prescribed_array"]), int(cfg["snowfall_array"]),
                                                                 L.SOLVE_BOTTOM_SALINITY_ARRAY if cfg["salinity_array"] else 0)))
        snow, balance = cfg["snow"], cfg["balance"]
        slab = L.SlabParams(2.0, 900.0, 917.0, 999.8, 4186.0, 2000.0, 334e3, 0.0, 0.054, 0.0, M.S0, 0.05, M.TP0, 0, cfg["bottom_flux_kind"],
                            cfg["Qu"], cfg["Qb"], 1 if (snow or balance) else 0, 0, 0.0)
        if snow:
            snowp = L.SnowParams(0.31, 330.0, M.PS0, M.TP0, 1 if balance else 0, 0)
            return lambda: ctx.call("csi_layered_thermo_step", C.byref(slab), C.byref(snowp), M.DT)
        return lambda: ctx.call("csi_slab_thermo_step", C.byref(slab), M.DT)

    def run(self, cfg, mode="fast"):
        """The state reset, the configuration set, nsteps_of(cfg) steps: (what csi_last_thermo reports, {slot: interior})."""
        self.ctx.call("csi_sync")
        self.state.copy_(self.init)
        start = "tu0" if cfg["balance"] else ("tp" if cfg["prescribed_array"] else "number")
        self.state[STATE.index("TUS" if cfg["snow"] else "TU")].copy_(self.start[start])
        torch.cuda.synchronize()
        step = self.configure(cfg, mode)
        for n in range(M.nsteps_of(cfg)):
            step()
        self.ctx.call("csi_sync")
        last = self.ctx.last_thermo()
        got = self.state.cpu().numpy()
        return (last["step"], last["shortwave"], last["index"]), {name: got[(k,) + self.inner] for k, name in enumerate(STATE)}


@pytest.fixture(scope="module")
def raw():
    r = Raw()
    yield r
    r.ctx.close()


def check(raw, cid, cfg, mode="fast", names=None):
    """One case: the reported kernel first, then every compared output bit for bit against the restatement."""
    its = []
    want = M.reference(cfg, raw.st, mode_iterations=its)
    assert max(its) < M.MAXITERS, (cid, "the restatement's secant reached maxiters")
    key, got = raw.run(cfg, mode)
    assert key == M.expected_key(cfg), (cid, mode, key, M.expected_key(cfg))
    slots = LAYERED_OUT if cfg["snow"] else SLAB_OUT
    for k in (names or M.compared(cfg)):
        x, y = got[slots[k]], want[k]
        assert np.all(np.isfinite(y)), (cid, k)
        assert np.array_equal(x, y), (cid, mode, k, int((x != y).sum()), float(np.nanmax(np.abs(x - y))))
    return want


@pytest.mark.parametrize("group", M.GROUPS, ids=lambda g: "%s-sw%d-lin%d-sb%d" % ("slab" if g[0] == M.K_SLAB_FLUX else "layered", g[1], g[2], g[3]))
def test_every_instantiation_matches_the_restatement(raw, group):
    cases = M.cases_of(group)
    assert len(cases) == M.STRIDE[group[0]] * 3 // 2
    moved = 0.0
    for cid, key, cfg in cases:
        assert M.expected_key(cfg) == key
        want = check(raw, cid, cfg)
        moved = max(moved, np.abs(want["h"] - raw.st["h"]).max())
    assert moved > 1e-5


@pytest.mark.parametrize("sw", [0, 1, 2])
@pytest.mark.parametrize("step", [M.K_SLAB_FLUX, M.K_LAYERED_FLUX], ids=["slab", "layered"])
def test_one_key_of_each_family_in_strict(raw, step, sw):
    """The key with every flag on (LIN per cell, SB), prescribed and under the flux balance, in STRICT mode."""
    key = (step, sw, M.TABLE[step] - 1)
    cases = [c for c in M.CASES if c[1] == key]
    assert [c[2]["balance"] for c in cases] == [False, True]
    for cid, _, cfg in cases:
        check(raw, cid, cfg, mode="strict")


@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_frazil_bottom_flux_in_the_flux_kernels(raw, snow):
    """bottom_flux_kind 1 -- Qb = -(1 - aice) * Qb -- with no bottom terms reaches the flux kernels through the per-cell salinity (no top
    terms either: the top takes csi_slab_params' number), through the bound used-flux outputs, and beside a shortwave term, where the
    bottom's flux is formed before the secant loop."""
    base = dict(snow=snow, balance=True, top=(), bottom=(), shortwave=None, prescribed_array=False, snowfall_array=False, salinity_array=False,
                used=False, bottom_flux_kind=1, Qu=-30.0, Qb=2.5)
    stride = M.STRIDE[M.K_LAYERED_FLUX if snow else M.K_SLAB_FLUX]
    step = M.K_LAYERED_FLUX if snow else M.K_SLAB_FLUX
    term = (("shortwave",), ("number", 40.0))
    variants = (("salinity", dict(base, salinity_array=True), (step, 0, 3 * stride)),
                ("used", dict(base, used=True), (step, 0, 0)),
                ("number", dict(base, used=True, top=term, shortwave=(False, "concentration", snow)), (step, 1, M.BIT_LTU)),
                ("cell", dict(base, used=True, top=term, shortwave=(True, None, False), salinity_array=True), (step, 2, M.BIT_LTU + 3 * stride)),
                ("cell prescribed", dict(base, balance=False, used=True, top=term, shortwave=(True, "ice_present", snow)), (step, 2, 0)))
    for what, cfg, key in variants:
        assert M.expected_key(cfg) == key, what
        names = [k for k in M.compared(cfg) if cfg["used"] or k not in ("q_top", "q_bottom")]
        want = check(raw, ("frazil", what), cfg, names=names)
        if cfg["used"]:
            assert np.array_equal(want["q_bottom"], (-(1 - raw.st["a"])) * 2.5) and np.unique(want["q_bottom"]).size > 10


@pytest.mark.parametrize("snow", [False, True], ids=["slab", "layered"])
def test_nothing_triggers_the_flux_path(raw, snow):
    """No terms, no per-cell flag, the used-flux outputs unbound: the numeric kernels run (index -1) and give the restatement's bits."""
    for balance in (True, False):
        cfg = dict(snow=snow, balance=balance, top=(), bottom=(), shortwave=None, prescribed_array=False, snowfall_array=False,
                   salinity_array=False, used=False, bottom_flux_kind=0, Qu=-30.0, Qb=2.0)
        assert M.expected_key(cfg) == (M.K_LAYERED if snow else M.K_SLAB, 0, -1)
        names = ["h", "aice", "hs", "mf_ice", "mf_snow", "mf_int", "tu_ice", "tu_snow"] if snow else ["h", "aice", "mf"]
        check(raw, ("numeric", balance), cfg, names=names)
    # ... and binding the outputs alone selects the flux kernels again
    key, _ = raw.run(dict(cfg, used=True))
    assert key == (M.K_LAYERED_FLUX if snow else M.K_SLAB_FLUX, 0, 0)


def test_nothing_launched_yet():
    ctx = L.Context(0)
    assert ctx.last_thermo() == dict(step=0, shortwave=0, index=-1)
    ctx.close()
