"""Which instantiation of the flux-term kernels k_slab_flux / k_layered_flux (csrc/thermo_flux.hip) a configuration selects, stated
once, and the case table of tests/test_gpu_thermo_flux_matrix.py.

The host (csrc/csi_thermo.hip, the launch functions of thermo_flux.hip) picks one of 864 kernels: 96 of k_slab_flux and 192 of
k_layered_flux in each of three tables (the SHORTWAVE term absent / its flux a number / per cell), by

    flux_bits = QT | QB << 1 | EMIT << 2 | LTU << 3
    slab      b = flux_bits             + 16 * (LIN + 3 * SB)
    layered   b = (flux_bits | PS << 4) + 32 * (LIN + 3 * SB)

QT / QB: the top / bottom has an ARRAY term; EMIT: the top has a RadiativeEmission term; LTU: the cell's surface temperature is read
(per-cell PrescribedTemperature, or Tu- of the secant under a flux balance with a term that depends on T); PS: per-cell snowfall; LIN:
the LINEAR term absent / numbers / per cell; SB: per-cell bottom salinity.  `expected_key` mirrors flux_path, flux_bits,
flux_reads_surface_temperature and flux_variant; `flags_of` is its inverse; tests/test_thermo_flux_matrix_table.py holds the numbers
against the source text and proves the table complete, and every GPU case asserts what the library reports (csi_last_thermo) against
`expected_key` before a number is compared.

A configuration is a dict of plain values, so that the restatement (here, `reference`) and the C ABI (the GPU file) read the same one:
  snow, balance                       the layered step; MeltingConstrainedFluxBalance (PrescribedTemperature otherwise)
  top, bottom                         tuples of terms: ("emission",) ("linear", per_cell, weighting) ("shortwave",) ("array", offset)
                                      ("number", value); the ARRAY term's field is the state's qt / qb + offset
  shortwave                           None or (per_cell, weighting, snow_pair): the setting of csi_shortwave_set
  prescribed_array, snowfall_array, salinity_array, used
                                      the per-cell flags of csi_surface_solve_set; used: the used-flux outputs are bound
  bottom_flux_kind, Qu, Qb            csi_slab_params: the numbers a side without terms takes (bottom_flux_kind 1: the frazil form)
"""
import numpy as np

import thermo_flux_ref as R
import thermo_linear_ref as T
import thermo_shortwave_ref as S
from test_gpu_thermo_shortwave import SNOW_PAIR, state

K_SLAB, K_LAYERED, K_SLAB_FLUX, K_LAYERED_FLUX = 1, 2, 3, 4      # csi_last_thermo's step
SW_NONE, SW_NUMBER, SW_CELL = 0, 1, 2
LIN_NONE, LIN_NUMBERS, LIN_ARRAYS = 0, 1, 2
BIT_QT, BIT_QB, BIT_EMIT, BIT_LTU, BIT_PS = 1, 2, 4, 8, 16
STRIDE = {K_SLAB_FLUX: 16, K_LAYERED_FLUX: 32}
VARIANTS = 6                                                     # LIN + 3 * SB
TABLE = {step: s * VARIANTS for step, s in STRIDE.items()}       # 96, 192
WEIGHTINGS = (None, "concentration", "ice_present")

NX, NY, HALO, SEED = 65, 5, 3, 2
DT = 600.0
MAXITERS = 1000
# the numbers a kernel LACKING a flag reads in place of the array: each differs from every cell of the state (asserted by the table test)
S0, PS0, F0, K0, TA0, TP0 = 30.0, 2e-5, -187.5, 17.5, -1.25, -0.07
EMISSION_VALUE, SHORTWAVE_VALUE = -3.0, -5.0      # the `value` field of the two terms that do not read it


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def has(terms, kind):
    return any(t[0] == kind for t in terms)


def shortwave_mode(cfg):
    """the SHORTWAVE term's setting as the kernels take it: SW_NONE unless the top's tuple has the term (flux_fields)"""
    if not has(cfg["top"], "shortwave"):
        return SW_NONE
    return SW_CELL if cfg["shortwave"][0] else SW_NUMBER


def linear_state(cfg):
    for t in cfg["top"]:
        if t[0] == "linear":
            return LIN_ARRAYS if t[1] else LIN_NUMBERS
    return LIN_NONE


def flux_path(cfg):
    return bool(len(cfg["top"]) > 0 or len(cfg["bottom"]) > 0 or cfg["prescribed_array"] or (cfg["snow"] and cfg["snowfall_array"]) or
                cfg["salinity_array"] or cfg["used"])


def reads_surface_temperature(cfg):
    if not cfg["balance"]:
        return bool(cfg["prescribed_array"])
    return has(cfg["top"], "emission") or linear_state(cfg) != LIN_NONE or shortwave_mode(cfg) != SW_NONE


def flux_bits(cfg):
    return ((BIT_QT if has(cfg["top"], "array") else 0) | (BIT_QB if has(cfg["bottom"], "array") else 0) |
            (BIT_EMIT if has(cfg["top"], "emission") else 0) | (BIT_LTU if reads_surface_temperature(cfg) else 0))


def flux_variant(cfg):
    return linear_state(cfg) + 3 * (1 if cfg["salinity_array"] else 0)


def expected_key(cfg):
    """(step, shortwave, index) as csi_last_thermo reports them."""
    if not flux_path(cfg):
        return (K_LAYERED if cfg["snow"] else K_SLAB, SW_NONE, -1)
    if cfg["snow"]:
        b = (flux_bits(cfg) | (BIT_PS if cfg["snowfall_array"] else 0)) + STRIDE[K_LAYERED_FLUX] * flux_variant(cfg)
        return (K_LAYERED_FLUX, shortwave_mode(cfg), b)
    return (K_SLAB_FLUX, shortwave_mode(cfg), flux_bits(cfg) + STRIDE[K_SLAB_FLUX] * flux_variant(cfg))


def flags_of(step, index):
    """The template flags of table entry `index`, as slab_inst<B> / layered_inst<B> decode it."""
    stride = STRIDE[step]
    assert 0 <= index < TABLE[step]
    f = dict(QT=bool(index & BIT_QT), QB=bool(index & BIT_QB), EMIT=bool(index & BIT_EMIT), LTU=bool(index & BIT_LTU),
             LIN=(index // stride) % 3, SB=(index // (3 * stride)) != 0)
    if step == K_LAYERED_FLUX:
        f["PS"] = bool(index & BIT_PS)
    return f


def all_keys():
    return [(step, sw, b) for step in (K_SLAB_FLUX, K_LAYERED_FLUX) for sw in (SW_NONE, SW_NUMBER, SW_CELL) for b in range(TABLE[step])]


def balance_capable(key):
    """Under the flux balance the host sets LTU exactly when the top has a term that depends on T."""
    f = flags_of(key[0], key[2])
    return f["LTU"] == (f["EMIT"] or f["LIN"] != LIN_NONE or key[1] != SW_NONE)


# ---- the case table ----------------------------------------------------------------------------------------------------------------
def configuration(key, balance, lin_weight=None, sw_weight=None, snow_pair=False):
    """A configuration that selects `key`.  The top tuple in the fixed order emission, linear, shortwave, array, number; the number
    is always there (n >= 1 for key 0).  Prescribed: the temperature per cell when LTU, a number otherwise."""
    step, sw, index = key
    f = flags_of(step, index)
    assert not balance or balance_capable(key), key
    top = []
    if f["EMIT"]:
        top.append(("emission",))
    if f["LIN"] != LIN_NONE:
        top.append(("linear", f["LIN"] == LIN_ARRAYS, lin_weight))
    if sw != SW_NONE:
        top.append(("shortwave",))
    if f["QT"]:
        top.append(("array", -200.0 if f["EMIT"] else 0.0))
    top.append(("number", (-50.0 if f["QT"] else -210.0) if f["EMIT"] else 40.0))
    bottom = [("array", 0.0), ("number", 1.5)] if f["QB"] else [("number", 2.5)]
    snow = step == K_LAYERED_FLUX
    return dict(snow=snow, balance=balance, top=tuple(top), bottom=tuple(bottom),
                shortwave=None if sw == SW_NONE else (sw == SW_CELL, sw_weight, bool(snow and snow_pair)),
                prescribed_array=bool(f["LTU"] and not balance), snowfall_array=bool(snow and f["PS"]), salinity_array=f["SB"],
                used=True, bottom_flux_kind=0, Qu=0.0, Qb=0.0)


def build_cases():
    """[(id, key, cfg)]: one prescribed case per key and a flux-balance case for each balance-capable one; the weightings of the linear
    and of the shortwave term taken in turn (the second three times slower, so that every pair occurs), the snow pair on every other
    layered case with the term."""
    out = []
    n_lin = n_sw = n_pair = 0
    for key in all_keys():
        step, sw, index = key
        f = flags_of(step, index)
        for balance in (False, True):
            if balance and not balance_capable(key):
                continue
            lw = sww = None
            pair = False
            if f["LIN"] != LIN_NONE:
                lw = WEIGHTINGS[n_lin % 3]
                n_lin += 1
            if sw != SW_NONE:
                sww = WEIGHTINGS[(n_sw // 3) % 3]
                n_sw += 1
                if step == K_LAYERED_FLUX:
                    pair = n_pair % 2 == 0
                    n_pair += 1
            out.append(((step, sw, index, "balance" if balance else "prescribed"), key, configuration(key, balance, lw, sww, pair)))
    return out


CASES = build_cases()


def group_of(key):
    """(step, shortwave, LIN, SB): one GPU test each"""
    f = flags_of(key[0], key[2])
    return (key[0], key[1], f["LIN"], int(f["SB"]))


GROUPS = sorted({group_of(key) for _, key, _ in CASES})


def cases_of(group):
    return [c for c in CASES if group_of(c[1]) == group]


# ---- the state and the restatement --------------------------------------------------------------------------------------------------
_STATE = {}


def matrix_state():
    """The shortwave file's state on 65 x 5 (mixed_state plus F and tp) plus a starting Tu- per cell that is nowhere zero.  Shared
    and left unchanged."""
    if not _STATE:
        st = state(NX, NY, SEED)
        rng = np.random.default_rng(SEED + 2000)
        st["tu0"] = -12.0 + 10.0 * rng.random((NY, NX))      # -12 ... -2
        # ... and in one cell of six so close below the albedo's threshold that the secant's two starting points, Tu- + 1 and Tu-, lie
        # on different sides of it: there the root depends on Tu- even where the stepped albedo is the balance's only dependence on T
        near = rng.random((NY, NX)) < 1 / 6
        st["tu0"] = np.where(near, -0.15 - 0.8 * rng.random((NY, NX)), st["tu0"])
        for v in st.values():
            v.setflags(write=False)
        _STATE.update(st)
    return _STATE


def nsteps_of(cfg):
    """Balances with emission or the linear term: two steps, Tu carried.  A balance whose only dependence on T is the stepped albedo
    (two parallel lines with a jump, on which the secant can cycle): one step from tu0.  Everything else: one step."""
    return 2 if cfg["balance"] and (has(cfg["top"], "emission") or linear_state(cfg) != LIN_NONE) else 1


def ref_terms(cfg, st, side, lacking=None):
    """The restatement's terms of a side.  lacking: a flag -- the terms as a kernel WITHOUT it reads them."""
    out = []
    for t in cfg[side]:
        if t[0] == "emission":
            out.append(float(EMISSION_VALUE) if lacking == "EMIT" else R.Emission(1.0, 5.67e-8, 273.15))
        elif t[0] == "linear":
            if lacking == "LIN":
                out.append(T.Linear(K0, TA0, t[2]) if t[1] else float(K0))
            else:
                out.append(T.Linear(st["K"], st["Ta"], t[2]) if t[1] else T.Linear(K0, TA0, t[2]))
        elif t[0] == "shortwave":
            per_cell, weighting, pair = cfg["shortwave"]
            snow_albedo = S.Albedo(*SNOW_PAIR) if pair else None
            if lacking == "SW":              # (the SW_NUMBER kernel reads the setting's number, the SW_NONE kernel the term's value)
                out.append(S.Shortwave(F0, S.SEMTNER, snow_albedo, weighting) if per_cell else float(SHORTWAVE_VALUE))
            elif lacking == "SW0":           # (csi_shortwave_set stores 0 for that number once the flux is per cell)
                out.append(S.Shortwave(0.0, S.SEMTNER, snow_albedo, weighting))
            else:
                out.append(S.Shortwave(st["F"] if per_cell else F0, S.SEMTNER, snow_albedo, weighting))
        elif t[0] == "array":
            q = st["qt" if side == "top" else "qb"] + t[1]
            out.append(0.0 if lacking == ("QT" if side == "top" else "QB") else q)
        else:
            assert t[0] == "number", t
            out.append(float(t[1]))
    if not out:                              # the side takes csi_slab_params' number (the frazil form at the bottom)
        if side == "bottom" and cfg["bottom_flux_kind"] == 1:
            return [(-(1 - st["a"])) * cfg["Qb"]]
        return [float(cfg["Qu" if side == "top" else "Qb"])]
    return out


def start_temperature(cfg, st, lacking=None):
    if cfg["balance"]:
        return np.zeros((NY, NX)) if lacking == "LTU" else st["tu0"].copy()
    return st["tp"].copy() if cfg["prescribed_array"] and lacking != "LTU" else np.full((NY, NX), TP0)


def flags_set(key):
    """The flags of a key that are on, by the names `lacking` takes."""
    f = flags_of(key[0], key[2])
    on = [k for k in ("QT", "QB", "EMIT", "LTU", "PS", "SB") if f.get(k)]
    if f["LIN"] != LIN_NONE:
        on.append("LIN")
    if key[1] != SW_NONE:
        on.append("SW")
    if key[1] == SW_CELL:
        on.append("SW0")
    return on


def reference(cfg, st, lacking=None, mode_iterations=None):
    """The restatement stepped nsteps_of(cfg) times: its last dict (the names of thermo_shortwave_ref).  mode_iterations: a list that
    receives the largest update count of the secant over the consolidated cells, per step."""
    rtop, rbottom = ref_terms(cfg, st, "top", lacking), ref_terms(cfg, st, "bottom", lacking)
    Sb = st["S"] if cfg["salinity_array"] and lacking != "SB" else S0
    Ps = st["ps"] if cfg["snowfall_array"] and lacking != "PS" else PS0
    h, a, hs, Tu = st["h"], st["a"], st["hs"], start_temperature(cfg, st, lacking)
    for n in range(nsteps_of(cfg)):
        its = []
        if cfg["snow"]:
            r = S.layered_step(h, a, hs, Tu, DT, rtop, rbottom, Ps, flux_balance=cfg["balance"], S=Sb, iterations=its)
            h, a, hs, Tu = r["h"], r["aice"], r["hs"], r["tu_snow"]
        else:
            r = S.slab_step(h, a, Tu, DT, rtop, rbottom, flux_balance=cfg["balance"], S=Sb, iterations=its)
            h, a, Tu = r["h"], r["aice"], r["Tu"]
        if mode_iterations is not None:
            mode_iterations.append(max([int(i.max()) for i in its if i.size] + [0]))
    return r


def compared(cfg):
    """The outputs a case compares bit for bit."""
    names = ["h", "aice", "q_top", "q_bottom"] + (["hs", "mf_ice", "mf_snow", "mf_int", "tu_ice", "tu_snow"] if cfg["snow"] else ["Tu", "mf"])
    return names + (["albedo"] if shortwave_mode(cfg) != SW_NONE else [])


def surface(cfg):
    """... and those the sensitivity check looks at: h, aice or a surface temperature."""
    return ["h", "aice"] + (["tu_ice", "tu_snow"] if cfg["snow"] else ["Tu"])
