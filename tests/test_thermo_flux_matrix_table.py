"""The table of tests/thermo_flux_matrix.py, checked without a GPU: its numbers are the ones csrc/thermo_flux.hip and csrc/csi_thermo.hip
state, its cases reach every one of the 864 instantiations of k_slab_flux / k_layered_flux (each flux-balance-capable one under both
boundary conditions), the inputs make every flag of every case matter -- shown on the restatement alone --, and the restatement
satisfies on its own what the GPU matrix relies on: no secant at maxiters, finite outputs, every regime present in the 65 x 5 state."""
import os
import re

import numpy as np
import pytest

import climaseaice_jl_amd as csi
import test_gpu_thermo_linear as TL
import test_gpu_thermo_shortwave as TS
import thermo_flux_matrix as M
import thermo_flux_ref as R
import thermo_linear_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaseaice.jl_amd", "csrc")
L = csi._lib


def read(*path):
    with open(os.path.join(*path), encoding="utf-8") as f:
        return f.read()


@pytest.fixture(scope="module")
def flux():
    return read(CSRC, "thermo_flux.hip")


@pytest.fixture(scope="module")
def host():
    return read(CSRC, "csi_thermo.hip")


@pytest.fixture(scope="module")
def results():
    """The restatement of every case, once: {id: (dict, [largest secant update count per step])}."""
    st = M.matrix_state()
    out = {}
    for cid, key, cfg in M.CASES:
        its = []
        out[cid] = (M.reference(cfg, st, mode_iterations=its), its)
    return out


# ---- the rule against the source ---------------------------------------------------------------------------------------------------
def test_bit_weights_and_strides(flux):
    assert ("return (ff.qtop.p ? %d : 0) | (ff.qbot.p ? %d : 0) | (flux_has_emission(F.top) ? %d : 0) |" % (M.BIT_QT, M.BIT_QB, M.BIT_EMIT)) in flux
    assert "(flux_reads_surface_temperature(F, sw.mode, top_bc_kind) ? %d : 0);" % M.BIT_LTU in flux
    assert "const int b = flux_bits(F, ff, sw, S.top_bc_kind) + %d * flux_variant(F);" % M.STRIDE[M.K_SLAB_FLUX] in flux
    assert ("const int b = (flux_bits(F, ff, sw, W.top_bc_kind) | (F.snowfall_array ? %d : 0)) + %d * flux_variant(F);"
            % (M.BIT_PS, M.STRIDE[M.K_LAYERED_FLUX])) in flux
    assert "int flux_variant(const HeatFluxDev& F) { return F.lin + 3 * (F.bottom_salinity_array ? 1 : 0); }" in flux
    assert M.BIT_PS == M.STRIDE[M.K_SLAB_FLUX] and 2 * M.BIT_PS == M.STRIDE[M.K_LAYERED_FLUX] and M.VARIANTS == 3 * 2
    kernels = read(CSRC, "csi_kernels.h")
    assert "enum : int { LIN_NONE = %d, LIN_NUMBERS = %d, LIN_ARRAYS = %d };" % (M.LIN_NONE, M.LIN_NUMBERS, M.LIN_ARRAYS) in kernels
    assert "enum : int { SW_NONE = %d, SW_NUMBER = %d, SW_CELL = %d };" % (M.SW_NONE, M.SW_NUMBER, M.SW_CELL) in kernels


def test_table_sizes_and_the_three_objects(flux):
    assert "slab_table_entry(b, std::make_integer_sequence<int, 16 * 6>{})" in flux and M.TABLE[M.K_SLAB_FLUX] == 16 * 6
    assert "layered_table_entry(b, std::make_integer_sequence<int, 32 * 6>{})" in flux and M.TABLE[M.K_LAYERED_FLUX] == 32 * 6
    make = read(CSRC, "Makefile")
    objs = dict(re.findall(r"^(thermo_flux\w*\.o): FLUX_SW := (\d)$", make, re.M))
    assert objs == {"thermo_flux.o": "0", "thermo_flux_sw1.o": "1", "thermo_flux_sw2.o": "2"}
    assert "-DCSI_FLUX_SW=$(FLUX_SW)" in make and "FLUX_OBJS := thermo_flux.o thermo_flux_sw1.o thermo_flux_sw2.o" in make
    assert (M.SW_NONE, M.SW_NUMBER, M.SW_CELL) == (0, 1, 2)      # CSI_FLUX_SW is the SW template argument itself
    assert flux.count("CSI_FLUX_SW, ShortwaveDev>") == 2
    assert len(M.all_keys()) == 3 * (96 + 192) == 864


def decode(flux, kernel, nargs):
    """The template arguments `kernel<...>` is launched with, as Python expressions of B: one list per launch statement."""
    found = re.findall(r"hipLaunchKernelGGL\(\(" + kernel + r"<(.*?)>\),", flux, re.S)
    assert len(found) == 2, kernel                        # the SW_NONE form and the form with the setting
    out = []
    for args in found:
        parts = [a.strip() for a in args.replace("\n", " ").split(",")]
        assert parts[nargs:] in ([], ["CSI_FLUX_SW", "ShortwaveDev"]), parts
        out.append([a.replace("/", "//") for a in parts[:nargs]])
    assert out[0] == out[1]
    return out[0]


def test_decode_expressions_are_the_inverse(flux):
    """slab_inst<B> / layered_inst<B> turn B back into the flags flags_of states, for every B of both tables."""
    for step, kernel, names in ((M.K_SLAB_FLUX, "k_slab_flux", ("QT", "QB", "EMIT", "LTU", "LIN", "SB")),
                                (M.K_LAYERED_FLUX, "k_layered_flux", ("QT", "QB", "EMIT", "LTU", "PS", "LIN", "SB"))):
        exprs = decode(flux, kernel, len(names))
        for B in range(M.TABLE[step]):
            got = {n: eval(e, {"B": B}) for n, e in zip(names, exprs)}
            assert got == M.flags_of(step, B), (kernel, B, got)
    assert re.search(r"template <bool QT, bool QB, bool EMIT, bool LTU, int LIN = LIN_NONE, bool SB = false, int SW = SW_NONE, class\.\.\. SwArg>\s*"
                     r"__global__ void __launch_bounds__\(256\) k_slab_flux\(", flux)
    assert re.search(r"template <bool QT, bool QB, bool EMIT, bool LTU, bool PS, int LIN = LIN_NONE, bool SB = false, int SW = SW_NONE, class\.\.\. SwArg>\s*"
                     r"__global__ void __launch_bounds__\(256\) k_layered_flux\(", flux)


def test_path_and_surface_temperature_rules(flux, host):
    assert ("return F.top.n > 0 || F.bot.n > 0 || F.prescribed_array || (snow && F.snowfall_array) || F.bottom_salinity_array ||\n"
            "           c->f[CSI_F_TOP_HEAT_FLUX_USED].p || c->f[CSI_F_BOTTOM_HEAT_FLUX_USED].p;") in host
    assert ("return (top_bc_kind == 0 && F.prescribed_array) ||\n"
            "           (top_bc_kind == 1 && (flux_has_emission(F.top) || F.lin != LIN_NONE || sw_mode != SW_NONE));") in flux
    # the array flags follow the tuples; the shortwave setting counts only when the top's tuple has the term
    assert "if (has_array_term(F.top)) { ids.push_back(CSI_F_TOP_HEAT_FLUX); ff.qtop = ref_of(c, CSI_F_TOP_HEAT_FLUX); }" in host
    assert "if (has_array_term(F.bot)) { ids.push_back(CSI_F_BOTTOM_HEAT_FLUX); ff.qbot = ref_of(c, CSI_F_BOTTOM_HEAT_FLUX); }" in host
    assert re.search(r"sw = ShortwaveDev\{\};\s*if \(c->heat_has_shortwave\) \{", host)


def test_the_launchers_report_what_they_launched(flux, host):
    thermo = read(CSRC, "thermo.hip")
    assert "return ThermoLaunch{%d, SW_NONE, -1};" % M.K_SLAB in thermo and "return ThermoLaunch{%d, SW_NONE, -1};" % M.K_LAYERED in thermo
    assert "return ThermoLaunch{%d, table, b};" % M.K_SLAB_FLUX in flux and "return ThermoLaunch{%d, table, b};" % M.K_LAYERED_FLUX in flux
    assert flux.count("const int table = sw.mode == SW_CELL ? SW_CELL : (sw.mode == SW_NUMBER ? SW_NUMBER : SW_NONE);") == 2
    assert "table == SW_CELL ? slab_flux_entry<SW_CELL>(b) : (table == SW_NUMBER ? slab_flux_entry<SW_NUMBER>(b) : slab_flux_entry<SW_NONE>(b))" in flux
    assert re.search(r"table == SW_CELL \? layered_flux_entry<SW_CELL>\(b\)\s*: \(table == SW_NUMBER \? layered_flux_entry<SW_NUMBER>\(b\) : "
                     r"layered_flux_entry<SW_NONE>\(b\)\)", flux)
    for launcher in ("launch_slab_flux_step", "launch_slab_step", "launch_layered_flux_step", "launch_layered_step"):
        assert host.count("c->last_thermo = %s(" % launcher) == 1 and len(re.findall(r"\b%s\(" % launcher, host)) == 1, launcher
    assert "tests/test_thermo_flux_matrix_table.py proves it" in flux


def test_the_export_is_declared_everywhere():
    header = read(ROOT, "include", "csi.h")
    assert re.search(r"int32_t csi_last_thermo\(csi_context\* ctx, int32_t\* step, int32_t\* shortwave, int32_t\* index\);", header)
    assert "csi_last_thermo" in L.SYMBOLS and len(L.load().csi_last_thermo.argtypes) == 4
    assert callable(L.Context.last_thermo)
    stub = read(ROOT, "julia", "ClimaSeaIceHIP.jl")
    assert re.search(r"ccall\(\(:csi_last_thermo, libcsi\), Int32, \(Ptr\{Cvoid\}, Ref\{Int32\}, Ref\{Int32\}, Ref\{Int32\}\)", stub)
    assert "function last_thermo(ctx)" in stub
    assert "`csi_last_thermo`" in read(ROOT, "INTEGRATION.md")


# ---- completeness --------------------------------------------------------------------------------------------------------------------
def test_the_matrix_reaches_every_instantiation():
    keys = M.all_keys()
    assert len(set(keys)) == 864
    prescribed = [key for (cid, key, cfg) in M.CASES if not cfg["balance"]]
    balance = [key for (cid, key, cfg) in M.CASES if cfg["balance"]]
    assert sorted(prescribed) == sorted(keys), sorted(set(keys) - set(prescribed))[:5]
    capable = [key for key in keys if M.balance_capable(key)]
    assert len(capable) == 432 and sorted(balance) == sorted(capable)
    assert len(M.CASES) == 1296 and len({cid for cid, _, _ in M.CASES}) == 1296
    for cid, key, cfg in M.CASES:
        assert M.expected_key(cfg) == key, (cid, M.expected_key(cfg))
        assert cid == key + ("balance" if cfg["balance"] else "prescribed",)
        assert len(cfg["top"]) >= 1 and cfg["top"][-1][0] == "number" and len(cfg["top"]) <= L.MAX_HEAT_FLUX_TERMS
        order = [t[0] for t in cfg["top"]]
        assert order == [k for k in ("emission", "linear", "shortwave", "array", "number") if k in order]
        assert cfg["prescribed_array"] == (M.flags_of(key[0], key[2])["LTU"] and not cfg["balance"])
    # 36 groups of 16 / 32 flux_bits values, each with both boundary conditions
    assert len(M.GROUPS) == 36
    for g in M.GROUPS:
        got = M.cases_of(g)
        assert len({key for _, key, _ in got}) == M.STRIDE[g[0]] and {cfg["balance"] for _, _, cfg in got} == {False, True}, g
    assert sum(len(M.cases_of(g)) for g in M.GROUPS) == 1296


def test_weightings_and_the_snow_pair_are_taken_in_turn():
    pairs = {(cfg["top"][[t[0] for t in cfg["top"]].index("linear")][2], cfg["shortwave"][1]) for _, key, cfg in M.CASES
             if M.linear_state(cfg) and cfg["shortwave"]}
    assert pairs == {(a, b) for a in M.WEIGHTINGS for b in M.WEIGHTINGS}
    for g in M.GROUPS:
        got = M.cases_of(g)
        if g[2] != M.LIN_NONE:
            assert {[t for t in cfg["top"] if t[0] == "linear"][0][2] for _, _, cfg in got} == set(M.WEIGHTINGS), g
            assert all([t for t in cfg["top"] if t[0] == "linear"][0][1] == (g[2] == M.LIN_ARRAYS) for _, _, cfg in got)
        if g[1] != M.SW_NONE:
            assert {cfg["shortwave"][1] for _, _, cfg in got} == set(M.WEIGHTINGS), g
            assert {cfg["shortwave"][2] for _, _, cfg in got} == ({False, True} if g[0] == M.K_LAYERED_FLUX else {False}), g


def test_the_rule_falls_back_to_the_numeric_kernels():
    base = dict(snow=False, balance=True, top=(), bottom=(), shortwave=None, prescribed_array=False, snowfall_array=False,
                salinity_array=False, used=False, bottom_flux_kind=0, Qu=-30.0, Qb=2.0)
    assert M.expected_key(base) == (M.K_SLAB, 0, -1) and M.expected_key(dict(base, snow=True)) == (M.K_LAYERED, 0, -1)
    assert M.expected_key(dict(base, snowfall_array=True)) == (M.K_SLAB, 0, -1)           # (the bare-ice step has no snowfall)
    assert M.expected_key(dict(base, snow=True, snowfall_array=True)) == (M.K_LAYERED_FLUX, 0, 16)
    assert M.expected_key(dict(base, used=True)) == (M.K_SLAB_FLUX, 0, 0) and M.expected_key(dict(base, salinity_array=True)) == (M.K_SLAB_FLUX, 0, 48)
    assert M.expected_key(dict(base, snow=True, salinity_array=True, bottom_flux_kind=1)) == (M.K_LAYERED_FLUX, 0, 96)
    # a shortwave setting without the term in the tuple selects nothing
    assert M.expected_key(dict(base, shortwave=(True, None, False), used=True)) == (M.K_SLAB_FLUX, 0, 0)


# ---- conditions the GPU matrix relies on, on the restatement alone -----------------------------------------------------------------
def test_no_secant_reaches_maxiters_and_everything_is_finite(results):
    worst = 0
    for cid, key, cfg in M.CASES:
        r, its = results[cid]
        assert len(its) == M.nsteps_of(cfg) and max(its) < M.MAXITERS, (cid, its)
        worst = max(worst, max(its))
        solved = cfg["balance"] and M.flags_of(key[0], key[2])["LTU"]
        assert (max(its) > 0) == bool(solved), (cid, its)          # the secant ran exactly where the host sets LTU under the balance
        for k in M.compared(cfg):
            assert r[k] is not None and r[k].shape == (M.NY, M.NX) and np.all(np.isfinite(r[k])), (cid, k)
    assert 2 <= worst < 200, worst


def test_the_scalars_differ_from_every_cell():
    st = M.matrix_state()
    for number, name in ((M.S0, "S"), (M.PS0, "ps"), (M.F0, "F"), (0.0, "tu0"), (M.K0, "K"), (M.TA0, "Ta"), (M.TP0, "tp")):
        assert not (st[name] == number).any(), name
    assert (st["tu0"] < -0.1).all() and ((st["tu0"] + 1 > -0.1) & (st["tu0"] < -0.1)).sum() > 20      # both kinds of starting pairs
    assert (M.NX, M.NY) == (65, 5) and M.NX % 64 == 1 and M.NY % 4 == 1 and M.HALO == TL.H == 3         # both last blocks partial


def test_every_flag_of_every_case_matters(results):
    """For each case and each flag of its key, the restatement with the input replaced by what a kernel lacking the flag reads: h, aice
    or a surface temperature differs in at least one cell.  Prints the smallest such distance."""
    st = M.matrix_state()
    smallest, runs = np.inf, 0
    for cid, key, cfg in M.CASES:
        r, _ = results[cid]
        for flag in M.flags_set(key):
            other = M.reference(cfg, st, lacking=flag)
            runs += 1
            assert any(not np.array_equal(other[k], r[k]) for k in M.surface(cfg)), (cid, flag)
            smallest = min(smallest, max(np.abs(other[k] - r[k]).max() for k in M.surface(cfg)))
    print(f"sensitivity: {runs} second runs, smallest largest-difference over the cases {smallest:.3e}")
    assert runs > 4000 and smallest > 0


def test_the_state_holds_every_regime_of_both_files():
    """test_the_state_holds_every_regime of test_gpu_thermo_linear.py and of test_gpu_thermo_shortwave.py, on the 65 x 5 state."""
    st = M.matrix_state()
    h, a, hs = st["h"], st["a"], st["hs"]
    # the LINEAR file's
    _, rtop = TL.tops(st, "concentration", "both", False)
    r = T.layered_step(h, a, hs, np.zeros_like(h), TL.DT, rtop, [st["qb"]], 0.0, S=st["S"])
    cons = h >= 0.05
    assert (h == 0).any() and ((h > 0) & ~cons).any() and (cons & (a == 0)).any()
    assert (cons & (r["tu_snow"] == 0.0) & (hs > 0)).any() and (cons & (r["tu_snow"] < -1.0)).any()
    assert ((hs > 0) & (r["hs"] == 0) & (r["aice"] > 0)).any()
    assert ((h > 0) & (a > 0) & (r["h"] == 0)).any()
    assert (r["h"] > h).any() and (r["h"] < h).any()
    # the SHORTWAVE file's
    _, rtop = TS.tops(st, None, True, True, "emission")
    r = TS.ref_steps(st, True, rtop, [st["qb"]], st["S"], 1, snowfall=st["ps"])
    tu = r["tu_snow"]
    snowy = hs > 0
    assert (cons & ~snowy & (tu < -0.1)).any() and (cons & ~snowy & (tu >= -0.1) & (tu < 0)).any() and (cons & (tu == 0)).any()
    assert (~cons).any() and (cons & (a == 0)).any()
    _, rtop_all = TS.tops(st, None, True, True, "all")
    r_all = TS.ref_steps(st, True, rtop_all, [st["qb"]], st["S"], 1, snowfall=st["ps"])
    assert set(np.unique(r["albedo"])) | set(np.unique(r_all["albedo"])) == {0.85, 0.75, 0.70, 0.64}
    r0 = TS.ref_steps(st, True, [R.EMISSION, -210.0], [st["qb"]], st["S"], 1, snowfall=st["ps"])
    assert np.abs(r["h"] - r0["h"]).max() > 1e-4
