"""The SHORTWAVE top-flux term (absorbed shortwave with a stepped, temperature-dependent albedo) without a GPU: the restatement
tests/thermo_shortwave_ref.py against tests/thermo_linear_ref.py and against itself on every branch of the surface solve, the
reference's energy-conservation test per cell, the layouts of include/csi.h as gcc, ctypes and the Julia stub see them, the Python front
end's checks, its series slot and writer hook, and the resource usage of the new kernel instantiations."""
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
import output_ref
import thermo_flux_ref as R
import thermo_linear_ref as T
import thermo_shortwave_ref as S
from test_thermo_linear_ref import CLOSURE, mixed_cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = csi._lib
MAXITERS = 1000


def converged(its):
    """The condition every comparison here stands on: no consolidated cell reaches maxiters in the restatement."""
    worst = max(int(i.max()) for i in its if i.size)
    assert worst < MAXITERS, worst
    return worst


# ---- the term ----------------------------------------------------------------------------------------------------------------------

def test_without_the_term_the_steps_are_the_linear_restatement():
    h, a, hs, Tu, Ta, K = mixed_cells(seed=5)
    rng = np.random.default_rng(6)
    q, qb, ps = -250.0 + 400.0 * rng.random(h.size), -20.0 + 40.0 * rng.random(h.size), 3e-5 * rng.random(h.size)
    Sb = 25.0 + 10.0 * rng.random(h.size)
    for top in ([q], [R.EMISSION, q - 200.0], [T.Linear(K, Ta, "concentration"), q], [R.EMISSION, T.Linear(9.0, -12.5, None), -80.0]):
        for balance in (True, False):
            r0 = T.slab_step(h, a, Tu, 600.0, top, [qb], flux_balance=balance, S=Sb)
            r1 = S.slab_step(h, a, Tu, 600.0, top, [qb], flux_balance=balance, S=Sb)
            assert r1.pop("albedo") is None
            for k in r0:
                assert np.array_equal(r0[k], r1[k], equal_nan=True), k
            l0 = T.layered_step(h, a, hs, Tu, 600.0, top, [qb], ps, flux_balance=balance, S=Sb)
            l1 = S.layered_step(h, a, hs, Tu, 600.0, top, [qb], ps, flux_balance=balance, S=Sb)
            assert l1.pop("albedo") is None
            for k in l0:
                assert np.array_equal(l0[k], l1[k], equal_nan=True), k


def test_the_threshold_is_strict():
    """T == threshold takes warm; the next double below takes cold."""
    thr = -0.1
    below = np.nextafter(thr, -np.inf)
    Ts = np.array([thr, below, 0.0, -5.0])
    sw = S.Shortwave(-100.0, S.SEMTNER, None, None)
    assert np.array_equal(S.albedo(sw, Ts, False), [0.64, 0.75, 0.64, 0.75])
    assert np.array_equal(S.term_value(sw, Ts, np.ones(4), False), [-100.0 * (1 - 0.64), -100.0 * (1 - 0.75)] * 2)
    # ... in a step under PrescribedTemperature as well
    r = S.slab_step(np.full(4, 1.0), np.ones(4), Ts, 600.0, [sw], [0.0], flux_balance=False)
    assert np.array_equal(r["albedo"], [0.64, 0.75, 0.64, 0.75]) and np.array_equal(r["q_top"], S.term_value(sw, Ts, np.ones(4), False))


def test_product_order_and_position_in_the_sum():
    rng = np.random.default_rng(3)
    n = 2000
    F, Ts, a = -320.0 * rng.random(n), -0.2 * rng.random(n), rng.random(n)      # (half of the cells on either side of the threshold;
    sw = S.Shortwave(F, S.SEMTNER, None, "concentration")                       #  1 - 0.75 is a power of two, 1 - 0.64 is not)
    alpha = np.where(Ts < -0.1, 0.75, 0.64)
    assert 0.4 * n < (alpha == 0.64).sum() < 0.6 * n
    good = (F * (1 - alpha)) * a
    assert np.array_equal(S.term_value(sw, Ts, a, False), good)
    # the order is pinned: F * ((1 - alpha) * a) differs in the last bit on many of these cells
    other = S.term_value(sw, Ts, a, False, variant="associate")
    assert np.array_equal(other, F * ((1 - alpha) * a))
    differ = good != other
    print(f"(F * (1 - alpha)) * a != F * ((1 - alpha) * a) on {differ.sum()} of {n} cells")
    assert differ.sum() > n // 20 and np.all(np.abs(good - other)[differ] <= 2 * np.spacing(np.abs(good[differ])))
    # the term's position in the right-nested sum: t0 + (t1 + t2), not (t0 + t1) + t2
    q = -300.0 + 500.0 * rng.random(n)
    e = R.term_value(R.EMISSION, Ts)
    for terms, expect in (([sw, q, R.EMISSION], good + (q + e)), ([q, sw, R.EMISSION], q + (good + e)), ([R.EMISSION, q, sw], e + (q + good))):
        got = S.getflux(terms, Ts, a)
        assert np.array_equal(got, expect)
        left = S.getflux_left(terms, Ts, a)
        assert (got != left).sum() > n // 20, "the left-nested sum cannot be told from the right-nested one on these inputs"
    assert np.array_equal(S.getflux([sw], Ts, a), good)


def test_three_weightings():
    rng = np.random.default_rng(4)
    n = 500
    F, Ts, a = -320.0 * rng.random(n), -30.0 * rng.random(n), rng.random(n)
    a[:50] = 0.0
    v = F * (1 - np.where(Ts < -0.1, 0.75, 0.64))
    assert np.array_equal(S.term_value(S.Shortwave(F, S.SEMTNER, None, None), Ts, a, False), v)
    assert np.array_equal(S.term_value(S.Shortwave(F, S.SEMTNER, None, "concentration"), Ts, a, False), v * a)
    got = S.term_value(S.Shortwave(F, S.SEMTNER, None, "ice_present"), Ts, a, False)
    assert np.all(got[:50] == 0.0) and not np.signbit(got[:50]).any() and np.array_equal(got[50:], v[50:])
    # ... and they move a step
    h = np.full(n, 1.0)
    rs = [S.slab_step(h, a, Ts, 600.0, [S.Shortwave(F, S.SEMTNER, None, w), -50.0], [2.0]) for w in (None, "concentration", "ice_present")]
    assert all((rs[i]["q_top"] != rs[j]["q_top"]).any() for i, j in ((0, 1), (1, 2), (0, 2)))
    assert (rs[0]["aice"] != rs[1]["aice"]).any() and (rs[1]["aice"] != rs[2]["aice"]).any()      # (None and "ice_present" differ at aice == 0 only)


def test_the_snow_pair_holds_only_where_hs_is_positive():
    h, a, hs, Tu, Ta, K = mixed_cells(seed=9)
    snow_pair = S.Albedo(0.85, 0.70, -0.05)
    sw = S.Shortwave(-150.0, S.SEMTNER, snow_pair, None)
    snowy = hs > 0
    assert snowy.sum() > 100 and (~snowy).sum() > 100
    Ts = np.where(np.arange(h.size) % 2 == 0, -0.07, -3.0)      # between the two thresholds / below both
    got = S.albedo(sw, Ts, snowy)
    expect = np.where(snowy, np.where(Ts < -0.05, 0.85, 0.70), np.where(Ts < -0.1, 0.75, 0.64))
    assert np.array_equal(got, expect) and set(np.unique(got)) == {0.85, 0.75, 0.64}
    r = S.layered_step(h, a, hs, Ts, 600.0, [sw, -40.0], [2.0], 2e-5, flux_balance=False)
    assert np.array_equal(r["albedo"], expect)
    # without a snow pair the ice pair serves both; the bare-ice step never takes the snow pair
    r0 = S.layered_step(h, a, hs, Ts, 600.0, [S.Shortwave(-150.0, S.SEMTNER, None, None), -40.0], [2.0], 2e-5, flux_balance=False)
    assert np.array_equal(r0["albedo"], np.where(Ts < -0.1, 0.75, 0.64))
    rs = S.slab_step(h, a, Ts, 600.0, [sw, -40.0], [2.0], flux_balance=False)
    assert np.array_equal(rs["albedo"], np.where(Ts < -0.1, 0.75, 0.64))
    # hs after the step does not matter: the snow that melts away within the step still had the snow pair
    its = []
    rb = S.layered_step(h, a, hs, np.full(h.size, -5.0), 86400.0, [sw, -300.0], [2.0], 0.0, iterations=its)
    converged(its)
    gone = snowy & (rb["hs"] == 0) & (h >= 0.05)
    assert gone.any() and set(np.unique(rb["albedo"][gone])) <= {0.85, 0.70}


# ---- every branch of the surface solve -----------------------------------------------------------------------------------------------

def test_branch_coverage_and_convergence():
    """The 200 000 random cells the stepped form was tried on (seed 3) plus thin ice: every branch has cells -- each count asserted
    non-zero first --, no consolidated cell reaches maxiters, and each branch behaves.  Recorded: at most 135 updates; cold 151 861,
    warm below Tm 80, capped 48 059, within tol of the jump 4, unconsolidated 2 000 (printed below)."""
    s = S.random_state()
    s["h"] = np.concatenate([s["h"], np.linspace(0.0, 0.0499, 2000)])
    for k in ("a", "S", "Tu", "Fsw", "Fin"):
        s[k] = np.concatenate([s[k], s[k][:2000]])
    top = S.random_top(s)
    its = []
    r = S.slab_step(s["h"], s["a"], s["Tu"], 8 * 3600.0, top, [0.0], S=s["S"], iterations=its)
    n = S.branch_counts(r, s, top)
    print("branches:", n, "most updates:", int(its[0].max()))
    for k in ("cold", "warm", "capped", "jump", "unconsolidated"):
        assert n[k] > 0, k
    assert converged(its) <= 200
    cons = s["h"] >= 0.05
    Tb = -0.054 * s["S"]
    assert np.array_equal(r["Tu"][~cons], Tb[~cons]) and np.all(np.isfinite(r["h"])) and np.all(np.isfinite(r["Tu"]))
    cold, warm, capped = cons & (r["Tu"] < -0.1), cons & (r["Tu"] >= -0.1) & (r["Tu"] < 0), cons & (r["Tu"] == 0)
    assert np.all(r["albedo"][cold] == 0.75) and np.all(r["albedo"][warm] == 0.64) and np.all(r["albedo"][capped] == 0.64)
    # away from the jump the balance is met to what tol leaves: |Qx - Qi| <= (|dQx/dT| + k / h) * tol, dQx/dT = 4 sigma x^3 < 6 W m^-2 K^-1
    jump = cons & (np.abs(r["Tu"] + 0.1) < 1e-3)
    Qi = -2.0 * (r["Tu"] - Tb) / np.where(cons, s["h"], 1.0)
    off = np.abs(r["q_top"] - Qi)
    smooth = (cold | warm) & ~jump
    unmet = smooth & (off > (6.0 + 2.0 / np.where(cons, s["h"], 1.0)) * 1e-3)
    # ... except where the iterates straddle the jump and the secant's step rule ends it early (e.g. x0 warm, x1 cold with nearly equal
    # residuals: one huge step out, one back, then |x1 - x0| < tol).  The reference's solver does the same with its closure; the cells
    # are few and the step stays finite there.
    print(f"balance unmet away from the jump on {unmet.sum()} of {smooth.sum()} cells")
    assert unmet.sum() <= smooth.sum() // 5000
    # at the jump neither branch has a root: the balance is positive on one side and negative on the other
    assert np.all(off[jump] <= np.abs(s["Fsw"][jump]) * (0.75 - 0.64) + (6.0 + 2.0 / s["h"][jump]) * 1e-3) and (off[jump] > 1.0).any()
    # a capped cell melts with the warm albedo
    q_warm = S.getflux([S.Shortwave(s["Fsw"], S.Albedo(0.64, 0.64, -0.1), None, None)] + top[1:], r["Tu"], s["a"])
    assert np.array_equal(r["q_top"][capped], q_warm[capped])
    not_melting = int((r["q_top"][capped] >= Qi[capped]).sum())      # (Qu < Qi: the top melts -- but for a root the step rule left above Tm)
    print(f"capped cells whose top does not melt: {not_melting} of {capped.sum()}")
    assert not_melting <= capped.sum() // 5000


@pytest.mark.parametrize("weighting", [None, "concentration", "ice_present"])
def test_layered_branches_on_mixed_cells(weighting):
    """Snow and bare cells, open water, aice == 0, thin ice: both steps stay finite, converge, and use each albedo somewhere."""
    h, a, hs, Tu, Ta, K = mixed_cells(seed=21)
    rng = np.random.default_rng(22)
    F = -320.0 * rng.random(h.size)
    top = [S.Shortwave(F, S.SEMTNER, S.Albedo(0.85, 0.70, -0.05), weighting), -150.0 - 150.0 * rng.random(h.size), R.EMISSION]
    its = []
    r = S.layered_step(h, a, hs, Tu, 3600.0, top, [2.0], 2e-5, S=30.0, iterations=its)
    converged(its)
    for k, x in r.items():
        assert np.all(np.isfinite(x)), k
    assert set(np.unique(r["albedo"])) == {0.85, 0.75, 0.70, 0.64}


# ---- energy closure: test/test_energy_conservation.jl per cell ------------------------------------------------------------------------

def _closure(snow, precipitation, melting, partial, variant=None):
    """T.closure_run's loop with the shortwave term ahead of its bulk term; q_top is the flux the step used -- or, with a variant, that
    flux as the variant would have it at the temperature the step solved.  The flux per cell: 20-150 W m^-2 on bare ice, 2-10 W m^-2
    over snow, so that the snow cover survives the 200 steps as it does in the bulk-only test: in the step in which the snow melts away
    the layered step of before does not close to round-off with ANY top flux (1.2e-7 with a constant -60 W m^-2 in place of the term),
    which is not this term's doing.  The premise is asserted."""
    st = T.closure_state(partial=partial, snow=snow, melting=melting)
    rng = np.random.default_rng(31)
    F = -(2.0 + 8.0 * rng.random(64)) if snow else -(20.0 + 130.0 * rng.random(64))
    sw = S.Shortwave(F, S.SEMTNER, S.Albedo(0.85, 0.70, -0.05) if snow else None, "concentration" if partial else None)
    its, seen, last = [], set(), {}

    def step(x, top, bottom, Ps):
        if snow:
            r = S.layered_step(x["h"], x["a"], x["hs"], x["Tu"], 600.0, top, bottom, Ps, iterations=its)
            r["Tu"] = r["tu_snow"]
            snowy = x["hs"] > 0
        else:
            r = S.slab_step(x["h"], x["a"], x["Tu"], 600.0, top, bottom, iterations=its)
            r.update(hs=np.zeros_like(x["h"]), mf_int=np.zeros_like(x["h"]))
            snowy = False
        recomputed = S.getflux(top, r["Tu"], x["a"], snowy)
        assert np.array_equal(recomputed, r["q_top"])           # the used flux is Qx at the temperature the step wrote
        seen.update(np.unique(r["albedo"]).tolist())
        last["hs"] = r["hs"]
        if variant is not None:
            r["q_top"] = S.getflux(top, r["Tu"], x["a"], snowy, variant=variant)
        return r
    worst = T.closure_run(st, snow, precipitation, 200, extra_top=(sw,), step=step)
    converged(its)
    assert not snow or np.all(last["hs"] > 0), "the snow cover melted away: the closure of the layered step of before no longer holds"
    return worst, seen


@pytest.mark.parametrize("snow, precipitation, melting, partial", CLOSURE)
def test_energy_closure(snow, precipitation, melting, partial):
    """The combinations and bounds of tests/test_thermo_linear_ref.py::test_energy_closure (1e-15 at aice = 1, 1e-13 at aice < 1), 200
    steps of 600 s on its 64 cells, with a per-cell shortwave flux ahead of the bulk term (_closure).  Measured on this
    restatement: 4.0e-16 ... 6.3e-16 over the twelve combinations."""
    worst, seen = _closure(snow, precipitation, melting, partial)
    print(f"energy closure snow={snow} precipitation={precipitation} melting={melting} partial={partial}: {worst.max():.2e} "
          f"(albedos used: {sorted(seen)})")
    assert seen, "no albedo was used"
    assert worst.max() < (1e-13 if partial else 1e-15)


@pytest.mark.parametrize("snow, melting", [(False, False), (False, True), (True, True)])
def test_the_closure_check_fails_with_cold_and_warm_swapped(snow, melting):
    """With q_top formed from the swapped pair the same check misses by (cold - warm) F dt of energy: 4e9 ... 5e10 times the bound
    (printed)."""
    worst, _ = _closure(snow, False, melting, False, variant="swap")
    print(f"swapped albedos, snow={snow} melting={melting}: residual {worst.max():.2e} = {worst.max() / 1e-15:.1e} x the bound")
    assert worst.min() > 1e-15 * 1e6


# ---- the example's column --------------------------------------------------------------------------------------------------------------

def column_run(t0, nsteps, h0, Tu0=0.0, dt=8 * 3600.0):
    """The example's column (bare ice, flux balance, S = 0, no bottom flux) from clock time t0: per step (Tu, albedo, updates)."""
    h, a, Tu = np.array([h0]), np.ones(1), np.array([Tu0])
    out = []
    for n in range(nsteps):
        its = []
        r = S.slab_step(h, a, Tu, dt, S.column_top(t0 + n * dt), [0.0], iterations=its)
        h, a, Tu = r["h"], r["aice"], r["Tu"]
        out.append((float(Tu[0]), float(r["albedo"][0]), int(its[0].max()), float(h[0])))
    return out


def test_the_column_crosses_the_threshold_from_day_130():
    """90 eight-hour steps from day 130 with 2.8 m of ice: the surface warms through the threshold, the albedo drops from 0.75 to 0.64
    and the surface reaches the melting point; the solve converges at every step."""
    run = column_run(130 * S.DAY, 90, 2.8, Tu0=-8.0)
    Tu = np.array([r[0] for r in run])
    alpha = np.array([r[1] for r in run])
    assert max(r[2] for r in run) < MAXITERS
    assert alpha[0] == 0.75 and alpha[-1] == 0.64 and Tu[0] < -0.1 and Tu[-1] == 0.0
    first_warm = int(np.argmax(alpha == 0.64))
    print(f"column: Tu {Tu[0]:.2f} -> {Tu[-1]:.2f}, first warm step {first_warm}, most updates {max(r[2] for r in run)}")
    assert 0 < first_warm < 89 and np.all(np.isfinite(Tu))
    assert S.forcing_at("shortwave", 0.0) == 0.0 and S.forcing_at("shortwave", 165 * S.DAY) == S.MONTHLY["shortwave"][5]
    # Cyclical indexing: December -> January across the year's end, and year 2 is year 1
    assert S.forcing_at("others", 350 * S.DAY) == S.forcing_at("others", (350 + 360) * S.DAY)
    lo, hi = sorted((S.MONTHLY["others"][11], S.MONTHLY["others"][0]))
    assert lo <= S.forcing_at("others", 359 * S.DAY) <= hi


# ---- layouts --------------------------------------------------------------------------------------------------------------------------

def _c_layout(tmp_path):
    exe = str(tmp_path / "thermo_shortwave_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "thermo_shortwave_layout.c"), "-o", exe])
    return json.loads(subprocess.check_output([exe]).decode())


def test_c_layout_matches_ctypes(tmp_path):
    got = _c_layout(tmp_path)
    assert got["sizeof_shortwave"] == C.sizeof(L.Shortwave) == 72
    for name, _ in L.Shortwave._fields_:
        assert got[f"csi_shortwave.{name}"] == getattr(L.Shortwave, name).offset, name
    # csi_heat_flux_term keeps its size and offsets
    assert got["sizeof_term"] == C.sizeof(L.HeatFluxTerm) == 40
    assert [got[f"csi_heat_flux_term.{n}"] for n, _ in L.HeatFluxTerm._fields_] == [0, 4, 8, 16, 24, 32]
    assert (got["CSI_FLUX_CONSTANT"], got["CSI_FLUX_ARRAY"], got["CSI_FLUX_RADIATIVE_EMISSION"], got["CSI_FLUX_LINEAR"],
            got["CSI_FLUX_SHORTWAVE"]) == (L.FLUX_CONSTANT, L.FLUX_ARRAY, L.FLUX_RADIATIVE_EMISSION, L.FLUX_LINEAR, L.FLUX_SHORTWAVE) == \
        (0, 1, 2, 3, 4)
    assert (got["CSI_WEIGHT_NONE"], got["CSI_WEIGHT_CONCENTRATION"], got["CSI_WEIGHT_ICE_PRESENT"]) == (0, 1, 2)
    # every older id and count keeps its value; the two new slots follow
    assert (got["CSI_F_COUNT"], got["CSI_F_COUNT_ALL"], got["CSI_F_COUNT_TOTAL"], got["CSI_F_COUNT_DERIVED"], got["CSI_F_COUNT_BINDABLE"],
            got["CSI_F_COUNT_THERMO"], got["CSI_F_COUNT_MIXED_LAYER"]) == (36, 39, 41, 48, 58, 63, 70) and got["CSI_VERSION"] == 100
    assert (L.F_COUNT_BINDABLE, L.F_COUNT_THERMO, L.F_COUNT_MIXED_LAYER) == (58, 63, 70)
    for k, n in enumerate(L.SHORTWAVE_FIELD_IDS):
        assert got["CSI_F_" + n] == L.F_SHORTWAVE[n] == L.slot_id(n) == 70 + k
    assert got["CSI_F_COUNT_SHORTWAVE"] == L.F_COUNT_SHORTWAVE == 72
    for name in list(L.F) + list(L.F_DERIVED) + list(L.F_MOMENTUM_TERMS) + list(L.F_THERMO_LINEAR) + list(L.F_MIXED_LAYER):
        assert L.slot_id(name) < 70, name
    assert "csi_shortwave_set" in L.SYMBOLS


def test_c_layout_matches_julia_stub(tmp_path):
    got = _c_layout(tmp_path)
    stub = open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl"), encoding="utf-8").read()
    m = re.search(r"^const SHORTWAVE = \((.*?)\)", stub, re.S | re.M)
    assert m, "const SHORTWAVE is missing from the Julia stub"
    slots = {k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)", m.group(1))}
    assert slots == {n: got["CSI_F_" + n] for n in L.SHORTWAVE_FIELD_IDS}
    m = re.search(r"^const CSI_FLUX_SHORTWAVE = (\d+)", stub, re.M)
    assert m and int(m.group(1)) == got["CSI_FLUX_SHORTWAVE"]
    m = re.search(r"^struct\s+CsiShortwave\b[^\n]*\n(.*?)\nend", stub, re.S | re.M)
    assert m, "struct CsiShortwave is missing from the Julia stub"
    fields = re.findall(r"([A-Za-z_]\w*)::(\w+)", re.sub(r"#[^\n]*", "", m.group(1)))
    size_of = {"Cdouble": 8, "Float64": 8, "Int32": 4, "Cint": 4}
    off, offsets = 0, {}
    for name, t in fields:
        off = (off + size_of[t] - 1) // size_of[t] * size_of[t]
        offsets[name] = off
        off += size_of[t]
    assert offsets == {n: got[f"csi_shortwave.{n}"] for n, _ in L.Shortwave._fields_} and (off + 7) // 8 * 8 == got["sizeof_shortwave"]
    assert re.search(r"ccall\(\(:csi_shortwave_set, ", stub) and "function attach_shortwave!" in stub
    assert re.search(r"CsiShortwave[^\n]*72", stub), "the static check does not carry the struct's size"
    assert re.search(r"FluxFunction[^\n]*attach_shortwave!", stub), "the stub's FluxFunction refusal does not point to attach_shortwave!"


def test_header_is_the_definition():
    text = open(os.path.join(ROOT, "include", "csi.h"), encoding="utf-8").read()
    for words in ("alpha = (T < threshold) ? cold : warm", "Q     = (F * (1 - alpha)) * w", "CSI_FLUX_SHORTWAVE = 4",
                  "CSI_F_SHORTWAVE = CSI_F_COUNT_MIXED_LAYER", "NOT OFFERED: a continuous ramp albedo", "246 cells cycling",
                  "melts with the warm albedo", "nineteen slots, one launch", "int32_t csi_shortwave_set(csi_context* ctx, const csi_shortwave* p);"):
        assert words in text, words


# ---- the kernels' generated code (the build keeps the compiler's resource-usage remarks beside the object) ---------------------------

def _remarks(*units):
    """The resource-usage remarks of the kernels of these units (csrc/Makefile keeps them beside the objects): name -> figures."""
    csrc = os.path.join(ROOT, "climaseaice.jl_amd", "csrc")
    subprocess.check_call(["make", "-s", "-j8", "-C", csrc], stdout=subprocess.DEVNULL)      # (no-op when the library is up to date)
    out = {}
    for unit in units:
        for b in open(os.path.join(csrc, unit + ".res")).read().split("remark: Function Name: ")[1:]:
            g = lambda k: int(re.search(k + r"[^:]*: (\d+)", b).group(1))
            out[b.split()[0]] = dict(scratch=g("ScratchSize"), vspill=g("VGPRs Spill"), sspill=g("SGPRs Spill"), lds=g("LDS Size"),
                                     vgprs=g(r"    VGPRs"), occupancy=g("Occupancy"))
    return out


def _instantiations():
    out = _remarks("thermo_flux", "thermo_flux_sw1", "thermo_flux_sw2")      # one object per state of the term (csrc/Makefile)
    for name, v in out.items():
        m = re.search(r"k_(slab|layered)_fluxILb([01])ELb([01])ELb([01])ELb([01])E(?:Lb([01])E)?Li(\d)ELb([01])ELi(\d)EJ", name)
        assert m, name
        v.update(kernel=m.group(1), sw=int(m.group(9)))
    return out


def test_new_instantiations_have_no_scratch_and_no_spills():
    """csrc/thermo_flux*.res: 16 x 6 slab and 32 x 6 layered combinations of the older flags, each in three shortwave states.  The
    number and per-cell states are new: 192 slab and 384 layered instantiations, none with scratch, spilled registers or LDS.
    csrc/thermo.res: neither have k_slab and k_layered."""
    inst = _instantiations()
    count = lambda kernel, sw: sum(1 for v in inst.values() if v["kernel"] == kernel and v["sw"] == sw)
    assert [count("slab", k) for k in (0, 1, 2)] == [96, 96, 96] and [count("layered", k) for k in (0, 1, 2)] == [192, 192, 192]
    new = {n: v for n, v in inst.items() if v["sw"] != 0}
    for n, v in new.items():
        assert v["scratch"] == 0 and v["vspill"] == 0 and v["sspill"] == 0 and v["lds"] == 0, (n, v)
    print("new instantiations: VGPRs %d ... %d, occupancy %d ... %d" % (min(v["vgprs"] for v in new.values()),
          max(v["vgprs"] for v in new.values()), min(v["occupancy"] for v in new.values()), max(v["occupancy"] for v in new.values())))
    assert max(v["vgprs"] for v in new.values()) <= 128
    # csrc/thermo.res: the numeric kernels, which run each step's second half from the same functions (thermo_dev.h)
    numeric = _remarks("thermo")
    assert len(numeric) == 2 and all(re.search(r"\dk_(slab|layered)E", n) for n in numeric), list(numeric)
    for n, v in numeric.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vspill"] == 0 and v["sspill"] == 0, (n, v)


# ---- front end -----------------------------------------------------------------------------------------------------------------------

def grid():
    return csi.RectilinearGrid((4, 3), x=(0, 1), y=(0, 1), halo=(3, 3))


def series(g, nt=3):
    return csi.FieldTimeSeries(g, (csi.Center, csi.Center), np.arange(nt) * 10.0, np.zeros((nt, g.Ny, g.Nx)))


@pytest.mark.parametrize("kw, err, words", [
    (dict(bottom_heat_flux=csi.ShortwaveRadiation(-100.0)), NotImplementedError, "ShortwaveRadiation is a top heat flux only"),
    (dict(bottom_heat_flux=(1.0, csi.ShortwaveRadiation(-100.0))), NotImplementedError, "ShortwaveRadiation is a top heat flux only"),
    (dict(top_heat_flux=(csi.ShortwaveRadiation(-100.0), csi.ShortwaveRadiation(-50.0))), NotImplementedError,
     "at most one ShortwaveRadiation"),
    (dict(top_heat_flux=csi.ShortwaveRadiation(-100.0, snow_albedo=csi.SteppedAlbedo(0.85, 0.7, 0.0))), ValueError,
     "snow_albedo is given, but the model has no snow layer"),
    (dict(top_heat_flux=csi.ShortwaveRadiation(np.zeros((4, 4)))), ValueError, "ShortwaveRadiation.flux"),
    (dict(top_heat_flux=(2.0, csi.ShortwaveRadiation(np.zeros(5)))), ValueError, "ShortwaveRadiation.flux"),
    (dict(top_heat_flux=lambda i, j, grid, T, clock, fields: 0.0), NotImplementedError, "FluxFunction and other callables.*ShortwaveRadiation"),
])
def test_model_refusals_by_name(kw, err, words):
    with pytest.raises(err, match=words):
        csi.SeaIceModel(grid(), ice_thermodynamics=csi.SlabThermodynamics(), **kw)


@pytest.mark.parametrize("make, err, words", [
    (lambda: csi.SteppedAlbedo(cold=1.2), ValueError, "SteppedAlbedo.cold = 1.2: an albedo lies in \\[0, 1\\]"),
    (lambda: csi.SteppedAlbedo(warm=-0.01), ValueError, "SteppedAlbedo.warm = -0.01: an albedo lies in \\[0, 1\\]"),
    (lambda: csi.SteppedAlbedo(threshold=float("nan")), ValueError, "SteppedAlbedo.threshold: a finite number"),
    (lambda: csi.ShortwaveRadiation(-100.0, albedo=lambda T: 0.7), TypeError, "ShortwaveRadiation.albedo: a SteppedAlbedo is needed"),
    (lambda: csi.ShortwaveRadiation(-100.0, snow_albedo=0.8), TypeError, "ShortwaveRadiation.snow_albedo: a SteppedAlbedo is needed"),
    (lambda: csi.ShortwaveRadiation(lambda i, j: 0.0), TypeError, "ShortwaveRadiation.flux"),
    (lambda: csi.ShortwaveRadiation(float("inf")), ValueError, "ShortwaveRadiation.flux is not finite"),
    (lambda: csi.ShortwaveRadiation(-100.0, area_weighting="area"), ValueError, "ShortwaveRadiation.area_weighting"),
])
def test_object_refusals_by_name(make, err, words):
    with pytest.raises(err, match=words):
        make()


def test_front_end_objects_params_and_series_slot():
    a = csi.SteppedAlbedo()
    assert (a.cold, a.warm, a.threshold) == (0.75, 0.64, -0.1)
    f = csi.ShortwaveRadiation(-120)
    p = f.params()
    assert (p.flux, p.cold, p.warm, p.threshold, p.weighting, p.per_cell, p.has_snow_pair, p.reserved) == \
        (-120.0, 0.75, 0.64, -0.1, L.WEIGHT_NONE, 0, 0, 0) and not f.per_cell
    f = csi.ShortwaveRadiation(np.zeros((3, 4)), csi.SteppedAlbedo(0.8, 0.6, -1.0), csi.SteppedAlbedo(0.9, 0.7, -0.5), "ice_present")
    p = f.params()
    assert (p.flux, p.cold, p.warm, p.threshold, p.snow_cold, p.snow_warm, p.snow_threshold, p.weighting, p.per_cell, p.has_snow_pair) == \
        (0.0, 0.8, 0.6, -1.0, 0.9, 0.7, -0.5, L.WEIGHT_ICE_PRESENT, 1, 1) and f.per_cell
    assert csi.ShortwaveRadiation(-1.0, area_weighting="concentration").params().weighting == L.WEIGHT_CONCENTRATION
    g = grid()
    from climaseaice_jl_amd import model as model_module
    fts = csi.ShortwaveRadiation(series(g))
    assert fts.per_cell
    model_module.check_heat_flux((fts, 2.0, csi.RadiativeEmission()), "top", g)          # accepted
    # the series slot: the nineteenth, reached through the model's one name -> slot lookup like every other per-cell input
    assert model_module.series_slot_of("shortwave") == "SHORTWAVE" == L.SHORTWAVE_SERIES_SLOTS[0] and L.slot_id("SHORTWAVE") == 70
    assert model_module.series_slot_of("top_heat_flux") == "TOP_HEAT_FLUX" and model_module.series_slot_of("ocean_coefficient") == "ML_COEFFICIENT"
    assert len(L.SERIES_SLOTS) + len(L.THERMO_SERIES_SLOTS) + len(L.MIXED_LAYER_SERIES_SLOTS) + len(L.SHORTWAVE_SERIES_SLOTS) == 19
    with pytest.raises(KeyError):
        model_module.series_slot_of("albedo_used")


def test_writer_takes_albedo_used_by_name(tmp_path):
    """OutputWriter(model, ["albedo_used"], ...): allocated the first time it is asked for -- by the writer, before it looks the names
    up -- on the stand-in recorder."""
    g = csi.RectilinearGrid((8, 6), x=(0, 8), y=(0, 6), topology=(csi.Bounded, csi.Bounded), halo=(2, 2))
    fields = OrderedDict()
    fields["h"] = csi.CenterField(g, None, "h")
    asked = []

    class Model(SimpleNamespace):
        @property
        def albedo_used(self):
            asked.append(1)
            if "albedo_used" not in fields:
                fields["albedo_used"] = csi.CenterField(g, None, "albedo_used")
                fields["albedo_used"].data.fill_(0.64)
            return fields["albedo_used"]
    mk = lambda shortwave: Model(grid=g, clock=SimpleNamespace(time=0.0, iteration=0), fields=fields, output_writers=OrderedDict(),
                                 shortwave=shortwave)
    with pytest.raises(ValueError, match="'albedo_used' is not a field the model has bound"):
        csi.OutputWriter(mk(None), ["albedo_used"], csi.IterationInterval(1), str(tmp_path / "none"), recorder=output_ref.RefRecorder)
    assert not asked
    m = mk(csi.ShortwaveRadiation(-100.0))
    w = csi.OutputWriter(m, ["h", "albedo_used"], csi.IterationInterval(1), str(tmp_path / "o"), dtype="f64", recorder=output_ref.RefRecorder)
    assert asked and w.names == ["h", "albedo_used"]
    w.write(m)
    w.close()
    out = csi.load_output(str(tmp_path / "o"))
    assert np.all(out["albedo_used"][0] == 0.64)
