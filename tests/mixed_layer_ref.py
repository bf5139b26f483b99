"""Test-side restatement of the slab-ocean mixed layer (include/csi.h, csi_mixed_layer_set) in NumPy fp64, statement for statement:

    C   = (rho * c) * depth
    Qs  = Fo + (K * (To - Ta))          absent terms are not added: Fo alone, the bulk term alone, or 0
    Qow = Qs * (1 - a)
    dT  = To - Tf                       Tf = liq_T0 - liq_slope * Sb
    Qio = dT > 0 ? min(((gamma * (rho * c)) * dT) * a, (C * dT) / dt) : 0
    T1  = To + (dt * ((Qd - Qow) - Qio)) / C
    Qfr = T1 < Tf ? (C * (T1 - Tf)) / dt : 0
    To' = T1 < Tf ? Tf : T1
    Qb  = Qio + Qfr

NumPy evaluates each binary operation in IEEE double and never contracts, so these lines are the device's bits.  Fo, K, Ta: None
(absent), a number or an array; Qd, Sb: a number or an array.  variant: the two wrong forms the tests show the budget check catches -- "frazil_sign": Qfr enters Qb with the wrong sign;
"no_open_water_weight": the water is cooled by Qs over the whole cell, not by Qow = Qs * (1 - a) over the open fraction."""
import numpy as np

from thermo_flux_ref import PHASE, jmin

RHO, CP, GAMMA = 1026.0, 3991.0, 6e-5


def step(To, a, dt, depth, Fo=None, K=None, Ta=None, Qd=0.0, Sb=0.0, rho=RHO, c=CP, gamma=GAMMA, p=PHASE, variant=None):
    """One step on every cell.  Returns a dict: To (To'), Qb, Qow, Qio, Qfr, Tf, C, T1."""
    To, a = np.asarray(To, dtype=np.float64), np.asarray(a, dtype=np.float64)
    assert (K is None) == (Ta is None)
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    Tf = np.array(np.broadcast_to(p["liq_T0"] - p["liq_slope"] * f64(Sb), To.shape), dtype=np.float64)
    with np.errstate(all="ignore"):
        C = (np.float64(rho) * c) * depth
        if K is not None:
            qk = f64(K) * (To - f64(Ta))
            Qs = f64(Fo) + qk if Fo is not None else qk
        elif Fo is not None:
            Qs = np.array(np.broadcast_to(f64(Fo), To.shape), dtype=np.float64)
        else:
            Qs = np.zeros_like(To)
        Qow = Qs * (1 - a)
        dT = To - Tf
        Qio = np.where(dT > 0, jmin(((gamma * (np.float64(rho) * c)) * dT) * a, (C * dT) / dt), 0.0)
        T1 = To + (dt * ((f64(Qd) - (Qs if variant == "no_open_water_weight" else Qow)) - Qio)) / C
        frazil = T1 < Tf
        Qfr = np.where(frazil, (C * (T1 - Tf)) / dt, 0.0)
        if variant == "frazil_sign":
            Qfr = -Qfr
        To1 = np.where(frazil, Tf, T1)
        Qb = Qio + Qfr
    return dict(To=To1, Qb=Qb, Qow=Qow, Qio=Qio, Qfr=Qfr, Tf=Tf, C=C, T1=T1)


def budget_residual(To, r, dt, Qd):
    """|C (To' - To) / dt - (Qd - Qow - Qb)| per cell."""
    return np.abs(r["C"] * (r["To"] - To) / dt - (np.asarray(Qd, dtype=np.float64) - r["Qow"] - r["Qb"]))


def budget_bound(To, r, dt, Qd):
    """16 * 2^-53 * (C (|To| + |To'| + |Tf|) / dt + |Qow| + |Qd| + |Qio| + |Qfr|) per cell."""
    return 16 * 2.0 ** -53 * (r["C"] * (np.abs(To) + np.abs(r["To"]) + np.abs(r["Tf"])) / dt + np.abs(r["Qow"]) +
                              np.abs(np.asarray(Qd, dtype=np.float64)) + np.abs(r["Qio"]) + np.abs(r["Qfr"]))


def random_state(n, seed, Sb=30.0):
    """Random cells around freezing: To within a few kelvin of Tf on either side, every concentration, both signs of every flux."""
    rng = np.random.default_rng(seed)
    Tf = PHASE["liq_T0"] - PHASE["liq_slope"] * Sb
    To = Tf + 3.0 * rng.standard_normal(n)
    a = np.clip(rng.random(n) * 1.2 - 0.1, 0.0, 1.0)
    Fo = 300.0 * rng.standard_normal(n)
    K = 5.0 + 20.0 * rng.random(n)
    Ta = -15.0 + 20.0 * rng.standard_normal(n)
    Qd = 20.0 * rng.standard_normal(n)
    return dict(To=To, a=a, Fo=Fo, K=K, Ta=Ta, Qd=Qd, Sb=Sb)


BRANCHES = ("frazil", "melt_free", "melt_limited", "cold_under_ice", "open_water", "full_cover")


def branch_state(shape=(6,), Sb=30.0):
    """A state in which every branch has cells, with gamma = 1e-2, dt = 3600, depth = 10 (gamma dt >= depth: the melt can be limited
    by the heat there is).  Cells cycle through six kinds along the flattened index; returns (inputs dict, kwargs of step)."""
    n = int(np.prod(shape))
    Tf = PHASE["liq_T0"] - PHASE["liq_slope"] * Sb
    kind = np.arange(n) % 6
    ramp = 1.0 + (np.arange(n) // 6) * 0.03125
    #                  frazil          melt, not limited   melt, limited    dT <= 0 under ice   a = 0            a = 1
    To = np.choose(kind, [Tf + 0.001 * ramp, Tf + 0.5 * ramp, Tf + 0.5 * ramp, Tf - 0.25 * ramp, Tf + 0.2 * ramp, Tf + 0.3 * ramp])
    a = np.choose(kind, [0.3 + 0 * ramp, 0.001 / ramp, 0.9 + 0 * ramp, 0.7 + 0 * ramp, 0 * ramp, 1.0 + 0 * ramp])
    Fo = np.choose(kind, [400.0 * ramp, 5.0 * ramp, -30.0 * ramp, 10.0 * ramp, 50.0 * ramp, 80.0 * ramp])
    inputs = dict(To=To.reshape(shape), a=a.reshape(shape), Fo=Fo.reshape(shape))
    return inputs, dict(dt=3600.0, depth=10.0, gamma=1e-2, Sb=Sb)


def branch_counts(To, a, r, dt, gamma, rho=RHO, c=CP):
    """How many cells took each branch."""
    dT = To - r["Tf"]
    free = ((gamma * (np.float64(rho) * c)) * dT) * a
    cap = (r["C"] * dT) / dt
    melting = (dT > 0) & (a > 0)
    return dict(frazil=int((r["Qfr"] < 0).sum()), melt_free=int((melting & (free < cap)).sum()),
                melt_limited=int((melting & (free >= cap)).sum()), cold_under_ice=int(((dT <= 0) & (a > 0)).sum()),
                open_water=int((a == 0).sum()), full_cover=int((a == 1).sum()))


def rk3_stages(To, a_stages, dt, depth, **kw):
    """Three RK3 stages, each from Psi^- (= To) with its own stage step dt / 3, dt / 2, dt and the concentration its thermodynamic step
    starts from: the last stage is the step's result."""
    r = None
    for beta, a in zip((3, 2, 1), a_stages):
        r = step(To, a, dt / beta, depth, **kw)
    return r
