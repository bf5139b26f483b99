"""Test-side restatement of the thermodynamic steps with the LINEAR top-flux term, a per-cell bottom salinity and the fluxes a step
used, in NumPy fp64.  It builds on tests/thermo_flux_ref.py (R): R's secant, latent heat, ice_volume_update, jmin / jmax and term
values are used as they are; what is restated here is what R's steps cannot express --

  the term Q(T) = (K * (T - Ta)) * w      the closure of examples/melting_in_spring.jl:64-73, examples/freezing_of_a_lake.jl:54-66 and
                                          test/test_energy_conservation.jl:8-13, in exactly this order:
                                            weighting None             no product by w
                                            "concentration"            w = aice at the start of the step
                                            "ice_present"              (aice == 0) ? 0 : K * (T - Ta)
  the secant whenever the top depends on T  top_heat_boundary_conditions.jl:82-100 (emission OR the linear term; never a closed form)
  Tb = liq_T0 - liq_slope * S(i, j)         bottom_heat_boundary_conditions.jl:36-39 with a per-cell salinity
  the used fluxes                           Qu / Qb of the bare-ice step, Qui / Qbi of the layered one

A flux is a list of terms: a float, an ndarray (one value per cell), R.Emission or Linear(K, Ta, weighting) with K, Ta numbers or
arrays.  Without a Linear term and with a number for S the steps here give R's bits (tests/test_thermo_linear_ref.py)."""
from collections import namedtuple

import numpy as np

import thermo_flux_ref as R
from thermo_flux_ref import PHASE, jmax, jmin

Linear = namedtuple("Linear", "coefficient reference_temperature weighting")


def term_value(t, T, a):
    if isinstance(t, Linear):
        K, Ta = np.asarray(t.coefficient, dtype=np.float64), np.asarray(t.reference_temperature, dtype=np.float64)
        v = K * (T - Ta)
        if t.weighting == "concentration":
            return v * a
        if t.weighting == "ice_present":
            return np.where(a == 0, 0.0, v)
        assert t.weighting is None, t.weighting
        return v
    return R.term_value(t, T)


def getflux(terms, T, a):
    """terms[0] + (terms[1] + (... + terms[-1])), as R.getflux, with the concentration the Linear term weighs by."""
    if len(terms) == 0:
        return np.zeros_like(T)
    acc = np.array(np.broadcast_to(term_value(terms[-1], T, a), np.shape(T)), dtype=np.float64)
    for t in reversed(terms[:-1]):
        acc = term_value(t, T, a) + acc
    return acc


def depends_on_temperature(terms):
    return any(isinstance(t, (R.Emission, Linear)) for t in terms)


def bottom_temperature(S, like, p=PHASE):
    return np.array(np.broadcast_to(p["liq_T0"] - p["liq_slope"] * np.asarray(S, dtype=np.float64), like.shape), dtype=np.float64)


def slab_step(h, a, Tu, dt, top, bottom, flux_balance=True, k=2.0, rho=900.0, hc=0.05, S=0.0, ice_salinity=0.0, tol=1e-3,
              maxiters=1000, p=PHASE, iterations=None):
    """R.slab_step with the Linear term, S a number or per cell.  Returns a dict: h, aice, Tu, mf, q_top (Qu), q_bottom (Qb).
    iterations: a list that receives the secant's update counts (consolidated cells)."""
    h, a, Tu = (np.asarray(x, dtype=np.float64) for x in (h, a, Tu))
    consolidated = h >= hc
    Tb = bottom_temperature(S, h, p)
    with np.errstate(all="ignore"):
        if flux_balance:
            Tm = p["liq_T0"] - p["liq_slope"] * ice_salinity
            if depends_on_temperature(top):
                f = lambda T: getflux(top, T, a) - np.where(h <= 0, 0.0, -k * (T - Tb) / h)
                root, iters = R.secant(f, Tu, consolidated, tol, maxiters)
                if iterations is not None:
                    iterations.append(iters[consolidated])
            else:
                root = Tb - getflux(top, np.zeros_like(h), a) * h / k
            Tu = np.where(consolidated, jmin(root, Tm), Tb)
        Eb = rho * R.latent_heat(Tb, p)
        Eu = rho * R.latent_heat(Tu, p)
        Qi_fun = np.where(h <= 0, 0.0, -k * (Tu - Tb) / h)
        Qu = getflux(top, Tu, a)
        Qb = getflux(bottom, Tu, a)
        Qi = np.where(consolidated, Qi_fun, 0.0)
        wu = (Qu - Qi) / Eu
        wb = (Qi - Qb) / Eb
        h1, a1 = R.ice_volume_update(wu + wb, h, a, hc, dt)
        mf = rho * (h1 * a1 - h * a) / dt
    return dict(h=h1, aice=a1, Tu=Tu, mf=mf, q_top=Qu, q_bottom=Qb)


def layered_step(h, a, hs, Tus, dt, top, bottom, snowfall, flux_balance=True, ki=2.0, ks=0.31, rho=900.0, rho_s=330.0, hc=0.05,
                 S=0.0, ice_salinity=0.0, tol=1e-3, maxiters=1000, p=PHASE, iterations=None):
    """R.layered_step with the Linear term, S a number or per cell; its dict plus q_top (Qui) and q_bottom (Qbi)."""
    hin, an, hsn, Tus = (np.asarray(x, dtype=np.float64) for x in (h, a, hs, Tus))
    Ps = np.asarray(snowfall, dtype=np.float64)
    with np.errstate(all="ignore"):
        Vin, Vsn = hin * an, hsn * an
        consolidated = hin >= hc
        Tb = bottom_temperature(S, hin, p)
        Tm = p["liq_T0"] - p["liq_slope"] * ice_salinity
        Tm = np.where(hsn > 0, 0.0, Tm)
        Rr = hsn / ks + hin / ki
        if flux_balance:
            if depends_on_temperature(top):
                f = lambda T: getflux(top, T, an) - np.where(Rr <= 0, 0.0, (Tb - T) / Rr)
                root, iters = R.secant(f, Tus, consolidated, tol, maxiters)
                if iterations is not None:
                    iterations.append(iters[consolidated])
            else:
                root = Tb - getflux(top, np.zeros_like(Tus), an) * Rr
            Tus = np.where(consolidated, jmin(root, Tm), Tb)
        Ri, Rs = hin / ki, hsn / ks
        Rt = Rs + Ri
        Tsi = np.where(Rt <= 0, Tb, Tb + (Tus - Tb) * Ri / Rt)
        Qic = np.where(Rr <= 0, 0.0, (Tb - Tus) / Rr)
        Qis = np.where(consolidated, Qic, 0.0)
        Qui = getflux(top, Tus, an)
        Qui_per_ice = np.where(an > 0, Qui / an, 0.0)
        dQ = Qui_per_ice - Qis
        melt_energy = jmax(0.0, -dQ)
        Ls = p["L0"]
        cap = rho_s * Ls * hsn / dt
        Qs = jmin(melt_energy, cap)
        Gsm = Qs / (rho_s * Ls)
        riL = rho * Ls
        Qbi = getflux(bottom, Tus, an)
        alpha, beta = (Qui - Qbi) / riL, Qs / riL
        Cm = np.where(hin > 0, an / (2 * hin), 0.0)
        Cf = (1 - an) / hc if hc > 0 else np.zeros_like(an)
        Km, Kf = dt * Cm, dt * Cf
        eps = np.finfo(np.float64).eps
        Dm, Df = 1 - Km * beta, 1 - Kf * beta
        am = np.where(np.abs(Dm) > eps, (an + Km * alpha) / Dm, an + Km * alpha)
        af = np.where(np.abs(Df) > eps, (an + Kf * alpha) / Df, an + Kf * alpha)
        dtVm = alpha + beta * am
        atmp = np.where(dtVm < 0, am, af)
        Qeff = Qui + Qs * atmp
        Eb, Eu = rho * R.latent_heat(Tb, p), rho * R.latent_heat(Tsi, p)
        Qii = np.where(consolidated, np.where(hin <= 0, 0.0, -ki * (Tsi - Tb) / hin), 0.0)
        wu, wb = (Qeff - Qii) / Eu, (Qii - Qbi) / Eb
        hi1, a1 = R.ice_volume_update(wu + wb, hin, an, hc, dt)
        hsn = np.where(a1 > 0, hsn * an / a1, 0.0)
        Gsp = np.where(a1 > 0, Ps / rho_s, 0.0)
        hs1 = hsn + dt * (Gsp - Gsm)
        hs1 = jmax(0.0, hs1)
        rw = p["rho_l"]
        hf = hi1 * (1 - rho / rw) - hs1 * rho_s / rw
        dhs = np.where(hf < 0, -hf * rho / rho_s, 0.0)
        hsp = jmax(0.0, hs1 - dhs)
        dhs = hs1 - hsp
        hi1 = hi1 + dhs * rho_s / rho
        hs1 = np.where(a1 <= 0, 0.0, hsp)
        Pabs = rho_s * Gsp * a1
        return dict(h=hi1, aice=a1, hs=hs1, mf_ice=rho * (hi1 * a1 - Vin) / dt, mf_snow=rho_s * (hs1 * a1 - Vsn) / dt - Pabs,
                    mf_int=Pabs, tu_ice=Tsi, tu_snow=Tus, q_top=Qui, q_bottom=Qbi)


# ---- the reference's energy-conservation test, per cell (test/test_energy_conservation.jl) ------------------------------------------

def energy(h, a, hs, rho=900.0, rho_s=330.0, L0=PHASE["L0"]):
    """E = -aice L0 (rho_i h + rho_s hs)"""
    return -a * L0 * (rho * h + rho_s * hs)


def closure_state(n=64, seed=7, partial=False, snow=False, melting=False):
    """The 64-cell state of the energy-closure tests: every cell differs in Ta, Qb, h, hs and (partial) aice.  Freezing: cold air and
    a small ocean flux; melting: warm air, so that the surface sits at the melting point and the ice (and snow) thins."""
    rng = np.random.default_rng(seed)
    h = 0.5 + 1.5 * rng.random(n)
    a = 0.3 + 0.6 * rng.random(n) if partial else np.ones(n)
    hs = 0.05 + 0.25 * rng.random(n) if snow else np.zeros(n)
    Ta = (2.0 + 8.0 * rng.random(n)) if melting else (-25.0 + 15.0 * rng.random(n))
    Qb = -(10.0 + 20.0 * rng.random(n)) if melting else -(1.0 + 9.0 * rng.random(n))      # (the reference's -20 / -5)
    return dict(h=h, a=a, hs=hs, Ta=Ta, Qb=Qb)


def closure_residual(E0, E1, q_top, q_bottom, intercepted, dt, L0=PHASE["L0"]):
    """One step's |E1 - E0 - expected| / max(|E0|, |E1|, |expected|, 1) per cell, expected = (-Q_top + Q_bottom - L0 P_intercepted) dt
    with the fluxes that step used (test_energy_conservation.jl:70-78; there P_intercepted is the snowfall where aice > 0)."""
    expected = (-q_top + q_bottom - L0 * intercepted) * dt
    scale = np.maximum(np.maximum(np.abs(E0), np.abs(E1)), np.maximum(np.abs(expected), 1.0))
    return np.abs((E1 - E0) - expected) / scale


def closure_run(state, snow, precipitation, nsteps, dt=600.0, K=1e-3 * 1.225 * 1004 * 5, extra_top=(), step=None):
    """The reference's loop on every cell of `state`: the top flux (extra terms..., Linear(K, Ta, "concentration")), the bottom flux
    Qb per cell, S = 0.  step(r, top, bottom, Ps) -> dict advances
    the state (default: the restatement); returns the largest residual per cell."""
    h, a, hs, Ta, Qb = (state[k].copy() for k in ("h", "a", "hs", "Ta", "Qb"))
    top = list(extra_top) + [Linear(K, Ta, "concentration")]
    bottom = [Qb]
    Ps = 6e-5 if precipitation else 0.0
    Tu = np.zeros_like(h)
    worst = np.zeros_like(h)
    for n in range(nsteps):
        E0 = energy(h, a, hs)
        if step is not None:
            r = step(dict(h=h, a=a, hs=hs, Tu=Tu), top, bottom, Ps)
        elif snow:
            r = layered_step(h, a, hs, Tu, dt, top, bottom, Ps)
            r["Tu"] = r["tu_snow"]
        else:
            r = slab_step(h, a, Tu, dt, top, bottom)
            r.update(hs=np.zeros_like(h), mf_int=np.zeros_like(h))
        h, a, hs, Tu = r["h"], r["aice"], r["hs"], r["Tu"]
        E1 = energy(h, a, hs)
        worst = np.maximum(worst, closure_residual(E0, E1, r["q_top"], r["q_bottom"], r["mf_int"], dt))
    return worst
