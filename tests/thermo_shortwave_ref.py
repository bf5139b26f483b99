"""Test-side restatement of the thermodynamic steps with the SHORTWAVE top-flux term (absorbed shortwave radiation with a stepped,
temperature-dependent albedo) in NumPy fp64.  It builds on tests/thermo_linear_ref.py (T), statement for statement: T's term values,
secant (R's), latent heat, ice_volume_update, jmin / jmax and bottom temperature are used as they are; what is restated here is what
T's steps cannot express --

  the term  alpha = (T < threshold) ? cold : warm      the closure of examples/arctic_basin_seasonal_cycle.jl:106-110, strict <
            Q     = (F * (1 - alpha)) * w              in exactly this order; w as for T.Linear:
                                                         weighting None             no product by w
                                                         "concentration"            w = aice at the start of the step
                                                         "ice_present"              (aice == 0) ? 0 : F * (1 - alpha)
  the snow triple                             the layered step takes it in cells whose hs at the start of the step is > 0
  the secant whenever the top depends on T    emission, the linear term OR the shortwave term; never a closed form
  the albedo a step used                      alpha at the temperature the step solved (capped) or was given

A flux is a list of terms: a float, an ndarray, R.Emission, T.Linear or Shortwave(flux, albedo, snow_albedo, weighting) with flux a
number or an array and the albedos Albedo(cold, warm, threshold) (snow_albedo None: the ice triple serves both).  Without a Shortwave
term the steps here give T's bits (tests/test_thermo_shortwave_ref.py)."""
from collections import namedtuple

import numpy as np

import thermo_flux_ref as R
import time_series_ref
import thermo_linear_ref as T
from thermo_flux_ref import PHASE, jmax, jmin

Albedo = namedtuple("Albedo", "cold warm threshold")
Shortwave = namedtuple("Shortwave", "flux albedo snow_albedo weighting")
SEMTNER = Albedo(0.75, 0.64, -0.1)


def triple(t, snowy):
    """(cold, warm, threshold) per cell: the snow triple where `snowy` (and one is given), the ice triple elsewhere."""
    if t.snow_albedo is None:
        return t.albedo
    return Albedo(*(np.where(snowy, s, i) for s, i in zip(t.snow_albedo, t.albedo)))


def albedo(t, Ts, snowy):
    cold, warm, thr = triple(t, snowy)
    return np.where(Ts < thr, cold, warm)


def term_value(t, Ts, a, snowy, variant=None):
    """variant: None, or a deliberately different statement the tests use to show that they can tell --
    "associate": F * ((1 - alpha) * w) instead of (F * (1 - alpha)) * w;  "swap": cold and warm exchanged."""
    if isinstance(t, Shortwave):
        F = np.asarray(t.flux, dtype=np.float64)
        alpha = albedo(t, Ts, snowy)
        if variant == "swap":
            cold, warm, thr = triple(t, snowy)
            alpha = np.where(Ts < thr, warm, cold)
        if variant == "associate" and t.weighting == "concentration":
            return F * ((1 - alpha) * a)
        v = F * (1 - alpha)
        if t.weighting == "concentration":
            return v * a
        if t.weighting == "ice_present":
            return np.where(a == 0, 0.0, v)
        assert t.weighting is None, t.weighting
        return v
    return T.term_value(t, Ts, a)


def getflux(terms, Ts, a, snowy=False, variant=None):
    """terms[0] + (terms[1] + (... + terms[-1])), as T.getflux, with what the Shortwave term reads of a cell."""
    if len(terms) == 0:
        return np.zeros_like(Ts)
    acc = np.array(np.broadcast_to(term_value(terms[-1], Ts, a, snowy, variant), np.shape(Ts)), dtype=np.float64)
    for t in reversed(terms[:-1]):
        acc = term_value(t, Ts, a, snowy, variant) + acc
    return acc


def getflux_left(terms, Ts, a, snowy=False):
    """The same terms summed LEFT-nested, ((t0 + t1) + t2) + ...: what the library does NOT compute."""
    acc = np.array(np.broadcast_to(term_value(terms[0], Ts, a, snowy), np.shape(Ts)), dtype=np.float64)
    for t in terms[1:]:
        acc = acc + term_value(t, Ts, a, snowy)
    return acc


def shortwave_of(terms):
    found = [t for t in terms if isinstance(t, Shortwave)]
    assert len(found) <= 1
    return found[0] if found else None


def depends_on_temperature(terms):
    return T.depends_on_temperature(terms) or shortwave_of(terms) is not None


def slab_step(h, a, Tu, dt, top, bottom, flux_balance=True, k=2.0, rho=900.0, hc=0.05, S=0.0, ice_salinity=0.0, tol=1e-3,
              maxiters=1000, p=PHASE, iterations=None, variant=None):
    """T.slab_step with the Shortwave term.  Returns T's dict plus albedo (None without the term).  The bare-ice step has no snow: the
    ice triple holds everywhere."""
    h, a, Tu = (np.asarray(x, dtype=np.float64) for x in (h, a, Tu))
    consolidated = h >= hc
    Tb = T.bottom_temperature(S, h, p)
    with np.errstate(all="ignore"):
        if flux_balance:
            Tm = p["liq_T0"] - p["liq_slope"] * ice_salinity
            if depends_on_temperature(top):
                f = lambda Ts: getflux(top, Ts, a, False, variant) - np.where(h <= 0, 0.0, -k * (Ts - Tb) / h)
                root, iters = R.secant(f, Tu, consolidated, tol, maxiters)
                if iterations is not None:
                    iterations.append(iters[consolidated])
            else:
                root = Tb - getflux(top, np.zeros_like(h), a, False, variant) * h / k
            Tu = np.where(consolidated, jmin(root, Tm), Tb)
        Eb = rho * R.latent_heat(Tb, p)
        Eu = rho * R.latent_heat(Tu, p)
        Qi_fun = np.where(h <= 0, 0.0, -k * (Tu - Tb) / h)
        Qu = getflux(top, Tu, a, False, variant)
        Qb = getflux(bottom, Tu, a)
        Qi = np.where(consolidated, Qi_fun, 0.0)
        wu = (Qu - Qi) / Eu
        wb = (Qi - Qb) / Eb
        h1, a1 = R.ice_volume_update(wu + wb, h, a, hc, dt)
        mf = rho * (h1 * a1 - h * a) / dt
        sw = shortwave_of(top)
        alpha = None if sw is None else np.array(np.broadcast_to(albedo(sw, Tu, False), h.shape), dtype=np.float64)
    return dict(h=h1, aice=a1, Tu=Tu, mf=mf, q_top=Qu, q_bottom=Qb, albedo=alpha)


def layered_step(h, a, hs, Tus, dt, top, bottom, snowfall, flux_balance=True, ki=2.0, ks=0.31, rho=900.0, rho_s=330.0, hc=0.05,
                 S=0.0, ice_salinity=0.0, tol=1e-3, maxiters=1000, p=PHASE, iterations=None, variant=None):
    """T.layered_step with the Shortwave term; its dict plus albedo.  snowy = hs > 0 at the start of the step, the condition under which
    Tm = 0."""
    hin, an, hsn, Tus = (np.asarray(x, dtype=np.float64) for x in (h, a, hs, Tus))
    Ps = np.asarray(snowfall, dtype=np.float64)
    with np.errstate(all="ignore"):
        Vin, Vsn = hin * an, hsn * an
        consolidated = hin >= hc
        snowy = hsn > 0
        Tb = T.bottom_temperature(S, hin, p)
        Tm = p["liq_T0"] - p["liq_slope"] * ice_salinity
        Tm = np.where(hsn > 0, 0.0, Tm)
        Rr = hsn / ks + hin / ki
        if flux_balance:
            if depends_on_temperature(top):
                f = lambda Ts: getflux(top, Ts, an, snowy, variant) - np.where(Rr <= 0, 0.0, (Tb - Ts) / Rr)
                root, iters = R.secant(f, Tus, consolidated, tol, maxiters)
                if iterations is not None:
                    iterations.append(iters[consolidated])
            else:
                root = Tb - getflux(top, np.zeros_like(Tus), an, snowy, variant) * Rr
            Tus = np.where(consolidated, jmin(root, Tm), Tb)
        Ri, Rs = hin / ki, hsn / ks
        Rt = Rs + Ri
        Tsi = np.where(Rt <= 0, Tb, Tb + (Tus - Tb) * Ri / Rt)
        Qic = np.where(Rr <= 0, 0.0, (Tb - Tus) / Rr)
        Qis = np.where(consolidated, Qic, 0.0)
        Qui = getflux(top, Tus, an, snowy, variant)
        Qui_per_ice = np.where(an > 0, Qui / an, 0.0)
        dQ = Qui_per_ice - Qis
        melt_energy = jmax(0.0, -dQ)
        Ls = p["L0"]
        cap = rho_s * Ls * hsn / dt
        Qs = jmin(melt_energy, cap)
        Gsm = Qs / (rho_s * Ls)
        riL = rho * Ls
        Qbi = getflux(bottom, Tus, an)
        alpha_, beta = (Qui - Qbi) / riL, Qs / riL
        Cm = np.where(hin > 0, an / (2 * hin), 0.0)
        Cf = (1 - an) / hc if hc > 0 else np.zeros_like(an)
        Km, Kf = dt * Cm, dt * Cf
        eps = np.finfo(np.float64).eps
        Dm, Df = 1 - Km * beta, 1 - Kf * beta
        am = np.where(np.abs(Dm) > eps, (an + Km * alpha_) / Dm, an + Km * alpha_)
        af = np.where(np.abs(Df) > eps, (an + Kf * alpha_) / Df, an + Kf * alpha_)
        dtVm = alpha_ + beta * am
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
        sw = shortwave_of(top)
        alb = None if sw is None else np.array(np.broadcast_to(albedo(sw, Tus, snowy), hin.shape), dtype=np.float64)
        return dict(h=hi1, aice=a1, hs=hs1, mf_ice=rho * (hi1 * a1 - Vin) / dt, mf_snow=rho_s * (hs1 * a1 - Vsn) / dt - Pabs,
                    mf_int=Pabs, tu_ice=Tsi, tu_snow=Tus, q_top=Qui, q_bottom=Qbi, albedo=alb)


# ---- inputs the CPU and the GPU tests share ---------------------------------------------------------------------------------------

SIGMA = 5.67e-8 * 1.02      # the example's 1.02 sigma


def random_state(n=200_000, seed=3):
    """The draw the stepped form was tried on before it was offered: h 0.05-4 m, shortwave 0-320 W m^-2 and other fluxes 120-330 W m^-2
    downward (negative), emission with the example's 1.02 sigma, Tu- in -30...0, Tb = -0.054 S with S in 30...35, aice = 1."""
    rng = np.random.default_rng(seed)
    h = rng.uniform(0.05, 4.0, n)
    S = rng.uniform(30, 35, n)
    Tu = rng.uniform(-30, 0, n)
    Fsw = -rng.uniform(0, 320, n)
    Fin = -rng.uniform(120, 330, n)
    return dict(h=h, a=np.ones(n), S=S, Tu=Tu, Fsw=Fsw, Fin=Fin)


def random_top(s, albedo=SEMTNER, weighting=None):
    return [Shortwave(s["Fsw"], albedo, None, weighting), s["Fin"], R.Emission(1.0, SIGMA, 273.15)]


def branch_counts(r, s, top, tol=1e-3, hc=0.05, ice_salinity=0.0, p=PHASE):
    """Cells of a slab step's result by the branch their surface temperature took: unconsolidated; capped at Tm; root on the cold
    branch; root on the warm branch below Tm; and, among the last two, within tol of the threshold (the jump)."""
    sw = shortwave_of(top)
    thr = sw.albedo.threshold
    Tm = p["liq_T0"] - p["liq_slope"] * ice_salinity
    cons = s["h"] >= hc
    capped = cons & (r["Tu"] == Tm) & (thr <= Tm)
    cold = cons & (r["Tu"] < thr)
    warm = cons & (r["Tu"] >= thr) & (r["Tu"] < Tm)
    jump = cons & (np.abs(r["Tu"] - thr) < tol)
    return dict(unconsolidated=int((~cons).sum()), capped=int(capped.sum()), cold=int(cold.sum()), warm=int(warm.sum()),
                jump=int(jump.sum()))


# ---- the example's column (examples/arctic_basin_seasonal_cycle.jl, Semtner 1976) ----------------------------------------------------

DAY = 86400.0
MONTH_DAYS = 30
YEAR = 12 * MONTH_DAYS * DAY
MONTH_TIMES = np.arange(15, 360, 30) * DAY
# Semtner (1976) Table 1, after Fletcher (1965): monthly totals in 1e4 kcal m^-2, downward
_TABLE = dict(shortwave=[0, 0, 1.9, 9.9, 17.7, 19.2, 13.6, 9.0, 3.7, 0.4, 0, 0],
              longwave=[10.4, 10.3, 10.3, 11.6, 15.1, 18.0, 19.1, 18.7, 16.5, 13.9, 11.2, 10.9],
              sensible=[1.18, 0.76, 0.72, 0.29, -0.45, -0.39, -0.30, -0.40, -0.17, 0.1, 0.56, 0.79],
              latent=[0, -0.02, -0.03, -0.09, -0.46, -0.70, -0.64, -0.66, -0.39, -0.19, -0.01, -0.01])
# ... as W m^-2, positive upward: 4184 J per kcal over a 30-day month
MONTHLY = {k: (-np.array(v, dtype=np.float64) * 1e4) * (4184 / (MONTH_DAYS * DAY)) for k, v in _TABLE.items()}
# at most one ARRAY term per side: longwave, sensible and latent are summed into one series (linear interpolation commutes with the sum)
MONTHLY["others"] = MONTHLY["longwave"] + (MONTHLY["sensible"] + MONTHLY["latent"])


def forcing_at(name, t):
    """MONTHLY[name] at clock time t: Cyclical indexing over the 360-day year with linear interpolation, by tests/time_series_ref.py."""
    return float(time_series_ref.at(MONTH_TIMES, MONTHLY[name], time_series_ref.CYCLICAL, YEAR, t))


def column_top(t, albedo=SEMTNER):
    """The example's top heat flux at clock time t: (shortwave, longwave + sensible + latent, emission with 1.02 sigma)."""
    return [Shortwave(forcing_at("shortwave", t), albedo, None, None), forcing_at("others", t), R.Emission(1.0, SIGMA, 273.15)]
