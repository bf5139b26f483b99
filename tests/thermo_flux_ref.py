"""Test-side restatement of the thermodynamic steps with per-cell heat fluxes, RadiativeEmission and the surface-temperature
solve, in NumPy fp64 (every operation rounds once: no contraction), restated from the reference and not from the library:

  getflux (Number, array, Tuple, RadiativeEmission)   SeaIceThermodynamics/HeatBoundaryConditions/boundary_fluxes.jl:8-22, 98-127
  thermodynamic_tendency with the surface solve        slab_thermodynamics_tendencies.jl:74-135
  top_surface_temperature (SecantMethod(Tu- + 1, Tu-)) top_heat_boundary_conditions.jl:82-100 (RootSolvers' loop as recalled in
                                                       include/csi.h: RootSolvers is not vendored)
  ice_volume_update                                    thermodynamic_time_step.jl:304-324, 358-370
  _layered_thermodynamic_time_step!                    thermodynamic_time_step.jl:131-298
  snow_accumulation, snow_ice_formation                thermodynamic_time_step.jl:328-353

Every function works elementwise on arrays of cells.  The secant keeps a per-cell "still iterating" mask, so each cell sees the
same operations as one thread of a per-cell loop.  (T + T_r)^4 is (x * x) * (x * x), as include/csi.h states.

A flux is a list of terms: a float, an ndarray (one value per cell) or Emission(eps, sigma, Tr)."""
from collections import namedtuple

import numpy as np

Emission = namedtuple("Emission", "emissivity stefan_boltzmann_constant reference_temperature")
EMISSION = Emission(1.0, 5.67e-8, 273.15)

PHASE = dict(L0=334e3, T0=0.0, rho_l=999.8, c_l=4186.0, rho_pure=917.0, c_i=2000.0, liq_slope=0.054, liq_T0=0.0)


def jmax(a, b):
    """Julia's max for floats: NaN if either is NaN."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    return np.where(np.isnan(a) | np.isnan(b), a + b, np.where(a < b, b, a))


def jmin(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    return np.where(np.isnan(a) | np.isnan(b), a + b, np.where(b < a, b, a))


def term_value(t, T):
    if isinstance(t, Emission):
        x = T + t.reference_temperature
        x2 = x * x
        return t.emissivity * t.stefan_boltzmann_constant * (x2 * x2)
    return np.asarray(t, dtype=np.float64)


def getflux(terms, T):
    """A Tuple sums as terms[0] + (terms[1] + (... + terms[-1])) (boundary_fluxes.jl:15-22); one term is itself."""
    if len(terms) == 0:
        return np.zeros_like(T)
    acc = np.array(np.broadcast_to(term_value(terms[-1], T), np.shape(T)), dtype=np.float64)
    for t in reversed(terms[:-1]):
        acc = term_value(t, T) + acc
    return acc


def has_emission(terms):
    return any(isinstance(t, Emission) for t in terms)


def secant(f, Tu_prev, active, tol=1e-3, maxiters=1000):
    """find_zero(f, SecantMethod(Tu- + 1, Tu-)): per cell at most maxiters updates, stop when |x1 - x0| < tol, root = x1.
    Only the cells of `active` iterate; the others return Tu- (unused by the callers)."""
    x0 = Tu_prev + 1.0
    x1 = Tu_prev.copy()
    y0, y1 = f(x0), f(x1)
    live = active.copy()
    iters = np.zeros(Tu_prev.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for _ in range(maxiters):
            if not live.any():
                break
            dx, dy = x1 - x0, y1 - y0
            nx0, ny0 = x1, y1
            nx1 = x1 - y1 * dx / dy
            ny1 = f(nx1)
            x0, y0 = np.where(live, nx0, x0), np.where(live, ny0, y0)
            x1, y1 = np.where(live, nx1, x1), np.where(live, ny1, y1)
            iters += live
            live = live & ~(np.abs(nx1 - nx0) < tol)
    return x1, iters


def latent_heat(T, p=PHASE):
    return p["L0"] + (p["rho_l"] * p["c_l"] / p["rho_pure"] - p["c_i"]) * (T - p["T0"])


def ice_volume_update(dtV, hn, an, hc, dt):
    with np.errstate(all="ignore"):
        V1 = hn * an + dt * dtV
        V1 = jmax(0.0, V1)
        dtV = (V1 - hn * an) / dt
        xf = (1 - an) / hc * dtV
        xm = an / (2 * hn) * dtV
        daf = np.where(dtV >= 0, xf, np.copysign(0.0, xf))      # x * Bool: false is a strong zero
        dam = np.where(dtV < 0, xm, np.copysign(0.0, xm))
        ap = an + dt * (daf + dam)
        ap = jmax(0.0, ap)
        hp = V1 / ap
        hp = np.where(ap <= 0, 0.0, hp)
        ap = np.where(dtV == 0, an, ap)
        hp = np.where(dtV == 0, hn, hp)
        ap = np.where(hp == 0, 0.0, ap)
        hp = np.where(ap == 0, 0.0, hp)
        return np.where(ap > 1, hp * ap, hp), np.where(ap > 1, 1.0, ap)


def surface_temperature(top, Tb, Tm, R, consolidated, Tu_prev, tol=1e-3, maxiters=1000):
    """MeltingConstrainedFluxBalance: the root of Qx(T) - Qi(T), Qi(T) = (Tb - T) / R (0 where R <= 0), capped at Tm; Tb where the
    ice is not consolidated.  Without emission Qx does not depend on T and the root is Tb - Qx R (the library's closed form)."""
    with np.errstate(all="ignore"):
        if has_emission(top):
            f = lambda T: getflux(top, T) - np.where(R <= 0, 0.0, (Tb - T) / R)
            root, _ = secant(f, Tu_prev, consolidated, tol, maxiters)
        else:
            root = Tb - getflux(top, np.zeros_like(Tu_prev)) * R
    return np.where(consolidated, jmin(root, Tm), Tb)


def slab_step(h, a, Tu, dt, top, bottom, flux_balance=True, k=2.0, rho=900.0, hc=0.05, S=0.0, ice_salinity=0.0,
              tol=1e-3, maxiters=1000, p=PHASE):
    """Bare-ice step (_ice_thermodynamic_time_step!).  Tu: Tu- under the flux balance, the prescribed temperature otherwise.
    Returns h, a, Tu (the solved temperature under the flux balance) and the ice mass flux."""
    h, a, Tu = (np.asarray(x, dtype=np.float64) for x in (h, a, Tu))
    consolidated = h >= hc
    Tb = p["liq_T0"] - p["liq_slope"] * S
    Tb = np.full_like(h, Tb)
    with np.errstate(all="ignore"):
        if flux_balance:
            Tm = p["liq_T0"] - p["liq_slope"] * ice_salinity
            # slab_internal_heat_flux: -k (T - Tb) / h = (Tb - T) / R only up to rounding, so the slab's own Qi is used here
            if has_emission(top):
                f = lambda T: getflux(top, T) - np.where(h <= 0, 0.0, -k * (T - Tb) / h)
                root, _ = secant(f, Tu, consolidated, tol, maxiters)
            else:
                root = Tb - getflux(top, np.zeros_like(h)) * h / k
            Tu = np.where(consolidated, jmin(root, Tm), Tb)
        Eb = rho * latent_heat(Tb, p)
        Eu = rho * latent_heat(Tu, p)
        Qi_fun = np.where(h <= 0, 0.0, -k * (Tu - Tb) / h)
        Qu = getflux(top, Tu)
        Qb = getflux(bottom, Tu)
        Qi = np.where(consolidated, Qi_fun, 0.0)
        wu = (Qu - Qi) / Eu
        wb = (Qi - Qb) / Eb
        h1, a1 = ice_volume_update(wu + wb, h, a, hc, dt)
        mf = rho * (h1 * a1 - h * a) / dt
    return h1, a1, Tu, mf


def layered_step(h, a, hs, Tus, dt, top, bottom, snowfall, flux_balance=True, ki=2.0, ks=0.31, rho=900.0, rho_s=330.0, hc=0.05,
                 S=0.0, ice_salinity=0.0, tol=1e-3, maxiters=1000, p=PHASE):
    """Snow on ice (_layered_thermodynamic_time_step!).  Tus: Tu- of the snow surface under the flux balance, the prescribed
    temperature otherwise.  snowfall: a number or one value per cell.  Returns a dict of the outputs."""
    hin, an, hsn, Tus = (np.asarray(x, dtype=np.float64) for x in (h, a, hs, Tus))
    Ps = np.asarray(snowfall, dtype=np.float64)
    with np.errstate(all="ignore"):
        Vin, Vsn = hin * an, hsn * an
        consolidated = hin >= hc
        Tb = np.full_like(hin, p["liq_T0"] - p["liq_slope"] * S)
        Tm = p["liq_T0"] - p["liq_slope"] * ice_salinity
        Tm = np.where(hsn > 0, 0.0, Tm)
        R = hsn / ks + hin / ki
        if flux_balance:
            Tus = surface_temperature(top, Tb, Tm, R, consolidated, Tus, tol, maxiters)
        Ri, Rs = hin / ki, hsn / ks
        Rt = Rs + Ri
        Tsi = np.where(Rt <= 0, Tb, Tb + (Tus - Tb) * Ri / Rt)
        Qic = np.where(R <= 0, 0.0, (Tb - Tus) / R)
        Qis = np.where(consolidated, Qic, 0.0)
        Qui = getflux(top, Tus)
        Qui_per_ice = np.where(an > 0, Qui / an, 0.0)
        dQ = Qui_per_ice - Qis
        melt_energy = jmax(0.0, -dQ)
        Ls = p["L0"]
        cap = rho_s * Ls * hsn / dt
        Qs = jmin(melt_energy, cap)
        Gsm = Qs / (rho_s * Ls)
        riL = rho * Ls
        Qbi = getflux(bottom, Tus)
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
        Eb, Eu = rho * latent_heat(Tb, p), rho * latent_heat(Tsi, p)
        Qii = np.where(consolidated, np.where(hin <= 0, 0.0, -ki * (Tsi - Tb) / hin), 0.0)
        wu, wb = (Qeff - Qii) / Eu, (Qii - Qbi) / Eb
        hi1, a1 = ice_volume_update(wu + wb, hin, an, hc, dt)
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
                    mf_int=Pabs, tu_ice=Tsi, tu_snow=Tus)
