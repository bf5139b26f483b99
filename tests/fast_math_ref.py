"""High-precision per-cell restatement of the REFERENCE's EVP arithmetic, and the derived error bounds of the FAST arithmetic
(csrc/evp_fast_math.h) against it.  CPU only; shared by tests/test_fast_math_ref.py and tests/test_gpu_fast_math.py.

The formulas are the reference's, not the rearranged FAST ones (paths relative to the reference's src/):
  viscosities               Rheologies/elasto_visco_plastic_rheology.jl:236-273
  replacement pressure      :282-289
  stresses and alpha        :294-354
  SemiImplicitStress        SeaIceDynamics/sea_ice_external_stress.jl:176-202
  velocity tendency         SeaIceDynamics/momentum_tendencies_kernel_functions.jl:11-74
  semi-implicit update      SeaIceDynamics/split_explicit_momentum_equations.jl:197-264 (with and without free drift)

Arithmetic: the standard library's `decimal` at 80 significant digits (265 bits; a double converts exactly, every operation and the
square root round once at 80 digits).  It is always there, so nothing is skipped where mpmath is missing, and it is several times faster
than mpmath at this precision.  Results are `Decimal`; `None` stands for NaN.

u = 2^-53 throughout.  "x has k u" means |computed x - exact x| <= k u |exact x| to first order; the constants below carry a few
units of slack for the second-order terms ((1 + 200 u)^2 - 1 - 400 u < 1e-27).

DERIVED CONSTANTS (forward error analysis of evp_fast_math.h as written; NOT fitted to any measurement)
--------------------------------------------------------------------------------------------------------
Primitives, one Newton / Goldschmidt step on a hardware seed with correctly rounded fused multiply-adds (the derivation is in
tests/test_fast_math_ref.py::test_refinement_step_bounds_by_exact_emulation, which also checks it by exact rational emulation):
  rcp       relative error <= e^2 + 2 u,        e = |seed x - 1|
  rsqrt     relative error <= 1.5 e^2 + 2 u,    e = |seed sqrt(x) - 1|
  sqrt_fast relative error <= 1.5 e^2 + 2 u
Under the cap e <= SEED_CAP = 2^-23 (2^-46 = 128 u):  RCP_U = 130 u,  RSQ_U = 194 u.  sqrt_rsqrt's s is within 1 ulp of the correctly
rounded root (asserted on the GPU), so within 1.5 ulp <= 3 u of the exact one: SQRT_S_U = 3.

stress_update_r, with R = RSQ_U, C = RCP_U:
  dc = e11 + e22, tc = e11 - e22                                  1 u each (inputs are exact)
  sc2 = fma(tc, tc, 4 e12c^2)    sum of positives                 tc^2: 2 u, e12c^2: 1 u, fma: 1 u            -> 3 u
  x  = fma(dc, dc, sc2 em2)      sum of positives                 dc^2: 2 u, sc2 em2: 4 u, fma: 1 u           -> 5 u
       max(x, Dmin^2): Dmin^2 has 1 u; the reference's max(sqrt(x), Dmin) is the same function of exact x     -> 5 u
  1/Delta = rsqrt(x)                                              5/2 + R                                     -> R + 2.5
  2 zeta = P rsqrt(x)                                                                                         -> R + 3.5
  P_r = P rcp(fma(Dmin, 1/Delta, 1)): the sum 1 + Dmin/Delta has (R + 2.5)/2 + 1 (the term is at most half the sum)
                                                                  + C + 1                                     -> R/2 + C + 3.25
  2 eta = 2 zeta em2                                                                                          -> R + 4.5
  A = (2 zeta hk1) dc:  hk1 = 0.5 (1 - em2) has 1 u, two products, dc 1 u                                     -> R + 7.5
  bulk = fma(., dc, -P_r / 2): 1 u of |A| + |B|;   sigma' = fma(2 eta, e, bulk): 1 u of |T| + |A| + |B|
  with T = 2 eta e, A = (zeta - eta) div, B = P_r / 2 and N = |T| + |A| + |B|:
       |error of sigma'| <= u ((R + 5.5)|T| + (R + 9.5)|A| + (R/2 + C + 5.25)|B|) <= SN u N,  SN = max(R + 9.5, R/2 + C + 5.25)
  gamma^2 = 2 zeta hkc rcp(m):                                    (R + 3.5) + 1 + C + 1                       -> R + C + 5.5
       the clamps are continuous and monotone, so the bound passes through them; on a plateau gamma^2 is the exact alpha+-^2
  alpha = s of sqrt_rsqrt:                                        (R + C + 5.5)/2 + SQRT_S_U                  =: K_ALPHA
  1/gamma = rs = rsqrt(gamma^2):                                  (R + C + 5.5)/2 + R                         =: W
  sigma_new = fma(sigma' - sigma, 1/gamma, sigma):  d = sigma' - sigma has SN u N + 1 u |d|, |d| <= N + |sigma|;
       |error| <= u [ (SN N + (1 + W)(N + |sigma|)) / gamma + |sigma| + (N + |sigma|) / gamma ]
               <= (SN + W + 2) u (|sigma| + (N + |sigma|) / gamma)                                            =: K_SIGMA
  With R = 194, C = 130:  SN = 232.25, W = 358.75, K_SIGMA = 593 -> 594, K_ALPHA = 167.75 -> 168.
  (The corner's sigma12 has fewer operations: 2 eta_f e12 has R + 5.5.)  Where the ice mass is <= 0 the weight is exactly 0 and
  fma(d, 0, sigma) = sigma bit for bit for every finite d.

ext_stress (kind 3):  d1 = we - w, d2 = webar - wbar: 1 u each;  n2 = fma(d1, d1, d2 d2): 2 u, 3 u, +1                -> 4 u
  n = sqrt_fast(max(n2, DBL_MIN)): 2 + R;  im = rhoCd n: + 1;  ex = im we: + 1                                        K_EXT = R + 4 = 198
  (rhoCd is the caller's product rho_e C_D, an input.)  Where n2 < DBL_MIN the result is rhoCd sqrt_fast(DBL_MIN) instead of the
  reference's rhoCd sqrt(n2) < rhoCd 1.5e-154: an absolute distance of at most rhoCd 1.4917e-154 (1 + (R + 1) u).

vel_update_avg:  rm = rcp(mi): C;  rai = rm ai: C + 1
  G = fma(wn - w, rdt, fma(div, rm, fma(exb - ext, rai, cor))):  terms t1 = (wn - w) rdt: 1 + 1 (rdt = 1/dt rounded) = 2,
       t2 = div rm: C, t3 = (exb - ext) rai: C + 2, cor: exact; each of the three fmas adds 1 u of its partial sum
       |error of G| <= (C + 5) u SG,  SG = |t1| + |t2| + |t3| + |cor|
  tau_i = (imb - imt) rai: C + 3
  numerator  fma(dt, G, abar w):  (C + 5) u dt SG + 1 u |abar w| + 1 u N  <= (C + 6) u N,   N = |abar w| + dt SG
  denominator fma(dt, tau_i, abar), both terms >= 0 (imb >= imt, the domain of the tests):  (C + 4) u D;  rcp: + C;  product: + 1
  |error of wD| <= ((C + 6) + (2 C + 5)) u N / D = (3 C + 11) u N / D                                              K_VEL = 401 -> 402
"""
import decimal
from decimal import Decimal as D

import numpy as np

U = 2.0 ** -53
SEED_CAP = 2.0 ** -23
RCP_U = 130            # (2^-23)^2 / u + 2
RSQ_U = 194            # 1.5 (2^-23)^2 / u + 2
SQRT_S_U = 3
K_SIGMA = 594
K_ALPHA = 168
K_EXT = 198
K_VEL = 402
DBL_MIN = 2.2250738585072014e-308
EPS64 = 2.220446049250313e-16

CTX = decimal.Context(prec=80, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN, traps=[decimal.InvalidOperation, decimal.DivisionByZero,
                                                                                  decimal.Overflow])
DU = D(U)


def hp():
    """`with hp():` -- the 80-digit context."""
    return decimal.localcontext(CTX)


def dec(x):
    """a double, exactly (a Decimal passes through: inputs the caller formed in high precision)"""
    return x if isinstance(x, D) else D(float(x))


def stress_constants(ecc=2.0, Dmin=2e-9, amin=50.0, amax=300.0, pressure_kind=0):
    """The constants as the library forms them (csi_launch.hip fast_coef): em2 = (1 / e)^2 and hk1 = 0.5 (1 - em2) in double."""
    ie = 1.0 / ecc
    em2 = ie * ie
    return dict(em2=em2, Dmin=float(Dmin), amin=float(amin), amax=float(amax), hk1=0.5 * (1.0 - em2), pressure_kind=int(pressure_kind))


def stress_cell(k, e11c, e22c, e12f, e11f, e22f, e12c, Pc, Pf, mc, mf, hkc, hkf, s11, s22, s12, em2=None, hk1=None, hkc_scale=None):
    """One stress index of the reference: evp:236-273 (viscosities), :282-289 (pressure), :294-354 (stresses, alpha), on exact inputs.

    hkc, hkf are HALF of c_alpha dt / Az at the cell / corner (what evp_fast_math.h takes), so the reference's c_alpha dt / Az is 2 hkc.
    em2: e^-2 (default: k's double, which is what the reference computes); hk1: the factor (1 - e^-2) / 2 of zeta - eta (default: exact
    from em2); hkc_scale: a factor on hkc.  These three exist for the tests' perturbed evaluations.
    Returns (s11, s22, s12, alpha, N11, N22, N12, gamma_c, gamma_f): the N are the sums of absolute terms of sigma'."""
    x = [dec(v) for v in (e11c, e22c, e12f, e11f, e22f, e12c, Pc, Pf, mc, mf, hkc, hkf, s11, s22, s12)]
    e11c, e22c, e12f, e11f, e22f, e12c, Pc, Pf, mc, mf, hkc, hkf, s11, s22, s12 = x
    em2 = dec(k["em2"]) if em2 is None else em2
    one_m = (1 - em2) if hk1 is None else 2 * hk1          # zeta - eta = zeta (1 - e^-2)
    if hkc_scale is not None:
        hkc = hkc * hkc_scale
    Dm, am, ap = dec(k["Dmin"]), dec(k["amin"]), dec(k["amax"])
    dc, df = e11c + e22c, e11f + e22f
    sc = ((e11c - e22c) ** 2 + 4 * e12c ** 2).sqrt()
    sf = ((e11f - e22f) ** 2 + 4 * e12f ** 2).sqrt()
    Dc = max((dc ** 2 + sc ** 2 * em2).sqrt(), Dm)
    Df = max((df ** 2 + sf ** 2 * em2).sqrt(), Dm)
    zc, zf = Pc / (2 * Dc), Pf / (2 * Df)
    Pr = Pc * Dc / (Dc + Dm) if k["pressure_kind"] == 0 else Pc
    etac, etaf = zc * em2, zf * em2
    A, B = zc * one_m * (e11c + e22c), Pr / 2
    T11, T22, T12 = 2 * etac * e11c, 2 * etac * e22c, 2 * etaf * e12f
    s11n, s22n, s12n = T11 + (A - B), T22 + (A - B), T12

    def gamma(z, hk, m):
        # zeta c_alpha dt / m / Az, NaN (0 / 0) -> alpha+^2, then clamp(sqrt(.), alpha-, alpha+): m = 0 gives NaN or +inf, both alpha+
        if m == 0:
            return ap
        return min(max((z * 2 * hk / m).sqrt(), am), ap)
    gc, gf = gamma(zc, hkc, mc), gamma(zf, hkf, mf)
    o11 = s11 + ((s11n - s11) / gc if mc > 0 else 0)
    o22 = s22 + ((s22n - s22) / gc if mc > 0 else 0)
    o12 = s12 + ((s12n - s12) / gf if mf > 0 else 0)
    return (o11, o22, o12, gc, abs(T11) + abs(A) + abs(B), abs(T22) + abs(A) + abs(B), abs(T12), gc, gf)


def stress_bound(sig_old, N, gamma):
    """K_SIGMA u (|sigma| + (N + |sigma|) / gamma) without the K (Decimal)."""
    s = abs(dec(sig_old))
    return DU * (s + (N + s) / gamma)


def ext_stress_cell(kind, tau, rhoCd, we, webar, w, wbar):
    """(ex, im) of one external stress: sea_ice_external_stress.jl:8-27 (numbers / arrays), :176-202 (SemiImplicitStress)."""
    if kind != 3:
        return dec(tau), D(0)
    du, dv = dec(we) - dec(w), dec(webar) - dec(wbar)
    im = dec(rhoCd) * (du * du + dv * dv).sqrt()
    return im * dec(we), im


ZERO, ACTIVE, MARGINAL = 0, 1, 2


def vel_cell(k, w, wn, mi, ai, abar, div, cor, ext, imt, exb, imb, peripheral, wf=None, dt=None):
    """One velocity point of the reference: the tendency (momentum_tendencies_kernel_functions.jl:11-74, `cor` the Coriolis term as it is
    ADDED to G: -x_f_cross_U / -y_f_cross_U), the numerical forcing (evp:391-401), the semi-implicit update and the active / marginal /
    zero selection (split_explicit_momentum_equations.jl:197-264).  wf: the free-drift velocity (None: free drift `nothing`, zero).
    dt: a Decimal replacing k["dt"] (the tests' perturbed evaluation).
    Returns (result, decision, N / |D|): decision ZERO / ACTIVE / MARGINAL; N / |D| the sum of the absolute terms of the numerator of
    (abar w + dt G) / (abar + dt tau_i) over its denominator (None where mi <= 0)."""
    w, wn, mi, ai, abar, div, cor, ext, imt, exb, imb = [dec(v) for v in (w, wn, mi, ai, abar, div, cor, ext, imt, exb, imb)]
    dt = dec(k["dt"]) if dt is None else dt
    dtau = dt / abar
    cond = None
    if mi > 0:
        t_top, t_bot, t_div, t_f = ext / mi * ai, exb / mi * ai, div / mi, (wn - w) / dtau / abar
        G = cor - t_top + t_bot + t_div + t_f
        tau_i = (imb - imt) / mi * ai
        N = abs(abar * w) + dt * (abs(cor) + abs(t_bot - t_top) + abs(t_div) + abs(t_f))
        cond = N / abs(abar + dt * tau_i)
    else:
        G, tau_i = D(0), D(0)
    wD = (w + dtau * G) / (1 + dtau * tau_i)
    active = (mi >= dec(k["min_mass"])) and (ai >= dec(k["min_conc"]))
    marginal = (mi > dec(EPS64)) and (ai > dec(EPS64))
    if active:
        res, what = wD, ACTIVE
    elif marginal:
        res, what = (D(0) if wf is None else dec(wf)), MARGINAL
    else:
        res, what = D(0), ZERO
    if peripheral:
        res = D(0)
    return res, what, cond


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (floats / Decimals / Decimals); a zero bound demands an exact match (ratio inf otherwise).
    Returns (ratio, index)."""
    worst, at = 0.0, -1
    with hp():
        for i, (g, r, b) in enumerate(zip(got, ref, bound)):
            g = float(g)
            if not np.isfinite(g):
                return float("inf"), i
            e = abs(D(g) - r)
            q = float(e / b) if b != 0 else (0.0 if e == 0 else float("inf"))
            if q > worst:
                worst, at = q, i
    return worst, at
