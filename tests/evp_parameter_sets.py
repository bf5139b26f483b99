"""Non-default EVP / dynamics parameter sets and rectangular cells, shared by tests/test_evp_parameters.py (the conditions the sets must
meet, on the CPU oracle alone) and tests/test_gpu_evp_parameters.py (the kernels against the oracle on them).

Every other test takes the defaults of tests/cases.py: square cells and P* 27500, C 20, e 2, Delta_min 2e-9, alpha- 50, alpha+ 300,
c_alpha pi^2, minimum_mass 1, minimum_concentration 1e-3, rho 900.  With e = 2 the constants FAST mode folds on the host (e^-2 = 1/4,
e^-2 / 8 = 1/32, (1 - e^-2) / 2 = 3/8) are exact, and with alpha- = 50 about 97 % of the icy cells sit on the lower clamp.

  set A  e = 1.7 (< 2), clamp bounds 6 / 11 so that all three regimes of alpha are populated, Delta_min 8e-6 so that both sides of the
         floor are, thresholds ABOVE the defaults, dx > dy
  set B  e = 2.7 (> 2, no power of two), IceStrength pressure, thresholds BELOW the defaults, dx < dy

`marginal` is the (aice, h) of make_case's two-row thin-ice patch, chosen per set so that the patch changes branch between the set's
thresholds and the default ones (rho h aice and aice lie between the two minimum_mass / minimum_concentration values).  Set B's
thresholds lie below the defaults, so its second row is active under B and marginal under the defaults; its first row (next to the open water) stays marginal
under both, or B would have no marginal u points at all.
"""
import numpy as np

DEFAULTS = dict(P_star=27500.0, C_star=20.0, ecc=2.0, delta_min=2e-9, alpha_min=50.0, alpha_max=300.0, c_alpha=float(np.pi) ** 2,
                min_mass=1.0, min_conc=1e-3, rho_ice=900.0)

SET_A = dict(P_star=15000.0, C_star=12.5, ecc=1.7, delta_min=8e-6, alpha_min=6.0, alpha_max=11.0, c_alpha=7.3,
             min_mass=2.5, min_conc=3e-3, rho_ice=917.0)
SET_B = dict(P_star=32000.0, C_star=17.0, ecc=2.7, delta_min=1.3e-5, alpha_min=4.0, alpha_max=9.0, c_alpha=5.9,
             min_mass=0.4, min_conc=4e-4, rho_ice=880.0)

RECT_A, RECT_B = (3000.0, 1250.0), (1100.0, 2600.0)

# name -> make_case keywords.  default/rectangular, A/square, A/rectangular, B/rectangular: a failure names the axis that caused it
CELLS = {
    "default_rect": dict(cell=RECT_A),
    "A_square": dict(evp=SET_A, marginal=(2e-3, 1.0)),
    "A_rect": dict(evp=SET_A, marginal=(2e-3, 1.0), cell=RECT_A),
    "B_rect": dict(evp=SET_B, marginal=((1e-4, 1e-3), (9e-4, 1.2)), cell=RECT_B, pressure="ice_strength"),
}
PARAMETER_CELLS = ["A_square", "A_rect", "B_rect"]          # the ones with a non-default set


def params_of(case):
    return dict(DEFAULTS, **case.get("evp", {}))


def face_branches(h, a, params, periodic=(True, True)):
    """(active, marginal, zero) masks at the u and at the v points of an (Ny, Nx) state on a periodic grid: the selection of the velocity
    steps (mi >= minimum_mass and ai >= minimum_concentration: the momentum equation; else mi, ai > eps: free drift; else zero)"""
    eps = np.finfo(np.float64).eps
    m = h * params["rho_ice"] * a
    out = {}
    for comp, axis in (("u", 1), ("v", 0)):
        mi, ai = (np.roll(m, 1, axis=axis) + m) / 2, (np.roll(a, 1, axis=axis) + a) / 2
        active = (mi >= params["min_mass"]) & (ai >= params["min_conc"])
        marginal = ~active & (mi > eps) & (ai > eps)
        out[comp] = (active, marginal, ~active & ~marginal)
    return out
