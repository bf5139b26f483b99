"""Test-side NumPy / Python restatement of the momentum balance terms, the interface stresses and their power (include/csi.h,
"momentum balance terms, interface stresses and their power").  TEST INFRASTRUCTURE ONLY.

Built on tests/momentum_ref.py's Ref (imported, not edited): its predicates, stress divergence, immersed flux term, external stresses,
Coriolis parameter and interpolated mass are the ones the tendency restatement adds up; here the pieces are kept, point by point in the
DOCUMENTED order of operations (plain Python floats: IEEE double, no contraction).  The state is an oracle.Problem's arrays: whatever
their halos hold is what is read, so a GPU test copies the model's parents in.  The sums go through the record tree of
tests/diagnostics_ref.py.  Nothing here is taken from the library.
"""
import math

import numpy as np

import diagnostics_ref as dref
import oracle as O
from momentum_ref import Ref

TERMS = ("coriolis", "top", "bottom", "internal", "forcing")
FIELDS = tuple(f"{t}_{c}" for t in TERMS for c in ("x", "y"))
GROUPS = {"external": ("top", "bottom"), "body": ("coriolis", "forcing"), "internal": ("internal",)}


def same_bits(a, b):
    """Arrays equal bit for bit (-0.0 != +0.0), NaN equal to NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


class TermsRef:
    """rheology: "evp" (the stored sigma11, sigma22, sigma12 of the problem), "viscous" (nu * delta u) or None (free-drift dynamics: the
    internal term is +0.0).  rho: the density the interpolated mass is formed with (None: the problem's)."""

    def __init__(self, p, rheology="evp", nu=1000.0, rho=None):
        self.r = Ref(p, nu=nu, viscous=(rheology != "evp"))
        self.p, self.s, self.rheology = p, p.s, rheology
        self.rho = p.s.rho_ice if rho is None else float(rho)
        self.exu = 1 if p.s.topo_x in (O.BOUNDED, O.LEFT_CONNECTED) else 0          # the last face of a high wall
        self.eyv = 1 if p.s.topo_y in (O.BOUNDED, O.LEFT_CONNECTED) else 0

    # ---- x_momentum_stress / y_momentum_stress, sea_ice_external_stress.jl:33-37, 162-174 -------------------------------------------
    def total_tau(self, st, comp, u, v, i, j):
        r = self.r
        if st.kind == O.STRESS_SEMI_IMPLICIT:
            du = r._ext(st, comp, i, j) - r.at(u if comp == "u" else v, i, j)
            return st.rho_e * st.Cd * r._drag_norm(st, comp, u, v, i, j) * du
        return r.explicit_tau(st, comp, u, v, i, j)

    def mass_conc(self, comp, i, j):
        r = self.r
        h, a = self.p.f["h"], self.p.f["aice"]
        (i0, j0) = (i - 1, j) if comp == "u" else (i, j - 1)
        mi = (r.at(h, i0, j0) * self.rho * r.at(a, i0, j0) + r.at(h, i, j) * self.rho * r.at(a, i, j)) / 2
        ai = (r.at(a, i0, j0) + r.at(a, i, j)) / 2
        return mi, ai

    # ---- the pieces of the tendency at one point -------------------------------------------------------------------------------------
    def pieces(self, comp, i, j):
        """What u_velocity_tendency / v_velocity_tendency add up, before any scaling: x_f_cross_U, tau_top, tau_bottom (TOTAL stresses),
        div, imm, the user forcing, m_i, a_i and whether the node is peripheral."""
        r, s = self.r, self.s
        u, v = self.p.f["u"], self.p.f["v"]
        mi, ai = self.mass_conc(comp, i, j)
        if comp == "u":
            cross = -r.fcor("u", i, j) * r._avg4([r.at(v, *q) for q in r._pts("u", i, j)]) if s.has_coriolis else None
            div, imm = (r.div1(u, v, i, j), r.immersed1(i, j)) if self.rheology else (None, None)
            user = r.at(r._arr(s.forcing_u, "u"), i, j) if s.has_forcing else None
        else:
            cross = r.fcor("v", i, j) * r._avg4([r.at(u, *q) for q in r._pts("v", i, j)]) if s.has_coriolis else None
            div, imm = (r.div2(u, v, i, j), r.immersed2(i, j)) if self.rheology else (None, None)
            user = r.at(r._arr(s.forcing_v, "v"), i, j) if s.has_forcing else None
        return dict(cross=cross, ttop=self.total_tau(s.top, comp, u, v, i, j), tbot=self.total_tau(s.bottom, comp, u, v, i, j),
                    div=div, imm=imm, user=user, mi=mi, ai=ai, peripheral=r.peripheral(comp, i, j))

    def point(self, comp, i, j, raw=False):
        """The five slot values at the u / v point (i, j), in the order of TERMS."""
        q = self.pieces(comp, i, j)
        if q["mi"] <= 0 or q["peripheral"]:
            return (0.0,) * 5
        mi, ai = q["mi"], q["ai"]
        return (0.0 if q["cross"] is None else mi * (-q["cross"]),
                q["ttop"] if raw else -(ai * q["ttop"]),
                q["tbot"] if raw else ai * q["tbot"],
                0.0 if q["div"] is None else q["div"] + q["imm"],
                0.0 if q["user"] is None else mi * q["user"])

    # ---- fields over the slots' own interiors ---------------------------------------------------------------------------------------------
    def fields(self, raw=False, extent=True):
        """name -> array over the slot's interior: (Ny, Nx + exu) for _x, (Ny + eyv, Nx) for _y (extent = False: (Ny, Nx) for both)."""
        s = self.s
        nxu, nyv = s.Nx + (self.exu if extent else 0), s.Ny + (self.eyv if extent else 0)
        out = {f"{t}_x": np.zeros((s.Ny, nxu)) for t in TERMS}
        out.update({f"{t}_y": np.zeros((nyv, s.Nx)) for t in TERMS})
        with np.errstate(all="ignore"):
            for j in range(1, s.Ny + 1):
                for i in range(1, nxu + 1):
                    for t, val in zip(TERMS, self.point("u", i, j, raw)):
                        out[f"{t}_x"][j - 1, i - 1] = val
            for j in range(1, nyv + 1):
                for i in range(1, s.Nx + 1):
                    for t, val in zip(TERMS, self.point("v", i, j, raw)):
                        out[f"{t}_y"][j - 1, i - 1] = val
        return out

    # ---- power: one summand per cell and term, (u * F_x) * Az^fc + (v * F_y) * Az^cf ------------------------------------------------
    def power_terms(self, fields=None):
        r, s = self.r, self.s
        f = fields or self.fields(extent=False)
        u, v = self.p.f["u"], self.p.f["v"]
        out = {t: np.zeros((s.Ny, s.Nx)) for t in TERMS}
        with np.errstate(all="ignore"):
            for j in range(1, s.Ny + 1):
                for i in range(1, s.Nx + 1):
                    uu, vv = r.at(u, i, j), r.at(v, i, j)
                    azfc, azcf = r.m("az", (O.FACE, O.CENTER), i, j), r.m("az", (O.CENTER, O.FACE), i, j)
                    for t in TERMS:
                        out[t][j - 1, i - 1] = (uu * float(f[f"{t}_x"][j - 1, i - 1])) * azfc + (vv * float(f[f"{t}_y"][j - 1, i - 1])) * azcf
        return out

    def budget(self, fields=None):
        """term -> the sum in the documented order (tests/diagnostics_ref.py ordered_sum)."""
        return {t: dref.ordered_sum(x) for t, x in self.power_terms(fields).items()}


def reassembled(q, total=True, coef=(0.0, 0.0), own=0.0, extra_forcing=0.0):
    """The reference's sum (-cor - ttop / m_i * a_i + tbot / m_i * a_i + div / m_i + imm / m_i + forcing) from the pieces of a point.
    total: the pieces hold TOTAL stresses; the explicit part is total + coef * u, coef = (top, bottom) implicit coefficients."""
    mi, ai = q["mi"], q["ai"]
    ttop, tbot = q["ttop"], q["tbot"]
    if total:
        ttop, tbot = ttop + coef[0] * own, tbot + coef[1] * own
    cor = 0.0 if q["cross"] is None else q["cross"]
    forcing = (0.0 if q["user"] is None else q["user"]) + extra_forcing
    return (-cor - ttop / mi * ai + tbot / mi * ai + q["div"] / mi + q["imm"] / mi + forcing)
