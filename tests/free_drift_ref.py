"""Test-side restatement of the two free-drift shapes this library adds (TEST INFRASTRUCTURE ONLY).

  free_drift = (u = ..., v = ...)          SeaIceDynamics/stress_balance_free_drift.jl:123-125: the velocity of marginal ice read from
                                           two fields -- momentum_ref.Ref's `free_drift` hook, the only place the viscous and
                                           explicit restatements read that velocity, returns the prescribed arrays' values
  dynamics = StressBalanceFreeDrift(...)   :131-151: one pass over i = 1 .. Nx, j = 1 .. Ny that sets u, v to the closed forms
                                           (:61-109, the C oracle's ora_free_drift_u / _v) at every point, then the local halo fills;
                                           FE / RK3 whole steps composed from it the way Ref composes its own

It works on an oracle.Problem like momentum_ref.Ref.  With `dynamics=True` the problem needs p.s.free_drift_kind = 1 (else the
oracle's closed forms return 0); which stress is the semi-implicit one the oracle reads off the stress kinds.
"""
import numpy as np

from momentum_ref import EPS64, Ref


class FreeDriftRef(Ref):
    def __init__(self, p, fields=None, dynamics=False, **kw):
        """fields = (F_u, F_v): prescribed free-drift velocities, arrays shaped like the parents of u and v (only interior points
        are read).  dynamics: time_step_momentum is the free-drift dynamics step."""
        super().__init__(p, **kw)
        self.fields = fields
        self.dynamics = dynamics
        if dynamics:
            assert p.s.free_drift_kind == 1, "the oracle's closed forms need free_drift_kind = 1"

    # ---- free_drift = (u, v) ---------------------------------------------------------------------------------------------------
    def free_drift(self, comp, i, j):
        if self.fields is None:
            return super().free_drift(comp, i, j)
        return self.at(self.fields[0] if comp == "u" else self.fields[1], i, j)

    # ---- dynamics = StressBalanceFreeDrift (:132-151) ----------------------------------------------------------------------------
    def free_drift_dynamics_step(self):
        p, f = self.p, self.p.f
        for (i, j) in self.points():
            f["u"][j + self.Hy - 1, i + self.Hx - 1] = p.L.ora_free_drift_u(p.ptr, i, j)
            f["v"][j + self.Hy - 1, i + self.Hx - 1] = p.L.ora_free_drift_v(p.ptr, i, j)
        self.fill("u")
        self.fill("v")

    def time_step_momentum(self, dt, substeps, rk_reset=False, explicit=False):
        if self.dynamics:                       # no dt, no sub-steps, no reset from Psi^-
            return self.free_drift_dynamics_step()
        return super().time_step_momentum(dt, substeps, rk_reset, explicit)

    # ---- what the tests count --------------------------------------------------------------------------------------------------
    def marginal(self, comp):
        return marginal_points(self.p, comp)

    def peripheral_points(self, comp):
        out = np.zeros((self.Ny, self.Nx), dtype=bool)
        for (i, j) in self.points():
            out[j - 1, i - 1] = self.peripheral(comp, i, j)
        return out

    def explicit_stress_magnitude(self, comp):
        """|tau| of the stress that is NOT the semi-implicit one, as the closed form of component `comp` sees it (own component at
        the point, the other one four-point averaged), at the points i = 1 .. Nx, j = 1 .. Ny."""
        s = self.s
        import oracle as O
        expl = s.top if s.bottom.kind == O.STRESS_SEMI_IMPLICIT else s.bottom
        u, v = self.p.f["u"], self.p.f["v"]
        out = np.zeros((self.Ny, self.Nx))
        other = "v" if comp == "u" else "u"
        for (i, j) in self.points():
            own = self.explicit_tau(expl, comp, u, v, i, j)
            x = self._avg4([self.explicit_tau(expl, other, u, v, *q) for q in self._pts(comp, i, j)])
            out[j - 1, i - 1] = np.sqrt(own * own + x * x)
        return out


def marginal_points(p, comp):
    """Boolean (Ny, Nx) array: the u / v points i = 1 .. Nx, j = 1 .. Ny of problem p that take the marginal branch of the velocity
    select (m > eps, a > eps, and m < minimum_mass or a < minimum_concentration; split_explicit_momentum_equations.jl:219-228), from
    the state as it stands (halos filled: p.update_state())."""
    s, f = p.s, p.f
    h, a = f["h"], f["aice"]
    m = h * s.rho_ice * a
    J, I = slice(s.Hy, s.Hy + s.Ny), slice(s.Hx, s.Hx + s.Nx)
    Jm, Im = slice(s.Hy - 1, s.Hy + s.Ny - 1), slice(s.Hx - 1, s.Hx + s.Nx - 1)
    lo = (J, Im) if comp == "u" else (Jm, I)
    mi = (m[lo] + m[J, I]) / 2
    ai = (a[lo] + a[J, I]) / 2
    return (mi > EPS64) & (ai > EPS64) & ((mi < s.min_mass) | (ai < s.min_conc))


def peripheral_mask(p, comp):
    """Boolean (Ny, Nx) array: the u / v points i = 1 .. Nx, j = 1 .. Ny that are peripheral nodes -- one of their two cells is inactive
    (land, or beyond a wall): momentum_ref.Ref.peripheral, vectorised.  The velocity select gives them a signed zero, not the free
    drift."""
    import oracle as O
    s = p.s
    active = np.ones(p.f["h"].shape, dtype=bool) if not s.has_mask else (np.asarray(p._mask) != 0)
    active = active.copy()
    if s.topo_x in (O.BOUNDED, O.RIGHT_CONNECTED, O.RIGHT_FOLDED):
        active[:, :s.Hx] = False
    if s.topo_x in (O.BOUNDED, O.LEFT_CONNECTED):
        active[:, s.Hx + s.Nx:] = False
    if s.topo_y in (O.BOUNDED, O.RIGHT_CONNECTED, O.RIGHT_FOLDED):
        active[:s.Hy, :] = False
    if s.topo_y in (O.BOUNDED, O.LEFT_CONNECTED):
        active[s.Hy + s.Ny:, :] = False
    J, I = slice(s.Hy, s.Hy + s.Ny), slice(s.Hx, s.Hx + s.Nx)
    Jm, Im = slice(s.Hy - 1, s.Hy + s.Ny - 1), slice(s.Hx - 1, s.Hx + s.Nx - 1)
    lo = (J, Im) if comp == "u" else (Jm, I)
    return ~(active[lo] & active[J, I])


def free_drift_points(p, comp):
    """The points that TAKE the free-drift velocity: marginal and not peripheral (what the tests' 10 % is counted on)."""
    return marginal_points(p, comp) & ~peripheral_mask(p, comp)


def free_drift_arrays(p):
    """(F_u, F_v): the oracle's closed forms at every interior u and v point of problem p (free_drift_kind = 1), interior-shaped."""
    s = p.s
    nyu, nxu = p.interior("u").shape
    nyv, nxv = p.interior("v").shape
    Fu = np.array([[p.L.ora_free_drift_u(p.ptr, i, j) for i in range(1, nxu + 1)] for j in range(1, nyu + 1)])
    Fv = np.array([[p.L.ora_free_drift_v(p.ptr, i, j) for i in range(1, nxv + 1)] for j in range(1, nyv + 1)])
    return Fu, Fv


def parent_like(p, name, interior):
    """An array shaped like the parent of oracle field `name` holding `interior` (halos zero: the restatement reads interior points)."""
    arr = np.zeros_like(p.f[name])
    ny, nx = interior.shape
    arr[p.s.Hy:p.s.Hy + ny, p.s.Hx:p.s.Hx + nx] = interior
    return arr


def marginal_band(case, rows=(0.4, 0.7)):
    """Make the rows [rows[0] Ny, rows[1] Ny) of a cases.make_case state marginal everywhere (h = 1e-3, aice = 5e-4: mass 4.5e-4 kg
    m^-2, below minimum_mass and minimum_concentration), land kept ice-free.  Edits the case in place and returns it."""
    Ny = case["Ny"]
    j0, j1 = int(rows[0] * Ny), int(rows[1] * Ny)
    wet = case["mask"][j0:j1, :] if case.get("mask") is not None else True
    case["h"][j0:j1, :] = np.where(wet, 1e-3, 0.0)
    case["a"][j0:j1, :] = np.where(wet, 5e-4, 0.0)
    return case
