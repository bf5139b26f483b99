"""Test-side NumPy / Python restatement of ViscousRheology and the ExplicitSolver (TEST INFRASTRUCTURE ONLY).

Restates, point by point in the reference's operation order (plain Python floats: IEEE double, no contraction), what the STRICT
kernels of csrc/momentum_viscous.hip and csrc/momentum_explicit.hip compute:

  ViscousRheology stresses           Rheologies/viscous_rheology.jl:15-22 (nu a Number: nu * delta u)
  conditional fluxes on masks        Rheologies/ice_stress_divergence.jl:21-24 (predicates restated from oracle/csi_oracle.c)
  stress divergence                  :36-51;  immersed flux term :65-123
  velocity tendencies                SeaIceDynamics/momentum_tendencies_kernel_functions.jl:11-74
  viscous sub-step / sub-cycle       SeaIceDynamics/split_explicit_momentum_equations.jl:103-264 with Rheologies.jl:42-55
  explicit tendency and step         SeaIceDynamics/explicit_momentum_equations.jl:6-113

It works on an oracle.Problem (oracle/oracle.py): the problem's arrays hold the state, its metrics, stresses, Coriolis parameter,
forcing, mask and boundary conditions describe the model, and its C routines provide what this file does not restate: the local
halo fills of u and v (ora_fill_halo_u / _v, the library's store images) and the free-drift velocities (ora_free_drift_u / _v).

Within a component the viscous sub-step is Jacobi: every point reads the OLD values of its own component (the library's
deliberate departure from the reference's in-place kernel, whose result depends on scheduling; include/csi.h); between the
components it is Gauss-Seidel in the parity order of split_explicit_momentum_equations.jl:178.
Arrays are (nj, ni), element (i, j) (1-based) at a[j + Hy - 1, i + Hx - 1], as in oracle_np.py.

The number type is a parameter.  Ref(p, ..., num=float) is the restatement above.  Ref(p, ..., num=fast_math_ref.CTX) evaluates the
same expressions, in the same order, in that `decimal` context (80 digits, one rounding per operation, the square root of the drag
norm included): every input is the same double, converted exactly, so the result is the truth that STRICT and FAST both approximate.
What a step stores goes into the problem's double arrays rounded once (the next launch reads doubles); the unrounded values of the
last tendency / component step are kept in `self.q` ("u", "v", "Gu", "Gv": object arrays over the interior).  The exact path has no
free drift: that value comes from the C oracle, in double.
"""
import contextlib
import ctypes as C
import decimal
import math

import numpy as np

import oracle as O

EPS64 = 2.220446049250313e-16
CC, FC, CF, FF = (O.CENTER, O.CENTER), (O.FACE, O.CENTER), (O.CENTER, O.FACE), (O.FACE, O.FACE)


def rel_error(Q, exact, ctx):
    """max|Q - exact| / max|exact| over the interior: Q an array of doubles, exact the object array of Decimals of Ref.q (evaluated in
    `ctx`, the differences formed there before anything is rounded to double).  A non-finite Q gives inf."""
    Q = np.asarray(Q, dtype=np.float64)
    assert Q.shape == exact.shape
    if not np.all(np.isfinite(Q)):
        return math.inf
    with decimal.localcontext(ctx):
        worst = max(abs(decimal.Decimal(float(a)) - b) for a, b in zip(Q.ravel(), exact.ravel()))
        scale = max(abs(b) for b in exact.ravel())
        return float(worst / scale)


class Ref:
    def __init__(self, p, nu=1000.0, viscous=True, num=float):
        self.p, self.s, self.viscous = p, p.s, viscous
        s = p.s
        if num is float:
            self.N, self.sqrt, self.nan, self.ctx = float, math.sqrt, math.nan, contextlib.nullcontext
            self.szero = lambda x: math.copysign(0.0, x)
        else:                                             # a decimal.Context: a double converts exactly, whatever the precision
            assert isinstance(num, decimal.Context) and not s.free_drift_kind, "the exact path has no free drift"
            self.N, self.sqrt, self.nan = (lambda x: decimal.Decimal(float(x))), (lambda x: x.sqrt()), decimal.Decimal("NaN")
            self.ctx = lambda: decimal.localcontext(num)
            self.szero = lambda x: decimal.Decimal(0).copy_sign(x)
        self.zero = self.N(0.0)
        self.nu = self.N(nu)
        self.Nx, self.Ny, self.Hx, self.Hy = s.Nx, s.Ny, s.Hx, s.Hy
        # metrics at every location over the parent index range (Ny + 2Hy + 1) x (Nx + 2Hx + 1), from the oracle's own operators
        ni, nj = s.Nx + 2 * s.Hx + 1, s.Ny + 2 * s.Hy + 1
        self.met = {}
        for w, fn in (("dx", p.L.ora_dx), ("dy", p.L.ora_dy), ("az", p.L.ora_az)):
            for loc in (CC, FC, CF, FF):
                self.met[w, loc] = [[self.N(fn(p.ptr, loc[0], loc[1], i - s.Hx + 1, j - s.Hy + 1)) for i in range(ni)] for j in range(nj)]
        self.mask = p._mask if s.has_mask else None
        self.Gu = np.zeros_like(p.f["u"])
        self.Gv = np.zeros_like(p.f["v"])
        self.q = {k: np.full((s.Ny, s.Nx), self.zero, dtype=object) for k in ("u", "v", "Gu", "Gv")}

    # ---- access ----------------------------------------------------------------------------------------------------------------
    def at(self, a, i, j):
        return self.N(a[j + self.Hy - 1, i + self.Hx - 1])

    def m(self, w, loc, i, j):
        return self.met[w, loc][j + self.Hy - 1][i + self.Hx - 1]

    def _arr(self, fld, like):
        return np.ctypeslib.as_array(fld.p, shape=(self.p.f[like].shape[0], fld.ld))

    # ---- predicates (csi_oracle.c inactive_cell / immersed_peripheral_*) -----------------------------------------------------------
    def under(self, i, j):
        s = self.s
        wl = lambda t: t in (O.BOUNDED, O.RIGHT_CONNECTED, O.RIGHT_FOLDED)
        wh = lambda t: t in (O.BOUNDED, O.LEFT_CONNECTED)
        return ((wl(s.topo_x) and i < 1) or (wh(s.topo_x) and i > s.Nx) or (wl(s.topo_y) and j < 1) or (wh(s.topo_y) and j > s.Ny))

    def inactive(self, i, j):
        if self.under(i, j):
            return True
        if self.mask is not None:
            if i < 1 - self.Hx or i > self.Nx + self.Hx or j < 1 - self.Hy or j > self.Ny + self.Hy:
                return True
            return not self.mask[j + self.Hy - 1, i + self.Hx - 1]
        return False

    def ipcc(self, i, j):
        return self.mask is not None and self.inactive(i, j) and not self.under(i, j)

    def ipff(self, i, j):
        if self.mask is None:
            return False
        cells = ((i, j), (i - 1, j), (i, j - 1), (i - 1, j - 1))
        return any(self.inactive(*c) for c in cells) and not any(self.under(*c) for c in cells)

    # ---- stresses (viscous_rheology.jl / stored sigma) behind conditional_flux_ccc / _ffc ----------------------------------------
    def ux(self, u, i, j):
        val = self.nu * (self.at(u, i + 1, j) - self.at(u, i, j)) if self.viscous else self.at(self.p.f["s11"], i, j)
        return self.zero if self.ipcc(i, j) else val

    def vy(self, v, i, j):
        val = self.nu * (self.at(v, i, j + 1) - self.at(v, i, j)) if self.viscous else self.at(self.p.f["s22"], i, j)
        return self.zero if self.ipcc(i, j) else val

    def uy(self, u, i, j):
        val = self.nu * (self.at(u, i, j) - self.at(u, i, j - 1)) if self.viscous else self.at(self.p.f["s12"], i, j)
        return self.zero if self.ipff(i, j) else val

    def vx(self, v, i, j):
        val = self.nu * (self.at(v, i, j) - self.at(v, i - 1, j)) if self.viscous else self.at(self.p.f["s12"], i, j)
        return self.zero if self.ipff(i, j) else val

    # ---- divergence, ice_stress_divergence.jl:36-51 ------------------------------------------------------------------------------
    def div1(self, u, v, i, j):
        sD = lambda ii: self.ux(u, ii, j) + self.vy(v, ii, j)
        sT = lambda ii: self.ux(u, ii, j) - self.vy(v, ii, j)
        dyfc = self.m("dy", FC, i, j)
        d = dyfc * (sD(i) - sD(i - 1)) / 2
        dyc, dycm = self.m("dy", CC, i, j), self.m("dy", CC, i - 1, j)
        T = ((dyc * dyc) * sT(i) - (dycm * dycm) * sT(i - 1)) / dyfc / 2
        dxfn, dxf = self.m("dx", FF, i, j + 1), self.m("dx", FF, i, j)
        S = ((dxfn * dxfn) * self.uy(u, i, j + 1) - (dxf * dxf) * self.uy(u, i, j)) / self.m("dx", FC, i, j)
        return (d + T + S) / self.m("az", FC, i, j)

    def div2(self, u, v, i, j):
        sD = lambda jj: self.ux(u, i, jj) + self.vy(v, i, jj)
        sT = lambda jj: self.ux(u, i, jj) - self.vy(v, i, jj)
        dxcf = self.m("dx", CF, i, j)
        d = dxcf * (sD(j) - sD(j - 1)) / 2
        dxc, dxcm = self.m("dx", CC, i, j), self.m("dx", CC, i, j - 1)
        T = -((dxc * dxc) * sT(j) - (dxcm * dxcm) * sT(j - 1)) / dxcf / 2
        dyfn, dyf = self.m("dy", FF, i + 1, j), self.m("dy", FF, i, j)
        S = ((dyfn * dyfn) * self.vx(v, i + 1, j) - (dyf * dyf) * self.vx(v, i, j)) / self.m("dy", CF, i, j)
        return (d + T + S) / self.m("az", CF, i, j)

    def immersed1(self, i, j):
        if self.mask is None:
            return self.zero
        b = [self.N(x) for x in self.s.ibc_u]
        qW = (-b[0] if self.ipcc(i - 1, j) else self.zero) * self.m("dy", CC, i - 1, j)
        qE = (b[1] if self.ipcc(i, j) else self.zero) * self.m("dy", CC, i, j)
        qS = (-b[2] if self.ipff(i, j) else self.zero) * self.m("dx", FF, i, j)
        qN = (b[3] if self.ipff(i, j + 1) else self.zero) * self.m("dx", FF, i, j + 1)
        return (qE - qW + qN - qS) / self.m("az", FC, i, j)

    def immersed2(self, i, j):
        if self.mask is None:
            return self.zero
        b = [self.N(x) for x in self.s.ibc_v]
        qW = (-b[0] if self.ipff(i, j) else self.zero) * self.m("dy", FF, i, j)
        qE = (b[1] if self.ipff(i + 1, j) else self.zero) * self.m("dy", FF, i + 1, j)
        qS = (-b[2] if self.ipcc(i, j - 1) else self.zero) * self.m("dx", CC, i, j - 1)
        qN = (b[3] if self.ipcc(i, j) else self.zero) * self.m("dx", CC, i, j)
        return (qE - qW + qN - qS) / self.m("az", CF, i, j)

    # ---- external stresses, sea_ice_external_stress.jl:8-27,176-202 ---------------------------------------------------------------
    def _ext(self, st, comp, i, j):
        kind, val = (st.ue_kind, st.ue) if comp == "u" else (st.ve_kind, st.ve)
        if kind == O.VEL_FIELD:
            return self.at(self._arr(st.fu if comp == "u" else st.fv, comp), i, j)
        return self.N(val) if kind == O.VEL_CONST else self.zero

    @staticmethod
    def _avg4(x):
        return ((x[0] + x[1]) / 2 + (x[2] + x[3]) / 2) / 2

    def _pts(self, comp, i, j):
        # the four points of the cross average at a u point (v points) / a v point (u points)
        return ((i - 1, j), (i, j), (i - 1, j + 1), (i, j + 1)) if comp == "u" else ((i, j - 1), (i + 1, j - 1), (i, j), (i + 1, j))

    def _drag_norm(self, st, comp, u, v, i, j):
        own, other, oc = (u, v, "v") if comp == "u" else (v, u, "u")
        d1 = self._ext(st, comp, i, j) - self.at(own, i, j)
        pts = self._pts(comp, i, j)
        d2 = self._avg4([self._ext(st, oc, *q) for q in pts]) - self._avg4([self.at(other, *q) for q in pts])
        return self.sqrt(d1 * d1 + d2 * d2)

    def explicit_tau(self, st, comp, u, v, i, j):
        if st.kind == O.STRESS_CONST:
            return self.N(st.tau_u if comp == "u" else st.tau_v)
        if st.kind == O.STRESS_FIELD:
            return self.at(self._arr(st.fu if comp == "u" else st.fv, comp), i, j)
        if st.kind == O.STRESS_SEMI_IMPLICIT:
            return self.N(st.rho_e) * self.N(st.Cd) * self._drag_norm(st, comp, u, v, i, j) * self._ext(st, comp, i, j)
        return self.zero

    def implicit_tau(self, st, comp, u, v, i, j):
        return self.N(st.rho_e) * self.N(st.Cd) * self._drag_norm(st, comp, u, v, i, j) if st.kind == O.STRESS_SEMI_IMPLICIT else self.zero

    def fcor(self, comp, i, j):
        s = self.s
        pts = s.fu_points if comp == "u" else s.fv_points
        if pts:
            return self.N(pts[(i + s.Hx - 1) + (j + s.Hy - 1) * s.f_points_ld])
        rows = s.fu_rows if comp == "u" else s.fv_rows
        return self.N(rows[j + s.Hy - 1] if rows else s.f_coriolis)

    # ---- interpolated mass / concentration ---------------------------------------------------------------------------------------
    def mass_conc(self, comp, i, j):
        h, a, rho = self.p.f["h"], self.p.f["aice"], self.N(self.s.rho_ice)
        (i0, j0) = (i - 1, j) if comp == "u" else (i, j - 1)
        mi = (self.at(h, i0, j0) * rho * self.at(a, i0, j0) + self.at(h, i, j) * rho * self.at(a, i, j)) / 2
        ai = (self.at(a, i0, j0) + self.at(a, i, j)) / 2
        return mi, ai

    # ---- velocity tendencies, momentum_tendencies_kernel_functions.jl:11-74 -------------------------------------------------------
    def tendency(self, comp, u, v, i, j, dt_forcing):
        s, f = self.s, self.p.f
        mi, ai = self.mass_conc(comp, i, j)
        if comp == "u":
            cor = -self.fcor("u", i, j) * self._avg4([self.at(v, *q) for q in self._pts("u", i, j)]) if s.has_coriolis else self.zero
            div, imm = self.div1(u, v, i, j), self.immersed1(i, j)
            user = self.at(self._arr(s.forcing_u, "u"), i, j) if s.has_forcing else self.zero
            own, n, al_pts = u, f["un"], ((i - 1, j), (i, j))
        else:
            cor = self.fcor("v", i, j) * self._avg4([self.at(u, *q) for q in self._pts("v", i, j)]) if s.has_coriolis else self.zero
            div, imm = self.div2(u, v, i, j), self.immersed2(i, j)
            user = self.at(self._arr(s.forcing_v, "v"), i, j) if s.has_forcing else self.zero
            own, n, al_pts = v, f["vn"], ((i, j - 1), (i, j))
        forcing = user                                    # Rheologies.jl:52-53
        if not self.viscous:                              # elasto_visco_plastic_rheology.jl:391-401
            abar = (self.at(f["alpha"], *al_pts[0]) + self.at(f["alpha"], *al_pts[1])) / 2
            forcing = user + (self.at(n, i, j) - self.at(own, i, j)) / self.N(dt_forcing) / abar
        G = (-cor
             - self.explicit_tau(s.top, comp, u, v, i, j) / mi * ai
             + self.explicit_tau(s.bottom, comp, u, v, i, j) / mi * ai
             + div / mi
             + imm / mi
             + forcing) if mi != 0 else self.nan
        return (self.zero if mi <= 0 else G), mi, ai

    def free_drift(self, comp, i, j):
        if not self.s.free_drift_kind:
            return self.zero
        return self.N((self.p.L.ora_free_drift_u if comp == "u" else self.p.L.ora_free_drift_v)(self.p.ptr, i, j))

    def fill(self, comp):
        (self.p.L.ora_fill_halo_u if comp == "u" else self.p.L.ora_fill_halo_v)(self.p.ptr)

    def peripheral(self, comp, i, j):
        return self.inactive(i, j) or self.inactive(*((i - 1, j) if comp == "u" else (i, j - 1)))

    def points(self, order=None):
        pts = [(i, j) for j in range(1, self.Ny + 1) for i in range(1, self.Nx + 1)]
        return pts if order is None else [pts[k] for k in order]

    # ---- the viscous split-explicit sub-step (split_explicit_momentum_equations.jl:197-264), Jacobi within the component ---------
    def viscous_component_step(self, comp, dtau, order=None):
        f = self.p.f
        old_u, old_v = f["u"].copy(), f["v"].copy()
        new = (old_u if comp == "u" else old_v).copy()
        s = self.s
        with self.ctx():
            dtau = self.N(dtau)
            for (i, j) in self.points(order):
                G, mi, ai = self.tendency(comp, old_u, old_v, i, j, 0.0)
                tau = ((self.implicit_tau(s.bottom, comp, old_u, old_v, i, j) - self.implicit_tau(s.top, comp, old_u, old_v, i, j)) / mi * ai
                       if mi != 0 else self.nan)
                tau = self.zero if mi <= 0 else tau
                c0 = self.at(old_u if comp == "u" else old_v, i, j)
                D = (c0 + dtau * G) / (1 + dtau * tau)
                F = self.free_drift(comp, i, j)
                marginal, active = (mi > EPS64) and (ai > EPS64), (mi >= s.min_mass) and (ai >= s.min_conc)
                sel = D if active else (F if marginal else self.zero)
                sel = self.szero(sel) if self.peripheral(comp, i, j) else sel
                self.q[comp][j - 1, i - 1] = sel
                new[j + self.Hy - 1, i + self.Hx - 1] = float(sel)
        np.copyto(f[comp], new)
        self.fill(comp)

    def viscous_subcycle(self, dt, substeps):
        self.fill("u")
        self.fill("v")
        dtau = dt / substeps                                                            # Rheologies.jl:48-49
        for sub in range(1, substeps + 1):
            for comp in (("u", "v") if sub % 2 == 0 else ("v", "u")):                  # :178-187
                self.viscous_component_step(comp, dtau)

    def time_step_momentum(self, dt, substeps, rk_reset=False, explicit=False):
        f = self.p.f
        if explicit:
            return self.explicit_step(dt, rk_reset)
        if rk_reset:                                                                    # reset_velocities!, :89-93
            np.copyto(f["u"], f["um"])
            np.copyto(f["v"], f["vm"])
        self.viscous_subcycle(dt, substeps)

    # ---- ExplicitSolver ----------------------------------------------------------------------------------------------------------
    def compute_tendencies(self, dt):
        u, v = self.p.f["u"], self.p.f["v"]
        with self.ctx():
            for (i, j) in self.points():
                for comp, G in (("u", self.Gu), ("v", self.Gv)):
                    g = self.tendency(comp, u, v, i, j, dt)[0]
                    self.q["G" + comp][j - 1, i - 1] = g
                    G[j + self.Hy - 1, i + self.Hx - 1] = float(g)

    def explicit_step(self, dt, rk_reset=False):
        f, s = self.p.f, self.s
        for comp, G in (("u", self.Gu), ("v", self.Gv)):
            prev = (f["um"] if comp == "u" else f["vm"]) if rk_reset else f[comp]
            u, v = f["u"].copy(), f["v"].copy()
            new = f[comp].copy()
            with self.ctx():
                dtn = self.N(dt)
                for (i, j) in self.points():
                    mi, ai = self.mass_conc(comp, i, j)
                    tau = ((self.implicit_tau(s.bottom, comp, u, v, i, j) - self.implicit_tau(s.top, comp, u, v, i, j)) / mi * ai
                           if mi != 0 else self.nan)
                    D = (self.at(prev, i, j) + dtn * self.at(G, i, j)) / (1 + dtn * tau)
                    F = self.free_drift(comp, i, j)
                    marginal, active = (mi > EPS64) and (ai > EPS64), (mi >= s.min_mass) and (ai >= s.min_conc)
                    sel = D if active else (F if marginal else self.zero)
                    self.q[comp][j - 1, i - 1] = sel
                    new[j + self.Hy - 1, i + self.Hx - 1] = float(sel)
            np.copyto(f[comp], new)
            self.fill(comp)                                                             # fill_halo_regions!, :33, :36

    # ---- whole steps composed with the oracle's tracer pieces (sea_ice_fe_step.jl:13-34, sea_ice_rk_substep.jl:81-94) ------------
    def _thermo(self, slab, dt):
        if slab is None:
            return
        h, a = self.p.interior("h"), self.p.interior("aice")
        hc, ac = np.ascontiguousarray(h), np.ascontiguousarray(a)
        dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
        self.p.L.ora_slab_thermo_step(C.byref(slab), hc.size, dp(hc), dp(ac), None, dt)
        h[...] = hc
        a[...] = ac

    def time_step_fe(self, dt, substeps, scheme, explicit, first_iteration=False, slab=None):
        p = self.p
        if first_iteration:
            p.update_state()
        p.compute_tracer_tendencies(scheme)
        if explicit:
            self.compute_tendencies(dt)
        self.time_step_momentum(dt, substeps, False, explicit)
        p.dynamic_step_tracers(dt, False)
        self._thermo(slab, dt)
        p.update_state()

    def time_step_rk3(self, dt, substeps, scheme, explicit, slab=None):
        p, f = self.p, self.p.f
        for dst, src in (("hm", "h"), ("am", "aice"), ("um", "u"), ("vm", "v")):       # cache_current_fields!
            np.copyto(f[dst], f[src])
        for beta in (3, 2, 1):
            dtau = dt / beta
            p.compute_tracer_tendencies(scheme)
            if explicit:
                self.compute_tendencies(dtau)
            self.time_step_momentum(dtau, substeps, True, explicit)
            p.dynamic_step_tracers(dtau, True)
            self._thermo(slab, dtau)
            p.update_state()
