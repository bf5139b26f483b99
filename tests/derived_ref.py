"""NumPy restatement of the derived fields and the energy budget integrals (include/csi.h, "derived fields and energy budget integrals"):
every formula in the DOCUMENTED order of operations, from the fields' PARENT arrays (halos included, as Field.numpy() returns them: shape
(nj, ni), element (i, j) (1-based) at [j + Hy - 1, i + Hx - 1]), the grid's metrics and the mask's parent.  Nothing here is taken from the
library; the three sums go through the record tree of tests/diagnostics_ref.py.

Every method returns (Ny, Nx) arrays over i = 1 .. Nx, j = 1 .. Ny; an operator "at (i + di, j + dj)" is the same array shifted, so the
elements read outside the interior are exactly the ones the stencils name -- what the header lists as HALO ELEMENTS READ."""
import numpy as np

import climaseaice_jl_amd as csi
import diagnostics_ref as dref

NAMES = ("divergence", "shear", "deformation", "speed", "sigma_I", "sigma_II", "stress_power")
SUMS = ("internal_work", "stress_power", "kinetic_energy")
C, F = "c", "f"


def _wall_lo(t):
    return t in (csi.Bounded, csi.RightConnected, csi.RightFolded)


def _wall_hi(t):
    return t in (csi.Bounded, csi.LeftConnected)


class Ref:
    """grid: a grid of the package (metrics(), topology, Nx, Ny, Hx, Hy).  parents: name -> parent array for u, v and whichever of
    s11, s22, s12, P, h, a the quantities asked for need.  mask: the (Ny + 2Hy, Nx + 2Hx) uint8 parent of the activity mask, or None."""

    def __init__(self, grid, parents, mask=None, rho=900.0):
        self.g, self.p, self.mask, self.rho = grid, parents, mask, rho
        self.m = grid.metrics()
        self.Nx, self.Ny, self.Hx, self.Hy = grid.Nx, grid.Ny, grid.Hx, grid.Hy
        self.I = np.arange(1, self.Nx + 1)[None, :]
        self.J = np.arange(1, self.Ny + 1)[:, None]

    # ---- elements and metrics at (i + di, j + dj) ---------------------------------------------------------------------------------------
    def at(self, name, di=0, dj=0):
        a = self.p[name]
        return a[self.Hy + dj:self.Hy + dj + self.Ny, self.Hx + di:self.Hx + di + self.Nx]

    def metric(self, which, lx, ly, di=0, dj=0):
        """dx / dy / az at location (lx, ly) and index (i + di, j + dj): the same calls as the reference's Oceananigans.Operators"""
        m, one = self.m, np.ones((self.Ny, self.Nx))
        if m["kind"] == "uniform":
            return {"dx": m["dx"], "dy": m["dy"], "az": m["dx"] * m["dy"]}[which] * one
        if m["kind"] == "per_j":
            if which == "dy":
                return m["dy"] * one
            v = np.asarray(m[("dx" if which == "dx" else "az") + ly])
            return v[self.Hy + dj:self.Hy + dj + self.Ny, None] * one
        a = m[which + lx + ly]
        return a[self.Hy + dj:self.Hy + dj + self.Ny, self.Hx + di:self.Hx + di + self.Nx]

    # ---- strain rates, elasto_visco_plastic_rheology.jl:360-375 --------------------------------------------------------------------------
    def eps_D(self, di=0, dj=0):
        u, v, M = self.at, self.at, self.metric
        a = M("dy", F, C, di + 1, dj) * u("u", di + 1, dj) - M("dy", F, C, di, dj) * u("u", di, dj)
        b = M("dx", C, F, di, dj + 1) * v("v", di, dj + 1) - M("dx", C, F, di, dj) * v("v", di, dj)
        return (a + b) / M("az", C, C, di, dj)

    def eps_T(self, di=0, dj=0):
        at, M = self.at, self.metric
        dycc, dxcc = M("dy", C, C, di, dj), M("dx", C, C, di, dj)
        a = at("u", di + 1, dj) / M("dy", F, C, di + 1, dj) - at("u", di, dj) / M("dy", F, C, di, dj)
        b = at("v", di, dj + 1) / M("dx", C, F, di, dj + 1) - at("v", di, dj) / M("dx", C, F, di, dj)
        return ((dycc * dycc) * a - (dxcc * dxcc) * b) / M("az", C, C, di, dj)

    def eps_S(self, di=0, dj=0):
        at, M = self.at, self.metric
        dxff, dyff = M("dx", F, F, di, dj), M("dy", F, F, di, dj)
        a = at("u", di, dj) / M("dx", F, C, di, dj) - at("u", di, dj - 1) / M("dx", F, C, di, dj - 1)
        b = at("v", di, dj) / M("dy", C, F, di, dj) - at("v", di - 1, dj) / M("dy", C, F, di - 1, dj)
        return ((dxff * dxff) * a + (dyff * dyff) * b) / M("az", F, F, di, dj)

    def e11(self, di=0, dj=0):
        return (self.eps_D(di, dj) + self.eps_T(di, dj)) / 2

    def e22(self, di=0, dj=0):
        return (self.eps_D(di, dj) - self.eps_T(di, dj)) / 2

    def e12(self, di=0, dj=0):
        return self.eps_S(di, dj) / 2

    @staticmethod
    def avg4(f00, f10, f01, f11):
        return ((f00 + f10) / 2 + (f01 + f11) / 2) / 2

    # ---- the seven fields ---------------------------------------------------------------------------------------------------------------
    def fields(self, names=NAMES):
        with np.errstate(all="ignore"):
            at = self.at
            e11, e22 = self.e11(), self.e22()
            x = [self.e12(di, dj) for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1))]
            e12c = self.avg4(*x)
            div = e11 + e22
            shear = np.sqrt((e11 - e22) * (e11 - e22) + 4 * (e12c * e12c))
            uc, vc = (at("u") + at("u", 1, 0)) / 2, (at("v") + at("v", 0, 1)) / 2
            out = {"divergence": div, "shear": shear, "deformation": np.sqrt(div * div + shear * shear),
                   "speed": np.sqrt(uc * uc + vc * vc)}
            if any(n in ("sigma_I", "sigma_II", "stress_power") for n in names):
                s11, s22, P = at("s11"), at("s22"), at("P")
                t = [at("s12", di, dj) for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1))]
                s12c = self.avg4(*t)
                half = (s11 - s22) / 2
                out["sigma_I"] = np.where(P == 0, 0.0, ((s11 + s22) / 2) / P)
                out["sigma_II"] = np.where(P == 0, 0.0, np.sqrt(half * half + s12c * s12c) / P)
                out["stress_power"] = (s11 * e11 + s22 * e22) + 2 * self.avg4(*(a * b for a, b in zip(t, x)))
            if self.mask is not None:
                land = self.mask[self.Hy:self.Hy + self.Ny, self.Hx:self.Hx + self.Nx] == 0
                out = {k: np.where(land, 0.0, v) for k, v in out.items()}
            return {n: np.ascontiguousarray(out[n], dtype=np.float64) for n in names}

    # ---- activity (upstream inactive_cell / immersed_peripheral_node) ---------------------------------------------------------------------
    def _outside(self, di, dj):
        i, j, tx, ty = self.I + di, self.J + dj, self.g.topology[0], self.g.topology[1]
        return ((_wall_lo(tx) & (i < 1)) | (_wall_hi(tx) & (i > self.Nx)) | (_wall_lo(ty) & (j < 1)) | (_wall_hi(ty) & (j > self.Ny))) \
            & np.ones((self.Ny, self.Nx), dtype=bool)

    def _inactive(self, di, dj):
        out = self._outside(di, dj)
        if self.mask is not None:
            out = out | (self.mask[self.Hy + dj:self.Hy + dj + self.Ny, self.Hx + di:self.Hx + di + self.Nx] == 0)
        return out

    def _imm_cc(self, di, dj):
        if self.mask is None:
            return np.zeros((self.Ny, self.Nx), dtype=bool)
        return self._inactive(di, dj) & ~self._outside(di, dj)

    def _imm_ff(self, di, dj):
        if self.mask is None:
            return np.zeros((self.Ny, self.Nx), dtype=bool)
        four = ((di, dj), (di - 1, dj), (di, dj - 1), (di - 1, dj - 1))
        p = np.logical_or.reduce([self._inactive(a, b) for a, b in four])
        pu = np.logical_or.reduce([self._outside(a, b) for a, b in four])
        return p & ~pu

    # ---- stress divergence, ice_stress_divergence.jl:16-51 -----------------------------------------------------------------------------------
    def sig(self, name, di=0, dj=0):
        imm = self._imm_ff(di, dj) if name == "s12" else self._imm_cc(di, dj)
        return np.where(imm, 0.0, self.at(name, di, dj))

    def sigD(self, di=0, dj=0):
        return self.sig("s11", di, dj) + self.sig("s22", di, dj)

    def sigT(self, di=0, dj=0):
        return self.sig("s11", di, dj) - self.sig("s22", di, dj)

    def div_sigma_1(self):
        M = self.metric
        dyfc = M("dy", F, C)
        d = dyfc * (self.sigD() - self.sigD(-1, 0)) / 2
        dyc, dycm = M("dy", C, C), M("dy", C, C, -1, 0)
        T = ((dyc * dyc) * self.sigT() - (dycm * dycm) * self.sigT(-1, 0)) / dyfc / 2
        dxfn, dxf = M("dx", F, F, 0, 1), M("dx", F, F)
        S = ((dxfn * dxfn) * self.sig("s12", 0, 1) - (dxf * dxf) * self.sig("s12")) / M("dx", F, C)
        return (d + T + S) / M("az", F, C)

    def div_sigma_2(self):
        M = self.metric
        dxcf = M("dx", C, F)
        d = dxcf * (self.sigD() - self.sigD(0, -1)) / 2
        dxc, dxcm = M("dx", C, C), M("dx", C, C, 0, -1)
        T = -((dxc * dxc) * self.sigT() - (dxcm * dxcm) * self.sigT(0, -1)) / dxcf / 2
        dyfn, dyf = M("dy", F, F, 1, 0), M("dy", F, F)
        S = ((dyfn * dyfn) * self.sig("s12", 1, 0) - (dyf * dyf) * self.sig("s12")) / M("dy", C, F)
        return (d + T + S) / M("az", C, F)

    def old_div_sigma(self):
        """the flux-form operator the reference's test keeps for contrast (test/test_rheology_energy_budget.jl:22-32)"""
        at, M = self.at, self.metric
        a = M("dy", C, C) * at("s11") - M("dy", C, C, -1, 0) * at("s11", -1, 0)
        b = M("dx", F, F, 0, 1) * at("s12", 0, 1) - M("dx", F, F) * at("s12")
        d1 = (a + b) / M("az", F, C)
        a = M("dy", F, F, 1, 0) * at("s12", 1, 0) - M("dy", F, F) * at("s12")
        b = M("dx", C, C) * at("s22") - M("dx", C, C, 0, -1) * at("s22", 0, -1)
        return d1, (a + b) / M("az", C, F)

    # ---- the three sums: one term per cell, formed in the order of test/test_rheology_energy_budget.jl:77-88 -------------------------------
    def terms(self, what=SUMS, old=False):
        at, M, out = self.at, self.metric, {}
        with np.errstate(all="ignore"):
            u, v, azfc, azcf = at("u"), at("v"), M("az", F, C), M("az", C, F)
            if "internal_work" in what:
                d1, d2 = self.old_div_sigma() if old else (self.div_sigma_1(), self.div_sigma_2())
                out["internal_work"] = (u * d1) * azfc + (v * d2) * azcf
            if "stress_power" in what:
                azcc, azff = M("az", C, C), M("az", F, F)
                out["stress_power"] = ((at("s11") * self.e11()) * azcc + (at("s22") * self.e22()) * azcc) + ((2 * at("s12")) * self.e12()) * azff
            if "kinetic_energy" in what:
                mass = lambda di, dj: at("h", di, dj) * self.rho * at("a", di, dj)
                mu, mv = (mass(-1, 0) + mass(0, 0)) / 2, (mass(0, -1) + mass(0, 0)) / 2
                out["kinetic_energy"] = ((0.5 * mu) * (u * u)) * azfc + ((0.5 * mv) * (v * v)) * azcf
        return {k: np.ascontiguousarray(t, dtype=np.float64) for k, t in out.items()}

    def budget(self, what=SUMS, old=False):
        return {k: dref.ordered_sum(t) for k, t in self.terms(what, old).items()}


def imbalance(W, D):
    """relative_imbalance of test/test_rheology_energy_budget.jl:93"""
    return abs(W + D) / max(abs(W), abs(D))


def same_bits(a, b):
    """Arrays equal bit for bit (-0.0 != +0.0), NaN equal to NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


# ---- inputs shared by tests/test_derived_ref.py (CPU) and tests/test_gpu_derived.py -------------------------------------------------------
# The block edges of the two kernels: 37 x 29 (narrower than a wave, partial everywhere), 64 x 16 (fewer rows than a budget block, exact
# derived blocks), 65 x 65 (a one-column last block column, a one-row last block row), 130 x 33 (a two-column last block column)
SHAPES = ((37, 29), (64, 16), (65, 65), (130, 33))
TOPOS = {"periodic": ("periodic", "periodic"), "channel": ("periodic", "bounded"), "bounded": ("bounded", "bounded")}
METRICS = ("uniform", "latlon", "curvilinear")


def grid_of(Nx, Ny, topo, metrics, H=4, seed=3):
    T = {"periodic": csi.Periodic, "bounded": csi.Bounded}
    tt = (T[topo[0]], T[topo[1]])
    if metrics in ("uniform", "distorted_rectilinear"):      # (the second: per-point metrics whose Periodic halos are exact images)
        g = csi.RectilinearGrid((Nx, Ny), x=(0.0, Nx * 2000.0), y=(0.0, Ny * 2000.0), topology=tt, halo=(H, H))
        return g if metrics == "uniform" else csi.OrthogonalCurvilinearGrid.from_grid(g, distort=0.05, seed=seed)
    g = csi.LatitudeLongitudeGrid((Nx, Ny), longitude=(0, 60), latitude=(20, 70), topology=tt, halo=(H, H))
    return csi.OrthogonalCurvilinearGrid.from_grid(g, distort=0.05, seed=seed) if metrics == "curvilinear" else g


def parent_shape(g, name):
    loc = {"u": (csi.Face, csi.Center), "v": (csi.Center, csi.Face), "s12": (csi.Face, csi.Face)}.get(name, (csi.Center, csi.Center))
    ni, nj = g.field_size(*loc)
    return nj, ni


# the elements each entry point may read, as (first column, last column - Nx, first row, last row - Ny) in reference indices
CONTRACT = {
    "derived": {"u": (1, 1, 0, 1), "v": (0, 1, 1, 1), "s12": (1, 1, 1, 1), "s11": (1, 0, 1, 0), "s22": (1, 0, 1, 0), "P": (1, 0, 1, 0)},
    "budget": {"u": (1, 1, 0, 1), "v": (0, 1, 1, 1), "s12": (1, 1, 1, 1), "s11": (0, 0, 0, 0), "s22": (0, 0, 0, 0), "h": (0, 0, 0, 0),
               "a": (0, 0, 0, 0)},
}


def white_noise(g, seed=11, land=False, poison=None, zero_P=True, margin=0, unit=False):
    """Seeded white-noise parents of u, v, sigma, P, h, a on grid g, halos included (every element is its own random number: no fill
    semantics enter), P == 0 in a patch and one single cell.  poison = "derived" / "budget": every element outside what that entry point
    may read is NaN.  margin: that many cells next to (and the faces on) every Bounded side are zero, as are all halos there -- the
    reference test's set_smooth! margin; periodic directions then get wrapped halos.  unit: unit variance for every field (default: magnitudes
    of a model run, so that a wrong factor cannot hide behind equal scales).  Returns (parents, (Ny, Nx) wet cells or None)."""
    rng = np.random.default_rng(seed)
    Nx, Ny, Hx, Hy = g.Nx, g.Ny, g.Hx, g.Hy
    scale = {"u": 0.1, "v": 0.1, "s11": 1e3, "s22": 1e3, "s12": 5e2, "P": 1e4, "h": 1.0, "a": 1.0}
    if unit:                # every field of amplitude one, as the smooth fields of test/test_rheology_energy_budget.jl:67-71 are
        scale = {k: 1.0 for k in scale}
    par = {}
    for name, s in scale.items():
        a = s * rng.standard_normal(parent_shape(g, name))
        if name in ("P", "h", "a"):
            a = np.abs(a)
        par[name] = a
    if zero_P:
        par["P"][Hy + Ny // 3:Hy + Ny // 3 + 3, Hx + Nx // 4:Hx + Nx // 4 + 5] = 0.0
        par["P"][Hy + Ny - 1, Hx + Nx - 1] = 0.0
    if margin:
        for name, a in par.items():
            nj, ni = a.shape
            for axis, topo, N, H in ((1, g.topology[0], Nx, Hx), (0, g.topology[1], Ny, Hy)):
                idx = [slice(None), slice(None)]
                if topo is csi.Bounded:
                    idx[axis] = slice(0, H + margin)
                    a[tuple(idx)] = 0.0
                    idx[axis] = slice(H + N - margin, None)
                    a[tuple(idx)] = 0.0
            for axis, topo, N, H in ((1, g.topology[0], Nx, Hx), (0, g.topology[1], Ny, Hy)):
                if topo is csi.Periodic:                                    # wrapped halos (after the zero margins of the other direction)
                    lo, hi = [slice(None)] * 2, [slice(None)] * 2
                    src_lo, src_hi = [slice(None)] * 2, [slice(None)] * 2
                    lo[axis], src_lo[axis] = slice(0, H), slice(N, N + H)
                    hi[axis], src_hi[axis] = slice(N + H, N + 2 * H), slice(H, 2 * H)
                    a[tuple(lo)] = a[tuple(src_lo)]
                    a[tuple(hi)] = a[tuple(src_hi)]
    wet = (np.random.default_rng(seed + 1).random((Ny, Nx)) > 0.2) if land else None
    if poison:
        for name, (c0, c1, r0, r1) in CONTRACT[poison].items():
            a = par[name]
            keep = np.zeros(a.shape, dtype=bool)
            keep[Hy - 1 + r0:Hy + Ny + r1, Hx - 1 + c0:Hx + Nx + c1] = True
            a[~keep] = np.nan
    return par, wet


def mask_parent(g, wet):
    """The activity mask's parent as SeaIceModel.set_mask and cases.oracle_problem build it from the (Ny, Nx) wet cells: wrapped in
    Periodic directions, inactive beyond walls."""
    if wet is None:
        return None
    full = np.zeros((g.Ny + 2 * g.Hy, g.Nx + 2 * g.Hx), dtype=np.uint8)
    full[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx] = wet
    if g.topology[0] is csi.Periodic:
        full[:, :g.Hx] = full[:, g.Nx:g.Nx + g.Hx]
        full[:, g.Nx + g.Hx:] = full[:, g.Hx:2 * g.Hx]
    if g.topology[1] is csi.Periodic:
        full[:g.Hy, :] = full[g.Ny:g.Ny + g.Hy, :]
        full[g.Ny + g.Hy:, :] = full[g.Hy:2 * g.Hy, :]
    return full
