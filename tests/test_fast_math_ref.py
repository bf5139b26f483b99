"""CPU side of the FAST-arithmetic tests (no GPU):

  * the refinement bounds of rcp / rsqrt / sqrt_fast (tests/fast_math_ref.py, asserted on the hardware by tests/test_gpu_fast_math.py)
    re-derived and checked by exact rational emulation of the steps with correctly rounded fused multiply-adds;
  * the per-cell high-precision restatement of the reference (tests/fast_math_ref.py) tied to the CPU oracle (oracle/, strict double
    order) on one stress phase and one velocity phase of a tiny case, so that "the reference" means what the rest of the suite means;
  * the stencil coefficients of csrc/csi_fast_coef.h against the reference's operators in exact rationals.
"""
import ctypes as C
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

import cases
import fast_math_build
import fast_math_ref as R
from fast_math_ref import D, U


# ---- 1. one refinement step, exactly ------------------------------------------------------------------------------------------------

def fl(q):
    """round-to-nearest-even of a rational to double (Fraction.__float__ divides two integers: correctly rounded)"""
    return float(q)


def fma(a, b, c):
    return fl(Fr(a) * Fr(b) + Fr(c))


def emu_rcp(x, r):
    return fma(fma(-x, r, 1.0), r, r)


def emu_rsqrt(x, y):
    g, h = fl(Fr(x) * Fr(y)), 0.5 * y
    r = fma(-h, g, 0.5)
    return fma(y, r, y)


def emu_sqrt_fast(x, y):
    g, h = fl(Fr(x) * Fr(y)), 0.5 * y
    r = fma(-h, g, 0.5)
    return fma(g, r, g)


def sqrt_hp(x):
    with R.hp():
        return D(x).sqrt()


def test_refinement_step_bounds_by_exact_emulation():
    """The bounds asserted on the hardware, derived (d1, d2, d3: roundings of at most u = 2^-53 each; every fma rounds once):

    rcp: r the seed, e = 1 - x r exactly.  t = fl(e) = e (1 + d1); result = (r + r t)(1 + d2) and 1 / x = r / (1 - e), so
      result x = (1 - e)(1 + e + e d1)(1 + d2) = (1 - e^2 + e d1 (1 - e))(1 + d2):   |result x - 1| <= e^2 + |e| u + u (1 + ...) <= e^2 + 2 u.
    rsqrt: y the seed, y sqrt(x) = 1 + e.  g = x y (1 + d1), h = y / 2 exactly, r = (1/2 - h g)(1 + d2) with
      1/2 - h g = -e - e^2 / 2 - (1 + e)^2 d1 / 2;  result = y (1 + r)(1 + d3), so
      result sqrt(x) = (1 + e)(1 - e - e^2 / 2 - d1 / 2 + ...)(1 + d3) = 1 - 3 e^2 / 2 - d1 / 2 + d3 + O(e^3, e u):   <= 1.5 e^2 + 2 u.
    sqrt_fast: result = g (1 + r)(1 + d3), g = sqrt(x)(1 + e)(1 + d1):  1 - 3 e^2 / 2 + d1 / 2 + d3 + ...:             <= 1.5 e^2 + 2 u.

    Checked here with synthetic seeds of relative error up to 2^-23 (the cap of the GPU test) on random arguments: the exact error of
    the emulated step never exceeds the bound, and at seed errors of 2^-24 .. 2^-23 it reaches more than half of it (the bounds are
    not slack by an order of magnitude)."""
    rng = np.random.default_rng(11)
    worst = dict(rcp=0.0, rsqrt=0.0, sqrt=0.0)
    for k in range(1500):
        x = float(rng.uniform(1.0, 4.0) * 2.0 ** int(rng.integers(-300, 300)))
        mag = 2.0 ** -float(rng.uniform(23.0, 30.0)) if k % 3 else 2.0 ** -float(rng.uniform(23.0, 24.0))
        e = mag * (1 if rng.random() < 0.5 else -1)
        r = (1.0 / x) * (1.0 + e)
        with R.hp():
            sx = D(x).sqrt()
            y = float(1 / sx) * (1.0 + e)
            er = abs(D(r) * D(x) - 1)
            ey = abs(D(y) * sx - 1)
            assert er <= D(R.SEED_CAP) * D(1.01) and ey <= D(R.SEED_CAP) * D(1.01)
            cases_ = (("rcp", abs(D(emu_rcp(x, r)) * D(x) - 1), er * er + 2 * D(U)),
                      ("rsqrt", abs(D(emu_rsqrt(x, y)) * sx - 1), D("1.5") * ey * ey + 2 * D(U)),
                      ("sqrt", abs(D(emu_sqrt_fast(x, y)) / sx - 1), D("1.5") * ey * ey + 2 * D(U)))
            for name, err, bound in cases_:
                assert err <= bound, (name, x, e, float(err), float(bound))
                if mag >= 2.0 ** -24:
                    worst[name] = max(worst[name], float(err / bound))
    print("worst error / bound at seed errors 2^-24 .. 2^-23:", worst)
    assert all(v > 0.5 for v in worst.values()), worst
    # the constants under the cap, as fast_math_ref.py states them
    assert R.RCP_U == R.SEED_CAP ** 2 / U + 2 and R.RSQ_U == 1.5 * R.SEED_CAP ** 2 / U + 2


# ---- 2. the restatement against the oracle ------------------------------------------------------------------------------------------

# Forward error of the ORACLE (every operation, division and square root included, rounds once: 1 u) against the exact evaluation of the
# same formulas on the same double inputs, by the analysis of fast_math_ref.py's docstring with the oracle's operation sequence (e = 2):
#   s = sqrt(t t + 4 e12^2): 3 u;  Delta = sqrt(dc dc + (s s) em2): (max(3, 8) + 1) / 2 + 1 = 5.5;  zeta = P / (2 Delta): 6.5
#   P_r = P Delta / (Delta + Dmin): 6.5 + 6.5 + 1 = 14;  eta: 7.5;  T = 2 eta e: 8.5
#   zeta - eta = 0.75 zeta: (6.5 + 7.5 / 4) / 0.75 + 1 < 13;  A = (zeta - eta)(e11 + e22): 15
#   sigma' = T + (A - B): SN = max(8.5 + 1, 15 + 2, 14 + 2) = 17
#   gamma^2 = zeta c dt / m / Az: 10.5;  gamma = sqrt: 6.25 -> K_ALPHA_ORACLE = 7;  (sigma' - sigma) / gamma: + 7.25;  sigma +=: + 1
#   K_SIGMA_ORACLE = 17 + 7.25 + 1 + 2 -> 28
#   velocity: G has at most (4 + 5) u of its absolute terms, dtau G: 11, numerator 12; tau_i: drag norm 3 + product 1 + / m * a 2 + 1 = 7,
#   denominator (positive terms) 10, quotient 1:  K_VEL_ORACLE = 12 + 10 + 1 -> 24
K_SIGMA_ORACLE, K_ALPHA_ORACLE, K_VEL_ORACLE = 28, 7, 24


def avg4(a, b, c, d):
    """Ixy in the oracle's order on doubles (numpy float64 scalars round like C doubles: the oracle's bits)"""
    return ((np.float64(a) + np.float64(b)) / 2 + (np.float64(c) + np.float64(d)) / 2) / 2


def test_restatement_matches_the_oracle_on_one_stress_and_one_velocity_phase(oracle_lib):
    c = cases.make_case(Nx=8, Ny=8, substeps=2, random_uv=0.02, coriolis=1e-4)
    c["h"][1:3, 2:4], c["a"][1:3, 2:4] = 0.0, 0.0              # open water two cells wide: u points with no ice on either side
    c["h"][4:6, 2:4], c["a"][4:6, 2:4] = 1e-3, 5e-4            # ... and with marginal ice on both sides
    p = cases.oracle_problem(c)
    s, L = p.s, p.L
    dt = c["dt"] / 1.0
    p.initialize_rheology()
    at = lambda name, i, j: p.f[name][j + s.Hy - 1, i + s.Hx - 1]
    mass = lambda i, j: np.float64(at("h", i, j)) * np.float64(s.rho_ice) * np.float64(at("aice", i, j))
    cells = [(i, j) for j in range(1, 9) for i in range(1, 9)]
    exx = {(i, j): L.ora_strain_xx(p.ptr, i, j) for j in range(0, 10) for i in range(0, 10)}
    eyy = {(i, j): L.ora_strain_yy(p.ptr, i, j) for j in range(0, 10) for i in range(0, 10)}
    exy = {(i, j): L.ora_strain_xy(p.ptr, i, j) for j in range(0, 11) for i in range(0, 11)}
    ff = lambda f, i, j: avg4(f[(i - 1, j - 1)], f[(i, j - 1)], f[(i - 1, j)], f[(i, j)])
    cc = lambda f, i, j: avg4(f[(i, j)], f[(i + 1, j)], f[(i, j + 1)], f[(i + 1, j + 1)])
    old = {n: p.f[n].copy() for n in ("s11", "s22", "s12")}
    k = R.stress_constants(ecc=s.ecc, Dmin=s.delta_min, amin=s.alpha_min, amax=s.alpha_max, pressure_kind=s.pressure_kind)
    p.compute_stresses(dt)
    az = s.dx * s.dy
    n_ice_free = 0
    with R.hp():
        hk = D(s.c_alpha) * D(dt) / D(az) / 2
        for (i, j) in cells:
            Pf = avg4(at("P", i - 1, j - 1), at("P", i, j - 1), at("P", i - 1, j), at("P", i, j))
            mf = avg4(mass(i - 1, j - 1), mass(i, j - 1), mass(i - 1, j), mass(i, j))
            o = lambda n: old[n][j + s.Hy - 1, i + s.Hx - 1]
            r = R.stress_cell(k, exx[(i, j)], eyy[(i, j)], exy[(i, j)], ff(exx, i, j), ff(eyy, i, j), cc(exy, i, j), at("P", i, j), Pf,
                              mass(i, j), mf, hk, hk, o("s11"), o("s22"), o("s12"))
            n_ice_free += mass(i, j) == 0
            for q, name, Nq, g in ((0, "s11", r[4], r[7]), (1, "s22", r[5], r[7]), (2, "s12", r[6], r[8])):
                err, bound = abs(D(float(at(name, i, j))) - r[q]), K_SIGMA_ORACLE * R.stress_bound(o(name), Nq, g)
                assert err <= bound, (name, i, j, float(err), float(bound))
                if (mass(i, j) if q < 2 else mf) <= 0:
                    assert at(name, i, j) == o(name)
            assert abs(D(float(at("alpha", i, j))) - r[3]) <= K_ALPHA_ORACLE * R.DU * r[3], (i, j)
    assert n_ice_free > 0                                     # the open-water patch: the m = 0 branch was compared too

    # one u step on the new stresses: bottom SemiImplicitStress against an ocean at rest, constant top stress, Coriolis
    u_old, v_old = p.f["u"].copy(), p.f["v"].copy()
    uo = lambda i, j: u_old[j + s.Hy - 1, i + s.Hx - 1]
    vo = lambda i, j: v_old[j + s.Hy - 1, i + s.Hx - 1]
    div = {(i, j): L.ora_div_sigma_1(p.ptr, i, j) for (i, j) in cells}
    p.u_step(dt)
    kv = dict(dt=dt, min_mass=s.min_mass, min_conc=s.min_conc)
    rhoCd = np.float64(s.bottom.rho_e) * np.float64(s.bottom.Cd)
    decisions = set()
    with R.hp():
        for (i, j) in cells:
            mi = (mass(i - 1, j) + mass(i, j)) / 2
            ai = (np.float64(at("aice", i - 1, j)) + np.float64(at("aice", i, j))) / 2
            abar = (np.float64(at("alpha", i - 1, j)) + np.float64(at("alpha", i, j))) / 2
            vbar = avg4(vo(i - 1, j), vo(i, j), vo(i - 1, j + 1), vo(i, j + 1))
            cor = np.float64(s.f_coriolis) * vbar               # G = -x_f_cross_U + ..., x_f_cross_U = -f vbar
            exb, imb = R.ext_stress_cell(3, 0.0, rhoCd, 0.0, 0.0, uo(i, j), vbar)
            res, what, cond = R.vel_cell(kv, uo(i, j), at("un", i, j), mi, ai, abar, div[(i, j)], cor, s.top.tau_u, 0.0, exb, imb, False)
            decisions.add(what)
            got = float(at("u", i, j))
            if what != R.ACTIVE:
                assert got == 0.0 and res == 0, (i, j, got)
            else:
                assert abs(D(got) - res) <= K_VEL_ORACLE * R.DU * cond, (i, j, got, float(res))
    assert decisions == {R.ZERO, R.ACTIVE, R.MARGINAL}


# ---- 3. the stencil coefficients --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def coef_lib():
    L = C.CDLL(fast_math_build.build_coef())
    pd = C.POINTER(C.c_double)
    L.fch_pair_coef_scale.restype = C.c_double
    L.fch_pair_coef_scale.argtypes = [C.c_int]
    L.fch_uniform.argtypes = [C.c_double, C.c_double, pd]
    L.fch_per_j.argtypes = [C.c_int, C.c_double, pd, pd, pd, pd, pd]
    L.fch_full.argtypes = [C.c_int, C.c_int, C.POINTER(pd), pd]
    L.fch_fast_params_supported.argtypes = [C.c_double, C.c_double]
    return L


# csi_fast_coef.h's enum, in its order
FC = {n: k for k, n in enumerate(["A", "CN", "BN", "BS", "CS", "RAZC", "RAZF", "SN", "SV", "SS", "E", "FN", "FS", "FU", "Q2N", "K", "FV",
                                  "Q1N", "Q1S", "Q2S"])}
C2 = {n: k for k, n in enumerate(["DYU", "RDXU", "RAZU", "DXV", "RDYV", "RAZV", "DYC2", "DXC2", "RAZC", "DXF2", "DYF2", "RAZF"])}


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def latlon_rows(n, top=89.9, dphi=1.25, dlam=1.0, radius=6371e3):
    """Row metrics of a regular latitude-longitude grid whose last cell centre lies at `top` degrees (Oceananigans' formulas as in
    climaseaice_jl_amd.LatitudeLongitudeGrid): dx^c, dx^f, Az^c, Az^f per row, dy."""
    phic = top - dphi * (n - 1 - np.arange(n))
    phif = phic - 0.5 * dphi
    dl = np.deg2rad(dlam)
    dxc, dxf = radius * np.cos(np.deg2rad(phic)) * dl, radius * np.cos(np.deg2rad(phif)) * dl
    azc = radius * radius * dl * (np.sin(np.deg2rad(phif + dphi)) - np.sin(np.deg2rad(phif)))
    azf = radius * radius * dl * (np.sin(np.deg2rad(phic)) - np.sin(np.deg2rad(phic - dphi)))
    return dxc, dxf, azc, azf, radius * np.deg2rad(dphi)


def check_operators(coef, dxc, dxf, azc, azf, dy, rows, seed):
    """coef[w][t]: the double coefficients; the metrics are doubles, exact as rationals.  For every row t in `rows` and a few columns of
    random fields: the reference's operators with the metrics INSIDE the differences (evp:360-375, ice_stress_divergence.jl:39-51; on
    these grids dy is a constant, dx and Az depend on the row only), in exact rationals, against sum(coefficient value), also exact.

    Bound, derived: a coefficient is a product / quotient of k metric factors and 1 / Az (k + 1 roundings at most: k <= 4, so 5 u of
    the piece), or half the sum or difference of two such PIECES (+ 1 u).  BN, BS, Q1N, Q1S are differences of two nearly equal pieces
    (dx^f / Az and dx^c dx^c / dx^f / Az): their error is 6 u of the pieces, not of the folded coefficient, which is why the bound sums
    |piece value| -- the reference's own double evaluation carries the same piece-relative error.  K_c = 6:
        |reference - sum(coefficient value)| <= 6 u sum(|piece| |value|)."""
    rng = np.random.default_rng(seed)
    F = lambda a: [Fr(float(v)) for v in a]
    dxc, dxf, azc, azf, dy = F(dxc), F(dxf), F(azc), F(azf), Fr(float(dy))
    n = len(dxc)
    ni = 4
    fld = lambda: [[Fr(float(v)) for v in row] for row in rng.uniform(-1.0, 1.0, (n + 1, ni + 2))]
    u, v, s11, s22, s12 = fld(), fld(), fld(), fld(), fld()
    c = lambda w, t: Fr(float(coef[FC[w]][t]))
    Kc, worst, worst_c = 6, 0.0, 0.0
    for t in rows:
        for i in range(1, ni + 1):
            # strain rates at cell (i, t) / corner (i, t)
            eD = (dy * u[t][i + 1] - dy * u[t][i] + dxf[t + 1] * v[t + 1][i] - dxf[t] * v[t][i]) / azc[t]
            eT = (dy ** 2 * (u[t][i + 1] / dy - u[t][i] / dy) - dxc[t] ** 2 * (v[t + 1][i] / dxf[t + 1] - v[t][i] / dxf[t])) / azc[t]
            eS = (dxf[t] ** 2 * (u[t][i] / dxc[t] - u[t - 1][i] / dxc[t - 1]) + dy ** 2 * (v[t][i] / dy - v[t][i - 1] / dy)) / azf[t]
            pn, ps = dxf[t + 1] / azc[t], dxf[t] / azc[t]
            qn, qs = dxc[t] ** 2 / dxf[t + 1] / azc[t], dxc[t] ** 2 / dxf[t] / azc[t]
            pieces_v = (abs(pn) + abs(qn)) / 2 * abs(v[t + 1][i]) + (abs(ps) + abs(qs)) / 2 * abs(v[t][i])
            pairs = [
                ("e11", (eD + eT) / 2, c("A", t) * (u[t][i + 1] - u[t][i]) + c("BN", t) * v[t + 1][i] - c("BS", t) * v[t][i],
                 abs(c("A", t)) * (abs(u[t][i + 1]) + abs(u[t][i])) + pieces_v),
                ("e22", (eD - eT) / 2, c("CN", t) * v[t + 1][i] - c("CS", t) * v[t][i], pieces_v),
                ("e12", eS / 2, c("SN", t) * u[t][i] - c("SS", t) * u[t - 1][i] + c("SV", t) * (v[t][i] - v[t][i - 1]),
                 abs(c("SN", t) * u[t][i]) + abs(c("SS", t) * u[t - 1][i]) + abs(c("SV", t)) * (abs(v[t][i]) + abs(v[t][i - 1]))),
            ]
            # stress divergences at the u point (i, t) / v point (i, t)
            sD = lambda tt, ii: s11[tt][ii] + s22[tt][ii]
            sT = lambda tt, ii: s11[tt][ii] - s22[tt][ii]
            d1 = (dy * (sD(t, i) - sD(t, i - 1)) / 2 + (dy ** 2 * sT(t, i) - dy ** 2 * sT(t, i - 1)) / dy / 2
                  + (dxf[t + 1] ** 2 * s12[t + 1][i] - dxf[t] ** 2 * s12[t][i]) / dxc[t]) / azc[t]
            d2 = (dxf[t] * (sD(t, i) - sD(t - 1, i)) / 2 - (dxc[t] ** 2 * sT(t, i) - dxc[t - 1] ** 2 * sT(t - 1, i)) / dxf[t] / 2
                  + (dy ** 2 * s12[t][i + 1] - dy ** 2 * s12[t][i]) / dy) / azf[t]
            G, Hn, Hs = dxf[t] / azf[t] / 2, dxc[t] ** 2 / dxf[t] / azf[t] / 2, dxc[t - 1] ** 2 / dxf[t] / azf[t] / 2
            pairs += [
                ("div1", d1, c("E", t) * (s11[t][i] - s11[t][i - 1]) + c("FN", t) * s12[t + 1][i] - c("FS", t) * s12[t][i],
                 abs(c("E", t)) * (abs(s11[t][i]) + abs(s11[t][i - 1])) + abs(c("FN", t) * s12[t + 1][i]) + abs(c("FS", t) * s12[t][i])),
                ("div2", d2, c("Q1N", t) * s11[t][i] + c("Q2N", t) * s22[t][i] - c("Q1S", t) * s11[t - 1][i] - c("Q2S", t) * s22[t - 1][i]
                 + c("K", t) * (s12[t][i + 1] - s12[t][i]),
                 (G + Hn) * (abs(s11[t][i]) + abs(s22[t][i])) + (G + Hs) * (abs(s11[t - 1][i]) + abs(s22[t - 1][i]))
                 + abs(c("K", t)) * (abs(s12[t][i + 1]) + abs(s12[t][i]))),
            ]
            if i == 1:
                # the coefficients that are no difference of nearly equal pieces, each against its exact rational value, relative to ITSELF
                # (at most 5 roundings each: K_c = 6 covers them one by one, which is the issue's sum|coefficient value| form for them)
                exact = dict(A=dy / azc[t], CN=(pn + qn) / 2, CS=(ps + qs) / 2, SN=dxf[t] ** 2 / dxc[t] / azf[t] / 2,
                             SS=dxf[t] ** 2 / dxc[t - 1] / azf[t] / 2, SV=dy / azf[t] / 2, E=dy / azc[t], FN=dxf[t + 1] ** 2 / dxc[t] / azc[t],
                             FS=dxf[t] ** 2 / dxc[t] / azc[t], Q2N=G + Hn, Q2S=G + Hs, K=dy / azf[t])
                for w, val in exact.items():
                    assert abs(c(w, t) - val) <= Kc * Fr(U) * abs(val), (w, t, float(abs(c(w, t) - val) / abs(val)) / U)
                    worst_c = max(worst_c, float(abs(c(w, t) - val) / abs(val)) / U)
            for name, ref, got, scale in pairs:
                bound = Kc * Fr(U) * scale
                assert abs(ref - got) <= bound, (name, t, i, float(abs(ref - got)), float(bound))
                worst = max(worst, float(abs(ref - got) / bound))
        assert coef[FC["RAZC"]][t] == 1.0 / float(azc[t]) and coef[FC["RAZF"]][t] == 1.0 / float(azf[t])
    print(f"worst single coefficient: {worst_c:.2f} u of itself (bound {Kc} u)")
    return worst


def test_per_row_coefficients_reproduce_the_reference_operators(coef_lib):
    """A regular latitude-longitude grid whose last row of cells is centred at 89.9 degrees (dx shrinks by a factor of 700 across the
    table; BN, BS, Q1N, Q1S are small differences of large pieces everywhere).  Every row whose neighbours exist is compared: the two
    edge rows of the table are built from CLAMPED neighbours (csi_fast_coef.h) and are wrong on purpose -- see the next test."""
    n = 61
    ext = latlon_rows(n + 2)
    dy = ext[4]
    assert all(a.min() > 0 for a in ext[:4]) and ext[0][0] / ext[0][-1] > 100
    big = np.zeros((len(FC), n + 2))
    coef_lib.fch_per_j(n + 2, dy, dptr(ext[0]), dptr(ext[1]), dptr(ext[2]), dptr(ext[3]), dptr(big))
    worst = check_operators(big, ext[0], ext[1], ext[2], ext[3], dy, range(1, n + 1), seed=5)
    print(f"per-row coefficients: worst |error| / bound = {worst:.3f}")
    # the table of the same rows without the first and the last: the clamped entries of ITS edge rows differ from what the real
    # neighbour gives; every other entry, of those rows too, is the same
    dxc, dxf, azc, azf = [np.ascontiguousarray(a[1:-1]) for a in ext[:4]]
    out = np.zeros((len(FC), n))
    coef_lib.fch_per_j(n, dy, dptr(dxc), dptr(dxf), dptr(azc), dptr(azf), dptr(out))
    uses_south, uses_north = ["SS", "Q1S", "Q2S"], ["BN", "CN", "FN"]
    for w, k in FC.items():
        if w in ("FU", "FV"):
            continue
        assert np.array_equal(out[k][1:-1], big[k][2:-2]), w
        assert (out[k][0] != big[k][1]) == (w in uses_south), w
        assert (out[k][-1] != big[k][-2]) == (w in uses_north), w


def test_clamped_edge_rows_of_the_coefficient_table_are_never_launched():
    """The table has one row per j in [1 - Hy, Ny + Hy + 1] (FastCoef.jmin, jmax: csi_core.hip); its first and last rows hold clamped
    neighbours.  Every range the launch plan can produce stays strictly inside: a stencil of row j reads coefficient row j only."""
    from climaseaice_jl_amd import _lib
    topos = (_lib.PERIODIC, _lib.BOUNDED, _lib.RIGHT_FOLDED)
    for Nx, Ny, H in ((8, 8, 3), (37, 29, 4), (64, 130, 4), (256, 256, 5)):
        jmin, jmax = 1 - H, Ny + H + 1
        for tx in (_lib.PERIODIC, _lib.BOUNDED):
            for ty in topos:
                try:
                    ranges = _lib.plan_ranges(Nx, Ny, H, H, tx, ty)
                except _lib.CsiError:
                    continue                                      # not a topology the library takes
                for (i0, i1, j0, j1) in ranges:
                    assert jmin < j0 and j1 < jmax, (Nx, Ny, H, tx, ty, j0, j1)
                p = _lib.plan_pair(Nx, Ny, H, H, tx, ty)
                if p is not None:
                    for key in ("first_compute", "second_compute", "store_sigma", "store_first_u", "store_first_v", "store_second"):
                        assert jmin < p[key][2] and p[key][3] < jmax, (key, p[key])


def test_uniform_coefficients_and_the_pair_scaling(coef_lib):
    dx, dy = 2000.0 / 3.0, 1234.5678
    uni = np.zeros(len(FC))
    coef_lib.fch_uniform(dx, dy, dptr(uni))
    n = 5
    rows = lambda v: np.full(n, v)
    out = np.repeat(uni[:, None], n, axis=1)
    worst = check_operators(out, rows(dx), rows(dx), rows(dx * dy), rows(dx * dy), dy, range(1, n - 1), seed=6)
    print(f"uniform coefficients: worst |error| / bound = {worst:.3f}")
    # what the UNI kernels assume (evp_fast_math.h strain_cell<true>, strain_corner<true>, div2<true>)
    assert uni[FC["CN"]] == uni[FC["CS"]] and uni[FC["SN"]] == uni[FC["SS"]] and uni[FC["Q2N"]] == uni[FC["Q2S"]]
    assert uni[FC["FN"]] == uni[FC["FS"]] and uni[FC["BN"]] == uni[FC["BS"]] and uni[FC["Q1N"]] == uni[FC["Q1S"]]
    # the pair kernel's copy is scaled by exact powers of two
    for w, k in FC.items():
        sc = coef_lib.fch_pair_coef_scale(k)
        assert sc == (8.0 if w in ("SN", "SS", "SV") else 2.0 if w in ("E", "FN", "FS", "Q1N", "Q2N", "Q1S", "Q2S", "K") else 1.0), w


def test_full_metric_planes_hold_the_metric_its_square_or_its_correctly_rounded_reciprocal(coef_lib):
    rng = np.random.default_rng(8)
    ni, nj = 7, 5
    m = [np.ascontiguousarray(rng.uniform(0.3, 3.0, (nj, ni)) * 10.0 ** rng.integers(-2, 6)) for _ in range(12)]
    arr = (C.POINTER(C.c_double) * 12)(*[dptr(a) for a in m])
    out = np.zeros((len(C2), nj, ni))
    coef_lib.fch_full(ni, nj, arr, dptr(out))
    M = lambda which, loc: m[4 * which + loc]          # which: dx, dy, Az; loc: cc, fc, cf, ff
    expect = dict(DYU=M(1, 1), RDXU=1.0 / M(0, 1), RAZU=1.0 / M(2, 1), DXV=M(0, 2), RDYV=1.0 / M(1, 2), RAZV=1.0 / M(2, 2),
                  DYC2=M(1, 0) * M(1, 0), DXC2=M(0, 0) * M(0, 0), RAZC=1.0 / M(2, 0), DXF2=M(0, 3) * M(0, 3), DYF2=M(1, 3) * M(1, 3),
                  RAZF=1.0 / M(2, 3))
    for w, k in C2.items():
        assert np.array_equal(out[k].view(np.int64), expect[w].view(np.int64)), w
