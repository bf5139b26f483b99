"""Exact per-face restatement of the advection reconstructions (csrc/advect.hip: WENO(3 | 5 | 7) in the WENO-Z form, UpwindBiased(3 | 5),
first-order upwind, their order reduction next to walls and land), the derived error bounds of the STRICT and FAST arithmetic against
it, and a NumPy restatement of the tracer update.  CPU only; shared by tests/test_advect_ref.py and tests/test_gpu_advect_faces.py.

Arithmetic: `decimal` at 80 digits (tests/fast_math_ref.py's context).  u = 2^-53.  A stencil p[0 .. 2B-2] is upwind-most first, as the
kernel's functions take it.  The reference evaluates, on the doubles of the stencil,

    q_s = (sum_k c_sk p_k) / D            beta_s = (sum_{i<=j} b_sij p_i p_j) [/ 3 for WENO5]      tau = |sum_s t_s beta_s|
    r_s = tau / (beta_s + eps)            a_s = d_s (1 + r_s^2)           w_s = a_s / sum a           R = sum_s w_s q_s

with the constants exact (1/6, 3/10, 2.107, ...: the rationals, not their doubles; eps is the double 1e-8 both sides use).

THE COMB (how one reconstruction becomes observable through the shipped kernels)
--------------------------------------------------------------------------------
Uniform grid of spacing 1 (Ax = Ay = V = 1 exactly), v == 0, u = +-1 on the faces of one parity in i and 0 elsewhere: every cell has
exactly one live face.  With F_i = Ax u_i c~_i the kernel's G = -(rV ((F_(i+1) - F_i) + (+-0))) involves a nonzero number and zeros only,
so no operation rounds:  G = +u c~ in the cell on the high side of a live face, -u c~ on the low side (rV = rcp(1.0) = 1.0 is asserted
on the hardware).  Two parities x two sign patterns observe every face under both biases; the v comb does the same for y.

DERIVED BOUND (forward error analysis of the functions as written; constants are operation counts, NOT fitted)
--------------------------------------------------------------------------------------------------------------
Every floating-point operation contributes a relative error of at most u; a contraction (fma) only removes one, so every count below
takes the expression unfused and holds for whatever the compiler fuses.  A constant that is not a double (1/6, 1/3, 3/10, 2.107, ...)
costs 1 u more.  A reciprocal fm::rcp costs RCP_U u (fast_math_ref.py: 130 under the seed cap held on the hardware), a division 1 u.

  candidates      q_s: the products c p_k (1), B - 1 additions, the factor 1/D (constant 1 + product 1; STRICT: one division)
                  |dq_s| <= KC u sum_k |c_sk p_k|,           KC = B + 2 (FAST), B + 1 (STRICT)
  indicators      beta_s in the nested form p_i (b_ii p_i + b_ij p_j + ...) + ...: constant 1 (WENO7's decimals), inner product 1, inner
                  additions B - 1, outer product 1, outer additions B - 1, [WENO5: x 1/3: 2]
                  d_beta_s = K_BETA u sum |b_sij p_i p_j|,   K_BETA = 3 (WENO3), 8 (WENO5), 9 (WENO7), both modes
  tau             d_tau = sum_s |t_s| d_beta_s + K_TAU u sum_s |t_s| beta_s,   K_TAU = 1 (one subtraction), 4 (WENO7: 3 b, three sums)
  ratios          g = beta_s + eps carries dg = d_beta_s + u g.  Where dg >= g / 2 nothing is claimed about the weights (see the cap).
                  Else the absolute error of r_s from its inputs is  rho_s = (d_tau g + tau dg) / (g (g - dg)),
                  and its own roundings (reciprocal or division, product) are (C + 1) u relative, C = RCP_U | 1.
  weights         a_s = d_s (1 + r_s^2):  relative error E_s <= (2 r rho + rho^2) / (1 + r^2) + K_W u,
                  K_W = 2 (C + 1) + 1 (square) + 1 (1 + .) + 2 (d_s: constant, product) = 2 C + 6:  266 (FAST), 8 (STRICT).
                  To first order (2 r rho) / (1 + r^2) = (2 r^2 / (1 + r^2)) (d_beta_s / (beta_s + eps) + d_tau / tau): the issue's
                  bracket.  The rho^2 term keeps the statement true where tau is smaller than its own error.
  combination     with relative weight errors e_s, |e_s| <= E_s, and ebar = sum w_s e_s:
                  sum_s (what_s - w_s) q_s = sum_s w_s e_s (q_s - R) / (1 + ebar)   (because sum w_s (q_s - R) = 0)
                  <= 2 sum_s w_s E_s |q_s - R|  for E_s <= 1/2.  CAP: the computed weights are positive whatever their errors, so the
                  computed value is a convex combination of the computed candidates: the weight term never exceeds
                  max_s |q_s - R|.  The bound takes the smaller of the two, so it is valid (and says little) on eps-scale data.
  numerator       products a_s q_s (1), B - 1 additions: (B u) sum w_s |q_s|, folded into the candidates' term:
                  K_Q = KC + B = 2 B + 2 (FAST), 2 B + 1 (STRICT)
  normalisation   sum of the positive a_s (B - 1), reciprocal or division (C), product (FAST: 1):
                  K_R = B + C:  RCP_U + B (FAST), B + 1 (STRICT; one more than counted, slack)

      |R_computed - R| <= u [ K_R |R| + K_Q sum_s w_s sum_k |c_sk p_k| ] + min( 2 sum_s w_s E_s |q_s - R| , max_s |q_s - R| )

  UpwindBiased    (sum c_k p_k) / D:  K_LIN u sum |c_k p_k|,  K_LIN = n + 2 (n = 2B - 1 terms: product, n - 1 additions, constant, product)
  first order     the upwind value itself: exact, bound 0.
  f32 weights     beta, tau, ratios, weights and their sum are evaluated in numpy.float32 statement for statement as weno*_w32 / the
                  oracle's weno*_f32 (bit for bit: tests/test_advect_ref.py); after that a_s and the float sum S are exact inputs and
                  R = (sum a_s q_s) / S:   |error| <= u [ K_Q sum_s a_s sum_k |c_sk p_k| / S + (C + 1) |R| ].
Products of two rounding errors (u^2, at most 270^2 u^2 < 1e-27) are covered by the factor (1 + 1e-9) on every bound; the higher orders
of the weight term by its factor 2 (valid for E_s <= 1/2) and, beyond that, by the cap.
"""
from decimal import Decimal as D
from fractions import Fraction as Fr

import numpy as np

from fast_math_ref import DU, RCP_U, hp

EPS = 1e-8
B_OF = {7: 4, 5: 3, -5: 3, 3: 2, -3: 2, 1: 1}
SCHEMES = (7, 5, -5, 3, -3, 1)
SLACK = D(1) + D("1e-9")

# ---- the constants as the kernel's functions write them (stencil index: upwind-most first) ----------------------------------------
QN = {3: [[0, 1, 1], [-1, 3, 0]],
      5: [[0, 0, 2, 5, -1], [0, -1, 5, 2, 0], [2, -7, 11, 0, 0]],
      7: [[0, 0, 0, 3, 13, -5, 1], [0, 0, -1, 7, 7, -1, 0], [0, 1, -5, 13, 3, 0, 0], [-3, 13, -23, 25, 0, 0, 0]]}
QD = {3: Fr(1, 2), 5: Fr(1, 6), 7: Fr(1, 12)}
LIN = {3: [Fr(2, 3), Fr(1, 3)], 5: [Fr(3, 10), Fr(3, 5), Fr(1, 10)], 7: [Fr(4, 35), Fr(18, 35), Fr(12, 35), Fr(1, 35)]}
TAU = {3: [1, -1], 5: [1, 0, -1], 7: [1, 3, -3, -1]}
BD = {3: Fr(1), 5: Fr(1, 3), 7: Fr(1)}
UPW = {3: ([-1, 5, 2], Fr(1, 6)), 5: ([2, -13, 47, 27, -3], Fr(1, 60))}
K_BETA = {3: 3, 5: 8, 7: 9}
K_TAU = {3: 1, 5: 1, 7: 4}


def _tri(start, rows):
    """rows of the nested form p_i (c p_i + c p_(i+1) + ...) + ...: {(i, j): coefficient}, i <= j"""
    return {(start + a, start + a + b): Fr(c) for a, row in enumerate(rows) for b, c in enumerate(row)}


BETA = {
    3: [_tri(1, [["1", "-2"], ["1"]]), _tri(0, [["1", "-2"], ["1"]])],
    5: [_tri(2, [["10", "-31", "11"], ["25", "-19"], ["4"]]), _tri(1, [["4", "-13", "5"], ["13", "-13"], ["4"]]),
        _tri(0, [["4", "-19", "11"], ["25", "-31"], ["10"]])],
    7: [_tri(3, [["2.107", "-9.402", "7.042", "-1.854"], ["11.003", "-17.246", "4.642"], ["7.043", "-3.882"], ["0.547"]]),
        _tri(2, [["0.547", "-2.522", "1.922", "-0.494"], ["3.443", "-5.966", "1.602"], ["2.843", "-1.642"], ["0.267"]]),
        _tri(1, [["0.267", "-1.642", "1.602", "-0.494"], ["2.843", "-5.966", "1.922"], ["3.443", "-2.522"], ["0.547"]]),
        _tri(0, [["0.547", "-3.882", "4.642", "-1.854"], ["7.043", "-17.246", "7.042"], ["11.003", "-9.402"], ["2.107"]])],
}


def constants(scheme):
    """name -> Fraction of every constant of one reconstruction function.  WENO (scheme 3 | 5 | 7): ("q", s, k), ("qd",), ("lin", s),
    ("b", s, i, j), ("bd",), ("tau", s), ("eps",); UpwindBiased (-3 | -5): ("c", k), ("cd",)."""
    if scheme < 0:
        c, d = UPW[-scheme]
        out = {("c", k): Fr(v) for k, v in enumerate(c)}
        out[("cd",)] = d
        return out
    out = {("q", s, k): Fr(v) for s, row in enumerate(QN[scheme]) for k, v in enumerate(row) if v}
    out[("qd",)] = QD[scheme]
    out.update({("lin", s): v for s, v in enumerate(LIN[scheme])})
    out.update({("b", s, i, j): v for s, t in enumerate(BETA[scheme]) for (i, j), v in t.items()})
    out[("bd",)] = BD[scheme]
    out.update({("tau", s): Fr(v) for s, v in enumerate(TAU[scheme]) if v})
    out[("eps",)] = Fr(EPS)
    return out


def literal_constants(scheme):
    """the names of the constants that are LITERALS of the source (a coefficient +-1 is a sign, a divisor 1 is absent)"""
    return [k for k, v in constants(scheme).items() if abs(v) != 1]


def _d(fr):
    return D(fr.numerator) / D(fr.denominator)


class Tables:
    """the constants of one scheme as Decimals, optionally with some of them multiplied by a factor (pert: {name: Fraction})"""
    _cache = {}

    def __init__(self, scheme, pert=None):
        C = constants(scheme)
        for k, f in (pert or {}).items():
            C[k] = C[k] * f
        with hp():
            self.scheme = scheme
            if scheme < 0:
                self.c = [(k[1], _d(v)) for k, v in C.items() if k[0] == "c"]
                self.cd = _d(C[("cd",)])
                return
            B = B_OF[scheme]
            self.B = B
            self.q = [[(k[2], _d(v)) for k, v in C.items() if k[0] == "q" and k[1] == s] for s in range(B)]
            self.qd = _d(C[("qd",)])
            self.lin = [_d(C[("lin", s)]) for s in range(B)]
            self.b = [[(k[2], k[3], _d(v)) for k, v in C.items() if k[0] == "b" and k[1] == s] for s in range(B)]
            self.bd = _d(C[("bd",)])
            self.tau = [(k[1], _d(v)) for k, v in C.items() if k[0] == "tau"]
            self.eps = _d(C[("eps",)])

    @classmethod
    def of(cls, scheme):
        if scheme not in cls._cache:
            cls._cache[scheme] = cls(scheme)
        return cls._cache[scheme]


# ---- the exact evaluation -----------------------------------------------------------------------------------------------------------
def weno_exact(p, order, T=None):
    """One WENO-Z reconstruction on the stencil p (2B - 1 doubles) in 80-digit arithmetic.  Returns a dict: value, q, beta, tau, r, w
    (normalised weights), absq (sum_k |c_sk p_k| per candidate), absb (sum |b_sij p_i p_j| per candidate)."""
    T = T or Tables.of(order)
    with hp():
        x = [D(float(v)) for v in p]
        q, absq, beta, absb = [], [], [], []
        for s in range(T.B):
            terms = [c * x[k] for k, c in T.q[s]]
            q.append(sum(terms) * T.qd)
            absq.append(sum(abs(t) for t in terms) * abs(T.qd))
            terms = [c * x[i] * x[j] for i, j, c in T.b[s]]
            beta.append(sum(terms) * T.bd)
            absb.append(sum(abs(t) for t in terms) * abs(T.bd))
        tau = abs(sum(t * beta[s] for s, t in T.tau))
        r = [tau / (beta[s] + T.eps) for s in range(T.B)]
        a = [T.lin[s] * (1 + r[s] * r[s]) for s in range(T.B)]
        sa = sum(a)
        w = [v / sa for v in a]
        return dict(value=sum(w[s] * q[s] for s in range(T.B)), q=q, beta=beta, tau=tau, r=r, w=w, absq=absq, absb=absb, T=T)


def mode_constants(order, mode):
    B = (order + 1) // 2
    C = RCP_U if mode == "fast" else 1
    return dict(C=C, K_Q=2 * B + 2 if mode == "fast" else 2 * B + 1, K_R=B + C, K_W=2 * C + 6, K_BETA=K_BETA[order], K_TAU=K_TAU[order])


def weno_bound(e, order, mode):
    """the derived bound (module docstring) from the parts weno_exact returned; a Decimal"""
    k = mode_constants(order, mode)
    T = e["T"]
    with hp():
        R, B = e["value"], T.B
        lin = DU * (k["K_R"] * abs(R) + k["K_Q"] * sum(e["w"][s] * e["absq"][s] for s in range(B)))
        spread = max(abs(e["q"][s] - R) for s in range(B))
        dbeta = [k["K_BETA"] * DU * e["absb"][s] for s in range(B)]
        dtau = sum(abs(t) * dbeta[s] for s, t in T.tau) + k["K_TAU"] * DU * sum(abs(t) * e["beta"][s] for s, t in T.tau)
        wt = D(0)
        for s in range(B):
            g = e["beta"][s] + T.eps
            dg = dbeta[s] + DU * g
            if 2 * dg >= g:
                wt = None
                break
            rho = (dtau * g + e["tau"] * dg) / (g * (g - dg))
            r = e["r"][s]
            E = (2 * r * rho + rho * rho) / (1 + r * r) + k["K_W"] * DU
            if 2 * E > 1:
                wt = None
                break
            wt += 2 * e["w"][s] * E * abs(e["q"][s] - R)
        wt = spread if wt is None else min(wt, spread)
        return (lin + wt) * SLACK


def linear_exact(p, order, T=None):
    """UpwindBiased(order): (value, sum |c_k p_k|)"""
    T = T or Tables.of(-order)
    with hp():
        terms = [c * D(float(p[k])) for k, c in T.c]
        return sum(terms) * T.cd, sum(abs(t) for t in terms) * abs(T.cd)


def linear_bound(absterms, order):
    with hp():
        return (order + 2) * DU * absterms * SLACK


# ---- f32 weights: numpy.float32, statement for statement as weno*_w32 (advect.hip) and weno*_f32 (oracle/csi_oracle.c) ---------------
def weights_f32(p, order):
    """(a_s as float32 array, their float32 sum, beta, tau): the single-precision part of one f32-weight reconstruction"""
    F = np.float32
    f = [F(v) for v in np.asarray(p, dtype=np.float64)]
    beta = []
    with np.errstate(all="ignore"):
        for s, t in enumerate(BETA[order]):
            rows = {}
            for (i, j), c in t.items():
                rows.setdefault(i, []).append((j, c))
            acc = None
            for i in sorted(rows):
                inner = None
                for j, c in rows[i]:
                    # the float literal of the source: WENO7's decimals are float literals (2.107f); the small integers are exact
                    term = f[j] if c == 1 else F(float(c)) * f[j]
                    inner = term if inner is None else F(inner + term)
                acc = F(f[i] * inner) if acc is None else F(acc + F(f[i] * inner))
            beta.append(F(acc / F(3)) if order == 5 else acc)
        t = TAU[order]
        tau = beta[0]
        for s in range(1, len(beta)):
            if t[s]:
                term = beta[s] if abs(t[s]) == 1 else F(F(abs(t[s])) * beta[s])
                tau = F(tau + term) if t[s] > 0 else F(tau - term)
        tau = F(abs(tau))
        a = []
        for s in range(len(beta)):
            r = F(tau / F(beta[s] + F(1e-8)))
            a.append(F(F(float(LIN[order][s])) * F(F(1) + F(r * r))))
        S = a[0]
        for s in range(1, len(a)):
            S = F(S + a[s])
    return np.array(a, dtype=F), S, np.array(beta, dtype=F), tau


def weno_f32_exact(p, order, mode):
    """(value, bound) of the f32-weight reconstruction: weights and their float sum as exact inputs, the rest in Decimal"""
    a, S, _, _ = weights_f32(p, order)
    T = Tables.of(order)
    k = mode_constants(order, mode)
    with hp():
        x = [D(float(v)) for v in p]
        num, absn = D(0), D(0)
        for s in range(T.B):
            terms = [c * x[i] for i, c in T.q[s]]
            num += D(float(a[s])) * sum(terms) * T.qd
            absn += D(float(a[s])) * sum(abs(t) for t in terms) * abs(T.qd)
        R = num / D(float(S))
        return R, DU * (k["K_Q"] * absn / D(float(S)) + (k["C"] + 1) * abs(R)) * SLACK


# ---- the functions as written, in doubles (a stand-in for the kernel on the CPU) -----------------------------------------------------
class Emu:
    """A number whose every operation is evaluated at 80 digits and then multiplied by (1 + sign u): the model of the analysis above
    (the 1e-80 of the emulation itself is 64 orders below u).  `signs` is a callable returning +1 / -1 / 0 per rounding.  Use inside
    `with hp():`."""
    __slots__ = ("v", "signs")

    def __init__(self, v, signs):
        self.v, self.signs = (v if isinstance(v, D) else D(float(v))), signs

    def _r(self, v, k=1):
        return Emu(v * (1 + k * self.signs() * DU), self.signs)

    def _o(self, o):
        return o.v if isinstance(o, Emu) else D(o)

    def __add__(self, o): return self._r(self.v + self._o(o))
    def __radd__(self, o): return self._r(self._o(o) + self.v)
    def __sub__(self, o): return self._r(self.v - self._o(o))
    def __rsub__(self, o): return self._r(self._o(o) - self.v)
    def __mul__(self, o): return self._r(self.v * self._o(o))
    def __rmul__(self, o): return self._r(self._o(o) * self.v)
    def __truediv__(self, o): return self._r(self.v / self._o(o))
    def __neg__(self): return Emu(-self.v, self.signs)
    def __abs__(self): return Emu(abs(self.v), self.signs)
    def rcp(self, k): return self._r(1 / self.v, k)


_CONSTANTS = {}


def _plan(C, scheme):
    """the order of operations of a WENO function: per candidate the (k, c) of its polynomial and the rows (i, [(j, c)]) of the nested
    form of its indicator"""
    if scheme < 0:
        return None
    B = B_OF[scheme]
    qs = [[(k[2], c) for k, c in C.items() if k[0] == "q" and k[1] == s] for s in range(B)]
    bs = []
    for s in range(B):
        rows = {}
        for key, c in C.items():
            if key[0] == "b" and key[1] == s:
                rows.setdefault(key[2], []).append((key[3], c))
        bs.append(sorted(rows.items()))
    return qs, bs


def _const(fr, like):
    """a constant as the arithmetic of `like` sees it: its double (floats) or the rational with one rounding (Emu)"""
    if isinstance(like, Emu):
        exact = Fr(float(fr)) == fr
        return Emu(_d(fr), like.signs) if exact else like._r(_d(fr))
    return float(fr)


def as_written(p, scheme, mode, pert=None):
    """The kernel's function of `scheme` (3 | 5 | 7 | -3 | -5) in `mode` evaluated operation by operation, unfused, in the arithmetic of
    the stencil's elements: Python floats (IEEE doubles; STRICT's order is the oracle's) or Emu.  pert: {name: factor} on constants."""
    if pert:
        C = constants(scheme)
        for k, f in pert.items():
            C[k] = C[k] * f
        plan = _plan(C, scheme)
    else:
        if scheme not in _CONSTANTS:
            _CONSTANTS[scheme] = (constants(scheme), _plan(constants(scheme), scheme))
        C, plan = _CONSTANTS[scheme]
    x = list(p)
    one = x[0]
    fast = mode == "fast"

    def term(c, v):
        return v if c == 1 else (-v if c == -1 else _const(c, one) * v)

    def scaled(acc, d):        # STRICT divides by the integer, FAST multiplies by the reciprocal constant
        if d == 1:
            return acc
        return acc * _const(d, one) if fast else acc / _const(1 / d, one)

    if scheme < 0:
        acc = None
        for k in range(len(x)):
            t = term(C[("c", k)], x[k])
            acc = t if acc is None else acc + t
        return scaled(acc, C[("cd",)])
    B = B_OF[scheme]
    q, beta = [], []
    for s in range(B):
        acc = None
        for k, c in plan[0][s]:
            t = term(c, x[k])
            acc = t if acc is None else acc + t
        q.append(scaled(acc, C[("qd",)]))
        acc = None
        for i, row in plan[1][s]:
            inner = None
            for j, c in row:
                t = term(c, x[j])
                inner = t if inner is None else inner + t
            acc = x[i] * inner if acc is None else acc + x[i] * inner
        beta.append(scaled(acc, C[("bd",)]))
    tau = None
    for s in range(B):
        if ("tau", s) in C:
            c = C[("tau", s)]
            t = term(abs(c), beta[s])
            tau = (t if c > 0 else -t) if tau is None else (tau + t if c > 0 else tau - t)
    tau = abs(tau)
    eps = _const(C[("eps",)], one)
    a = []
    for s in range(B):
        g = beta[s] + eps
        if fast:
            r = tau * (g.rcp(RCP_U) if isinstance(g, Emu) else 1.0 / g)
        else:
            r = tau / g
        a.append(_const(C[("lin", s)], one) * (1 + r * r))
    num, den = a[0] * q[0], a[0]
    for s in range(1, B):
        num, den = num + a[s] * q[s], den + a[s]
    if fast:
        return num * (den.rcp(RCP_U) if isinstance(den, Emu) else 1.0 / den)
    return num / den


# ---- order reduction and the faces of a grid, restated ------------------------------------------------------------------------------
class Lines:
    """What the per-face reference needs of one case: sizes, halos, which sides are walls, the active mask with halos (None: no land).
    Parents are (Ny + 2 Hy, Nx + 2 Hx) arrays, element (i, j) (1-based) at [j + Hy - 1, i + Hx - 1]."""

    def __init__(self, Nx, Ny, Hx, Hy, wall_x, wall_y, active=None):
        self.Nx, self.Ny, self.Hx, self.Hy, self.wall_x, self.wall_y, self.active = Nx, Ny, Hx, Hy, wall_x, wall_y, active

    def inactive(self, i, j):
        if (self.wall_x and (i < 1 or i > self.Nx)) or (self.wall_y and (j < 1 or j > self.Ny)):
            return True
        if self.active is None:
            return False
        if i < 1 - self.Hx or i > self.Nx + self.Hx or j < 1 - self.Hy or j > self.Ny + self.Hy:
            return True
        return not self.active[j + self.Hy - 1, i + self.Hx - 1]

    def closed(self, i, j, along_y):
        """conditional_flux: a face with an inactive cell on either side carries no flux (immersed grids only)"""
        if self.active is None:
            return False
        return self.inactive(i, j) or (self.inactive(i, j - 1) if along_y else self.inactive(i - 1, j))

    def buffer_at(self, scheme, i, j, along_y, left, blunder=None):
        """B of the scheme used at face (i, j): the immersed rule on a grid with land (walls count as inactive cells), else the
        topological rule next to walls.  blunder = (i, j, along_y): that face takes the unreduced stencil (the tests' wrong decision)."""
        B = B_OF[scheme]
        if blunder is not None and blunder == (i, j, along_y):
            return B
        if self.active is not None:
            while B > 1:
                cells = [(i, j + k) if along_y else (i + k, j) for k in range(-B, B)]
                if not any(self.inactive(a, b) for a, b in cells):
                    break
                B -= 1
            return B
        wall = self.wall_y if along_y else self.wall_x
        idx, N = (j, self.Ny) if along_y else (i, self.Nx)
        while B > 1 and wall:
            if idx >= (B + 1 if left else B) and idx <= (N + 2 - B if left else N + 1 - B):
                break
            B -= 1
        return B

    def stencil(self, parent, B, i, j, along_y, left):
        """the 2B - 1 values the reconstruction at face (i, j) reads, upwind-most first"""
        jj, ii = j + self.Hy - 1, i + self.Hx - 1
        out = []
        for k in range(2 * B - 1):
            o = (k - (B - 1)) - 1 if left else -(k - (B - 1))
            out.append(float(parent[jj + o, ii]) if along_y else float(parent[jj, ii + o]))
        return tuple(out)


_MEMO = {}


def reconstruct_exact(p, scheme, B, w32=False):
    """(exact value, {mode: bound}, max |stencil|) of the function the kernel runs on stencil p for a face whose reduced buffer is B;
    memoised on the stencil, so faces shared between topologies, tracers and tests cost one evaluation."""
    key = (scheme > 0, B, bool(w32) and scheme > 0, p)
    if key not in _MEMO:
        if B == 1:
            out = (D(p[0]), dict(strict=D(0), fast=D(0)))
        elif scheme < 0:
            v, ab = linear_exact(p, 2 * B - 1)
            bd = linear_bound(ab, 2 * B - 1)
            out = (v, dict(strict=bd, fast=bd))
        elif w32:
            v, bf = weno_f32_exact(p, 2 * B - 1, "fast")
            out = (v, dict(strict=weno_f32_exact(p, 2 * B - 1, "strict")[1], fast=bf))
        else:
            e = weno_exact(p, 2 * B - 1)
            out = (e["value"], dict(strict=weno_bound(e, 2 * B - 1, "strict"), fast=weno_bound(e, 2 * B - 1, "fast")))
        _MEMO[key] = out + (max(abs(v) for v in p),)
    return _MEMO[key]


# ---- the comb -----------------------------------------------------------------------------------------------------------------------
def comb(L, along_y, parity, flip):
    """(u, v) interiors of a comb: +-1 on the faces of one parity along the comb's direction, wall faces and everything else 0.
    The sign of a face is fixed by its indices (a seeded table), `flip` negates all of them.  Returns (u, v, sign) with sign the
    (Ny, Nx) array of the value at the low (west / south) face of each cell, 0 where that face is not live."""
    nxu, nyv = L.Nx + (1 if L.wall_x else 0), L.Ny + (1 if L.wall_y else 0)
    u, v = np.zeros((L.Ny, nxu)), np.zeros((nyv, L.Nx))
    sgn = np.where(np.random.default_rng(2024).random((L.Ny + 1, L.Nx + 1)) < 0.5, -1.0, 1.0) * (-1.0 if flip else 1.0)
    f = v if along_y else u
    idx = np.arange(f.shape[0] if along_y else f.shape[1]) + 1                  # 1-based face index along the comb
    live = (idx % 2 == parity)
    if (L.wall_y if along_y else L.wall_x):
        live &= (idx > 1) & (idx < idx[-1])
    if along_y:
        f[live, :] = sgn[:nyv, :L.Nx][live, :]
    else:
        f[:, live] = sgn[:L.Ny, :nxu][:, live]
    return u, v, f[:L.Ny, :L.Nx].copy()


def faces_of(L, sign, along_y):
    """[(i, j, s)]: the live faces of a comb (1-based face indices, s = +-1 the velocity there), closed ones included"""
    jj, ii = np.nonzero(sign)
    return [(int(i) + 1, int(j) + 1, float(sign[j, i])) for j, i in zip(jj, ii)]


def observed(L, G, faces, along_y):
    """c~ at each live face read off the tendency G (Ny, Nx): s G at the cell on the high side; also returns the low-side values
    and the mask of the cells that touch no live face (their G must be 0).  The low side of face 1 in a periodic direction is cell N."""
    hi, lo = [], []
    touched = np.zeros(G.shape, dtype=bool)
    for i, j, s in faces:
        a, b = j - 1, i - 1
        la, lb = ((a - 1) % L.Ny, b) if along_y else (a, (b - 1) % L.Nx)
        hi.append(s * G[a, b])
        lo.append(-s * G[la, lb])
        touched[a, b] = touched[la, lb] = True
    return np.array(hi), np.array(lo), ~touched


def reference_faces(L, parent, scheme, faces, along_y, w32=False, blunder=None):
    """exact value, bounds and stencil scale of every face of `faces` (closed faces: 0, bound 0)"""
    val, bnd, scale = [], dict(strict=[], fast=[]), []
    for i, j, s in faces:
        if L.closed(i, j, along_y):
            v, b, m = D(0), dict(strict=D(0), fast=D(0)), 0.0
        else:
            left = s > 0
            B = L.buffer_at(scheme, i, j, along_y, left, blunder)
            v, b, m = reconstruct_exact(L.stencil(parent, B, i, j, along_y, left), scheme, B, w32)
        val.append(v); scale.append(m)
        for k in bnd:
            bnd[k].append(b[k])
    return val, bnd, scale


# ---- input families ----------------------------------------------------------------------------------------------------------------
FAMILIES = ("rand", "smooth", "step", "const", "spike", "big", "tiny", "mixed", "eps_rand", "eps_kink", "zero", "step2")
ILL = ("eps_rand", "eps_kink")            # the two eps-scale families: the bound is printed, not capped


def family_line(kind, n, rng):
    x = np.arange(n)
    if kind == "rand":
        return 0.3 + 0.2 * rng.random(n)
    if kind == "smooth":
        return 0.3 + 0.005 * np.sin(2 * np.pi * (x + rng.random()) / 40.0)          # 40 cells per wave: resolved
    if kind in ("step", "step2"):       # open water | ice, runs of 1 .. 8 cells: a step at every offset of every stencil
        out, k, ice = np.zeros(n), 0, kind == "step2"
        while k < n:
            run = int(rng.integers(1, 9))
            if ice:
                out[k:k + run] = 0.3 + 0.1 * rng.random(min(run, n - k))
            k, ice = k + run, not ice
        return out
    if kind == "const":
        return np.full(n, float(rng.choice([0.3, 1.0, 0.7, 1e6 / 3])))
    if kind == "spike":
        out = np.zeros(n)
        out[rng.integers(0, n, max(1, n // 12))] = 1.0 + rng.random(max(1, n // 12))
        return out
    if kind == "big":
        return 1e6 * rng.random(n)
    if kind == "tiny":
        return 1e-9 * rng.random(n)
    if kind == "mixed":
        return rng.uniform(-1.0, 1.0, n)
    if kind == "eps_rand":
        return 0.3 + 1e-4 * rng.random(n)
    if kind == "eps_kink":
        return 0.3 + 1e-4 * np.abs(((x + int(rng.integers(0, 5))) % 10) - 5.0)
    if kind == "zero":
        return np.zeros(n)
    raise KeyError(kind)


F32_FAMILIES = ("rand", "smooth", "step", "const", "spike", "kilo", "f32tiny", "mixed", "eps_rand", "eps_kink", "zero", "step2")


def family_line_f32(kind, n, rng):
    """the f32-weight inputs: |c| <= 1e3 plus the 1e-30 family, whose float squares underflow"""
    if kind == "kilo":
        return 1e3 * rng.random(n)
    if kind == "f32tiny":
        return 1e-30 * rng.random(n)
    if kind == "const":
        return np.full(n, float(rng.choice([0.3, 1.0, 0.7, 1e3 / 3])))
    return family_line(kind, n, rng)


def family_fields(Nx, Ny, seed, f32=False):
    """(FX, FY, rows, cols): FX's rows and FY's columns hold one family each (the u comb reads along rows, the v comb along columns);
    rows[j] / cols[i] name them."""
    rng = np.random.default_rng(seed)
    names = F32_FAMILIES if f32 else FAMILIES
    gen = family_line_f32 if f32 else family_line
    rows = [names[j % len(names)] for j in range(Ny)]
    cols = [names[i % len(names)] for i in range(Nx)]
    FX = np.stack([gen(k, Nx, rng) for k in rows], axis=0)
    FY = np.stack([gen(k, Ny, rng) for k in cols], axis=1)
    return FX, FY, rows, cols


# ---- the tracer update: _dynamic_step_tracers! / dynamic_step_snow!, sea_ice_fe_step.jl:56-94, in NumPy doubles ----------------------
def jmax0(x):
    """Julia's max(0, x): NaN if x is NaN, +0.0 for -0.0 (max(0.0, -0.0) is 0.0)"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x + 0.0, np.where(0.0 < x, x, 0.0))


BRANCHES = ("h+ < 0", "a+ < 0", "h+ == 0, a+ > 0", "a+ == 0, h+ > 0", "a+ > 1", "plain", "-0.0", "NaN", "+-Inf", "snow over a <= 0")


def tracer_update(hn, an, Gh, Ga, dt, sn=None, Ghs=None):
    """(h, a[, hs], taken): the statements of the reference in their order on arrays of doubles; taken[name] marks the cells of each
    branch of BRANCHES."""
    with np.errstate(all="ignore"):
        hp_, ap_ = hn + dt * Gh, an + dt * Ga
        taken = {"h+ < 0": hp_ < 0, "a+ < 0": ap_ < 0, "-0.0": ((hp_ == 0) & np.signbit(hp_)) | ((ap_ == 0) & np.signbit(ap_)),
                 "NaN": np.isnan(hp_) | np.isnan(ap_), "+-Inf": np.isinf(hp_) | np.isinf(ap_)}
        ap = jmax0(ap_)
        hp = jmax0(hp_)
        taken["h+ == 0, a+ > 0"] = (hp == 0) & (ap > 0)
        ap = np.where(hp == 0, 0.0, ap)
        taken["a+ == 0, h+ > 0"] = (ap == 0) & (hp > 0)
        hp = np.where(ap == 0, 0.0, hp)
        Vp = hp * ap
        taken["a+ > 1"] = ap > 1
        taken["plain"] = (ap > 0) & (ap <= 1) & (hp > 0) & np.isfinite(hp)
        a1 = np.where(ap > 1, 1.0, ap)
        h1 = np.where(ap > 1, Vp, hp)
        if sn is None:
            return h1, a1, taken
        sp = jmax0(sn + dt * Ghs)
        taken["snow over a <= 0"] = (a1 <= 0) & (sp > 0)
        return h1, a1, np.where(a1 <= 0, 0.0, sp), taken


def same_bits(a, b):
    """bit for bit, signs of zero included; a NaN matches any NaN (its class: the sign and payload of a generated NaN are the
    hardware's choice -- 0 x inf is the negative default NaN on x86 and the positive one on the GPU)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])
