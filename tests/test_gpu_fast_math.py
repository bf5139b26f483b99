"""The FAST-mode arithmetic (csrc/evp_fast_math.h), function by function, on the GPU.

tests/fast_math_probe.hip (built by csrc/Makefile's `probe` target with evp_fast.o's flags) runs every function element-wise; here
  (a) the primitives are held to bounds that follow from ONE refinement step on the measured hardware seed,
  (b) the "same bits" claims of the header are compared as bit patterns,
  (c) the composite functions are compared element by element with the high-precision restatement of the REFERENCE
      (tests/fast_math_ref.py) under condition-scaled bounds whose constants come from forward error analysis (derived there),
      and each bound is shown to be tight enough to see a constant that is off by 2^-40.
Every figure a bound is compared with is printed before the assertion (pytest -s); profiles/r20_fast_math_probe.md keeps them.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import evp_parameter_sets as ps
import fast_math_build
import fast_math_ref as R
from fast_math_ref import D, U

pytestmark = pytest.mark.gpu

DBL_MIN = R.DBL_MIN
I64 = np.int64


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(fast_math_build.PROBE):
        raise RuntimeError(f"{fast_math_build.PROBE} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(fast_math_build.PROBE)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_long
    pd = C.POINTER(C.c_double)
    L.fmp_primitives.argtypes = [vp, vp, i64, vp]
    L.fmp_stress.argtypes = [i32, pd, vp, vp, i64, vp]
    L.fmp_ext_stress.argtypes = [i32, vp, vp, i64, vp]
    L.fmp_vel.argtypes = [i32, pd, vp, vp, i64, vp]
    L.fmp_avg.argtypes = [vp, vp, i64, vp]
    L.fmp_full.argtypes = [vp, vp, i64, vp]
    return L


def launch(fn, head, rows, nout):
    """rows: (k, n) float64 inputs -> (nout, n) float64 outputs of one launch of probe entry point fn(*head, in, out, n, stream)"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim == 1:
        rows = rows[None, :]
    n = rows.shape[1]
    x = torch.from_numpy(rows).to("cuda:0")
    out = torch.full((nout, n), float("nan"), dtype=torch.float64, device="cuda:0")
    rc = fn(*head, x.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"launch failed: hipError_t {rc}"
    torch.cuda.synchronize()
    return out.cpu().numpy()


def primitives(probe, x):
    """rows: rcp seed, rsq seed, rcp, rsqrt, sqrt_fast, s, rs"""
    return launch(probe.fmp_primitives, (), x, 7)


def cvec(*v):
    return (C.c_double * len(v))(*[float(a) for a in v])


def stress_consts(k):
    return cvec(k["em2"], k["Dmin"], k["amin"], k["amax"], k["hk1"], k["pressure_kind"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(I64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def first_difference(a, b):
    d = np.nonzero(bits(a) != bits(b))[-1]
    return None if d.size == 0 else int(d[0])


# ---- input domains (the issue's) -------------------------------------------------------------------------------------------------------

def logmag(rng, n, lo, hi, zero=0.1, signed=True):
    v = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)
    if signed:
        v *= rng.choice([-1.0, 1.0], n)
    v[rng.random(n) < zero] = 0.0
    return v


def masses(rng, n):
    """0, subnormal, or 1e-300 .. 1e6 (most of them where ice is: 1e-3 .. 1e4)"""
    m = np.where(rng.random(n) < 0.7, 10.0 ** rng.uniform(-3, 4, n), 10.0 ** rng.uniform(-300, 6, n))
    r = rng.random(n)
    m[r < 0.10] = 0.0
    m[(r >= 0.10) & (r < 0.14)] = rng.integers(1, 2 ** 40, n)[(r >= 0.10) & (r < 0.14)] * 5e-324
    return m


STRESS_ROWS = ["e11c", "e22c", "e12f", "e11f", "e22f", "e12c", "Pc", "Pf", "mc", "mf", "rmc", "rmf", "hkc", "hkf", "s11", "s22", "s12"]


def stress_inputs(probe, n, seed, gamma_targets=0.3, own_set_apart=False, consts=None):
    """(17, n) rows in stress_update_r's argument order; rmc, rmf from fm::rcp itself.  Every row is drawn independently of the others
    (P = 0 under an ordinary mass, P > 0 over no mass, ...).  A fraction of the elements gets an hkc / hkf that puts gamma between the
    clamps (elsewhere the broad magnitudes leave it on a plateau almost always).
    own_set_apart: the comparison with the REFERENCE leaves one combination to a test of its own
    (test_subnormal_mass_under_zero_ice_strength): P == 0 under a SUBNORMAL mass, where evp_fast_math.h documents alpha+ against the
    reference's alpha-.  Exactly those elements get the smallest normal mass instead; nothing else is touched.
    consts: the stress constants of a non-default parameter set (fast_math_ref.stress_constants); the targeted gammas then lie between
    that set's clamps, 4 % of their distance inside, as 60 .. 290 do between the default 50 and 300."""
    rng = np.random.default_rng(seed)
    a = {k: logmag(rng, n, 1e-30, 1e3) for k in STRESS_ROWS[:6]}
    small = rng.random(n) < 0.5                                  # half of the cells at geophysical rates (1e-10 .. 1e-4 s^-1)
    for k in STRESS_ROWS[:6]:
        a[k] = np.where(small, logmag(rng, n, 1e-10, 1e-4), a[k])
    a["Pc"], a["Pf"] = logmag(rng, n, 1e-10, 1e9, signed=False), logmag(rng, n, 1e-10, 1e9, signed=False)
    a["mc"], a["mf"] = masses(rng, n), masses(rng, n)
    a["hkc"], a["hkf"] = 10.0 ** rng.uniform(-8, 2, n), 10.0 ** rng.uniform(-8, 2, n)
    for k in ("s11", "s22", "s12"):
        a[k] = logmag(rng, n, 1e-10, 1e9)
    if own_set_apart:
        for P, m in (("Pc", "mc"), ("Pf", "mf")):
            a[m][(a[P] == 0) & (a[m] > 0) & (a[m] < DBL_MIN)] = DBL_MIN
    k0 = R.stress_constants() if consts is None else consts
    inside = 0.04 * (k0["amax"] - k0["amin"])
    g_lo, g_hi = (60.0, 290.0) if consts is None else (k0["amin"] + inside, k0["amax"] - inside)
    t = rng.random(n) < gamma_targets
    for (P, m, hk, e1, e2, e12, other) in (("Pc", "mc", "hkc", "e11c", "e22c", "e12c", None), ("Pf", "mf", "hkf", "e11f", "e22f", "e12f", None)):
        delta = np.maximum(np.sqrt((a[e1] + a[e2]) ** 2 + ((a[e1] - a[e2]) ** 2 + 4 * a[e12] ** 2) * k0["em2"]), k0["Dmin"])
        ok = t & (a[P] > 0) & (a[m] > 1e-3)
        g = rng.uniform(g_lo, g_hi, n)
        a[hk] = np.where(ok, g * g * delta * a[m] / np.where(ok, a[P], 1.0), a[hk])
    rows = np.stack([a.get(k, np.zeros(n)) for k in STRESS_ROWS])
    rows[10], rows[11] = primitives(probe, rows[8])[2], primitives(probe, rows[9])[2]
    return rows


def scaled_for_sums(probe, rows):
    """the inputs of stress_update_s from those of stress_update_r: exact multiplications by powers of two, rM4 = fm::rcp(M4)"""
    s = rows.copy()
    s[2] = 8.0 * rows[2]                      # E12f = 8 e12f
    s[3], s[4] = 4.0 * rows[3], 4.0 * rows[4]     # S11f, S22f
    s[5] = 2.0 * rows[5]                      # y2 = 2 e12c
    s[7] = 4.0 * rows[7]                      # XP
    s[9] = 4.0 * rows[9]                      # M4
    s[11] = primitives(probe, s[9])[2]        # rM4
    s[13] = 4.0 * rows[13]                    # hkf4
    return s


VEL_ROWS = ["w", "wn", "m_a", "m_b", "a_a", "a_b", "al_a", "al_b", "div", "cor", "ext", "imt", "exb", "imb", "peripheral", "wf"]
VK = dict(dt=120.0, min_mass=1.0, min_conc=1e-3)


def vel_consts(k, scale=1.0):
    return cvec(scale * k["dt"], 1.0 / k["dt"], scale * k["min_mass"], scale * k["min_conc"])


def vel_inputs(n, seed, ordered_drag=False):
    rng = np.random.default_rng(seed)
    a = dict(w=logmag(rng, n, 1e-12, 1e2), wn=logmag(rng, n, 1e-12, 1e2), m_a=masses(rng, n), m_b=masses(rng, n),
             a_a=rng.random(n), a_b=rng.random(n), al_a=rng.uniform(50.0, 300.0, n), al_b=rng.uniform(50.0, 300.0, n),
             div=logmag(rng, n, 1e-10, 1e6), cor=logmag(rng, n, 1e-12, 1e-2), ext=logmag(rng, n, 1e-6, 10.0), imt=logmag(rng, n, 1e-8, 1e2, 0.5, False),
             exb=logmag(rng, n, 1e-6, 10.0), imb=logmag(rng, n, 1e-8, 1e2, 0.1, False), peripheral=(rng.random(n) < 0.05).astype(np.float64),
             wf=logmag(rng, n, 1e-6, 1.0, 0.0))
    for k in ("a_a", "a_b"):
        r = rng.random(n)
        a[k][r < 0.1] = 0.0
        a[k][r > 0.9] = 1.0
        a[k][(r > 0.1) & (r < 0.2)] *= 1e-3
    for k in ("al_a", "al_b"):
        r = rng.random(n)
        a[k][r < 0.3] = 300.0
        a[k][r > 0.9] = 50.0
    if ordered_drag:
        a["imb"] = np.maximum(a["imb"], a["imt"])            # the denominator's terms have one sign: fast_math_ref.py, K_VEL
    return np.stack([a[k] for k in VEL_ROWS])


# ---- (a) primitives ------------------------------------------------------------------------------------------------------------------

def ulps_apart(a, b):
    return np.abs(bits(a) - bits(b))


def test_primitives_one_refinement_step_on_the_hardware_seed(probe):
    """rcp, rsqrt, sqrt_fast, sqrt_rsqrt over 512 log-uniform mantissas in every binade of [2^-1000, 2^1000), the powers of two, 1 -+ 1 ulp and
    the smallest normal number (the floor of ext_stress): 1 026 005 elements, one launch.

    Per element the seed error e = |seed x - 1| (rcp), |seed sqrt(x) - 1| (rsq) is MEASURED (x87 long double: 64-bit mantissa, correctly
    rounded 1 / x and sqrt; the residual of a product near 1 is then good to 2^-63) and the refined result is held to
        rcp: e^2 + 2 u        rsqrt, sqrt_fast: 1.5 e^2 + 2 u        (+ 2^-62 for the long double evaluation of the residual itself)
    which is what one Newton / Goldschmidt step with correctly rounded fmas gives (derived and emulated exactly in
    tests/test_fast_math_ref.py).  Every seed error is capped at 2^-23, so every refined result is within 194 u = 2.2e-14."""
    LD = np.longdouble
    assert np.finfo(LD).nmant >= 63
    rng = np.random.default_rng(1)
    ex = np.arange(-1000, 1000)
    x = np.concatenate([np.ldexp(1.0 + rng.random((ex.size, 512)), ex[:, None]).ravel(), np.ldexp(1.0, np.arange(-1000, 1001)),
                        [np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), DBL_MIN]])
    assert x.size <= 2 ** 20
    seed_r, seed_q, rc, rq, sq, s, rs = primitives(probe, x)
    xl = x.astype(LD)
    sx = np.sqrt(xl)
    e_r, e_q = np.abs(seed_r.astype(LD) * xl - 1), np.abs(seed_q.astype(LD) * sx - 1)
    print(f"seed error: v_rcp_f64 max {float(e_r.max()):.3e} = 2^{np.log2(float(e_r.max())):.2f}, v_rsq_f64 max {float(e_q.max()):.3e} "
          f"= 2^{np.log2(float(e_q.max())):.2f}")
    assert float(e_r.max()) <= R.SEED_CAP and float(e_q.max()) <= R.SEED_CAP
    u, slack = LD(U), LD(2.0) ** -62
    for name, err, bound in (("rcp", np.abs(rc.astype(LD) * xl - 1), e_r * e_r + 2 * u + slack),
                             ("rsqrt", np.abs(rq.astype(LD) * sx - 1), LD(1.5) * e_q * e_q + 2 * u + slack),
                             ("sqrt_fast", np.abs(sq.astype(LD) / sx - 1), LD(1.5) * e_q * e_q + 2 * u + slack)):
        q = err / bound
        k = int(np.argmax(q))
        exact = {"rcp": 1.0 / x, "rsqrt": (1 / sx).astype(np.float64), "sqrt_fast": np.sqrt(x)}[name]
        got = {"rcp": rc, "rsqrt": rq, "sqrt_fast": sq}[name]
        ul = ulps_apart(got, exact)
        print(f"{name}: worst error / bound {float(q[k]):.3f} at x = {x[k]!r}; max relative error {float(err.max()):.3e}; "
              f"max {int(ul.max())} ulp / mean {float(ul.mean()):.2f} ulp from the correctly rounded value")
        assert float(q[k]) <= 1.0, (name, x[k], float(err[k]), float(bound[k]))
    # sqrt_rsqrt: rs is rsqrt(x) bit for bit; s within 1 ulp of the correctly rounded root
    assert same_bits(rs, rq)
    off = ulps_apart(s, np.sqrt(x))
    print(f"sqrt_rsqrt s: {int((off != 0).sum())} of {x.size} elements are not the correctly rounded root (max {int(off.max())} ulp away)")
    assert int(off.max()) <= 1


def test_sqrt_rsqrt_returns_the_plateau_values_exactly(probe):
    """x = alpha^2 for every alpha = k / 4, 4 <= k <= 4000, the defaults 50 and 300 and 20 000 random alpha of at most 26 significant bits
    (alpha^2 is exact): s must be alpha bit for bit, or a user's alpha+- would not be the number the reference stores in the field."""
    rng = np.random.default_rng(2)
    alpha = np.concatenate([np.arange(4, 4001) / 4.0, [50.0, 300.0],
                            np.ldexp(rng.integers(2 ** 25, 2 ** 26, 20000).astype(np.float64), rng.integers(-26, -15, 20000))])
    x = alpha * alpha
    assert all(float(a) ** 2 == float(v) for a, v in zip(alpha[::97], x[::97]))
    s = primitives(probe, x)[5]
    bad = np.nonzero(bits(s) != bits(alpha))[0]
    print(f"plateau set: {bad.size} of {alpha.size} roots differ from alpha" + (f", first alpha = {alpha[bad[0]]!r} -> {s[bad[0]]!r}" if bad.size else ""))
    assert bad.size == 0
    assert same_bits(s, np.sqrt(x))


# ---- (b) the same bits ---------------------------------------------------------------------------------------------------------------

OUT8 = ["s11", "s22", "s12", "alpha", "zc2", "zf2", "xc", "rDc"]


@pytest.mark.parametrize("pressure_kind", [0, 1])
def test_stress_update_forms_give_the_same_bits(probe, pressure_kind):
    """stress_update_s (sums, scaled by powers of two) and stress_update (rcp inside) against stress_update_r: all eight outputs, ice-free
    cells and corners (m = 0: rcp(0), 0 * inf) and subnormal masses included; no output may be NaN (the selects absorb them)."""
    n = 1 << 16
    k = R.stress_constants(pressure_kind=pressure_kind)
    rows = stress_inputs(probe, n, seed=20 + pressure_kind)
    assert (rows[8] == 0).sum() > 1000 and (rows[9] == 0).sum() > 1000
    sub = lambda m: (m > 0) & (m < DBL_MIN)
    assert ((rows[6] == 0) & (rows[8] >= DBL_MIN)).sum() > 1000 and ((rows[7] == 0) & sub(rows[9])).sum() > 100    # P = 0: under ice, under subnormal mass
    r = launch(probe.fmp_stress, (0, stress_consts(k)), rows, 8)
    s = launch(probe.fmp_stress, (1, stress_consts(k)), scaled_for_sums(probe, rows), 8)
    p = launch(probe.fmp_stress, (2, stress_consts(k)), rows, 8)
    assert np.isfinite(r).all()
    for q, name in enumerate(OUT8):
        assert same_bits(r[q], s[q]), ("stress_update_s", name, first_difference(r[q], s[q]))
        assert same_bits(r[q], p[q]), ("stress_update", name, first_difference(r[q], p[q]))
    # ice-free cells / corners keep their stresses bit for bit
    free_c, free_f = rows[8] <= 0, rows[9] <= 0
    assert same_bits(r[0][free_c], rows[14][free_c]) and same_bits(r[1][free_c], rows[15][free_c]) and same_bits(r[2][free_f], rows[16][free_f])


def test_velocity_update_forms_give_the_same_bits(probe):
    n = 1 << 16
    rows = vel_inputs(n, seed=30)
    avg = rows.copy()
    for q in (2, 4, 6):
        avg[q] = 0.5 * (rows[q] + rows[q + 1])
    summed = rows.copy()
    for q in (2, 4, 6):
        summed[q] = rows[q] + rows[q + 1]
    summed[8] = 2.0 * rows[8]
    k, k2 = vel_consts(VK), vel_consts(VK, 2.0)
    ref, ref_fd = launch(probe.fmp_vel, (0, k), avg, 1)[0], launch(probe.fmp_vel, (1, k), avg, 1)[0]
    assert np.isfinite(ref).all() and np.isfinite(ref_fd).all()
    assert (ref != 0).sum() > n // 4
    for which, consts, inp, want, name in ((2, k2, summed, ref, "vel_update_sum"), (3, k2, summed, ref_fd, "vel_update_sum_fd"),
                                           (4, k, rows, ref, "vel_update"), (5, k, rows, ref_fd, "vel_update_fd")):
        got = launch(probe.fmp_vel, (which, consts), inp, 1)[0]
        assert same_bits(got, want), (name, first_difference(got, want))


def test_small_forms_give_the_same_bits(probe):
    """avg4 / quarter against the nested halvings; ext_stress_rest against ext_stress(3, we = webar = 0) with w = -0.0 and w = wbar = 0;
    full_strain_corner8, full_div1_x2, full_div2_x2 against 8 x / 2 x their plain forms."""
    rng = np.random.default_rng(40)
    n = 1 << 16
    a = np.stack([logmag(rng, n, 1e-30, 1e3) for _ in range(4)])
    o = launch(probe.fmp_avg, (), a, 3)
    nested = 0.5 * (0.5 * (a[0] + a[1]) + 0.5 * (a[2] + a[3]))
    assert same_bits(o[2], nested) and same_bits(o[0], nested) and same_bits(o[1], nested)

    e = np.zeros((6, n))
    e[1] = 1026.0 * 5.5e-3
    e[4], e[5] = logmag(rng, n, 1e-12, 1e2), logmag(rng, n, 1e-12, 1e2)
    e[4][:4], e[5][:4] = [-0.0, 0.0, -0.0, 0.0], [0.0, 0.0, -0.0, 1.0]
    o = launch(probe.fmp_ext_stress, (3,), e, 4)
    assert np.isfinite(o).all()
    assert same_bits(o[0], o[2]) and same_bits(o[1], o[3])
    assert (bits(o[2]) == 0).all()                                 # ex = +0

    p = np.stack([logmag(rng, n, 1e-6, 1e6, 0.05) for q in range(10)])
    o = launch(probe.fmp_full, (), p, 6)
    assert np.isfinite(o).all()
    assert same_bits(o[1], 8.0 * o[0]) and same_bits(o[3], 2.0 * o[2]) and same_bits(o[5], 2.0 * o[4])


def test_report_where_the_scaled_stress_form_first_differs(probe):
    """Not a bound but a measurement (profiles/r20_fast_math_probe.md, and the comment of stress_update_s): strain rates and Delta_min are
    scaled down by powers of two until stress_update_s and stress_update_r first differ in any output bit.  Asserted: they agree as long
    as every squared strain rate stays a normal number (|strain rate| >= 2^-500 here)."""
    n = 4096
    base = stress_inputs(probe, n, seed=50, gamma_targets=0.0)
    rng = np.random.default_rng(51)
    for q in range(6):
        base[q] = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n)      # magnitudes in [1, 2): the scale below is the magnitude
    first = None
    for e in range(0, -1080, -4):
        sc = np.ldexp(1.0, e)
        rows = base.copy()
        rows[:6] *= sc
        k = R.stress_constants(Dmin=sc)
        r = launch(probe.fmp_stress, (0, stress_consts(k)), rows, 8)
        s = launch(probe.fmp_stress, (1, stress_consts(k)), scaled_for_sums(probe, rows), 8)
        if not same_bits(r, s):
            first = e
            break
    print(f"stress_update_s == stress_update_r bit for bit down to strain rates and Delta_min of 2^{(first + 4) if first is not None else -1076}; "
          f"first difference at 2^{first}")
    assert first is None or first < -500


# ---- (c) composite functions against the reference -----------------------------------------------------------------------------------

def ratios(got, ref, bound, K):
    with R.hp():
        return R.worst_ratio(got, ref, [K * b for b in bound])


# the parameter sets of tests/evp_parameter_sets.py as fast_math_ref.stress_constants keywords: e = 1.7 and 2.7 (e^-2 and (1 - e^-2) / 2 are
# not exact there, as they are at the default e = 2), clamps 6 / 11 and 4 / 9, Delta_min 8e-6 and 1.3e-5
PARAMETER_SETS = {name: dict(ecc=s["ecc"], Dmin=s["delta_min"], amin=s["alpha_min"], amax=s["alpha_max"]) for name, s in (("A", ps.SET_A), ("B", ps.SET_B))}


@pytest.mark.parametrize("pressure_kind", [0, 1])
def test_stress_update_against_the_reference(probe, pressure_kind):
    stress_update_against_the_reference(probe, pressure_kind)


@pytest.mark.parametrize("pressure_kind", [0, 1])
@pytest.mark.parametrize("name", sorted(PARAMETER_SETS))
def test_stress_update_against_the_reference_on_parameter_sets(probe, name, pressure_kind):
    """The same comparison, under the same derived bounds, with the constants of the non-default parameter sets: 3000 elements each, the
    targeted gammas between that set's clamps, the plateaus at that set's alpha-, alpha+."""
    stress_update_against_the_reference(probe, pressure_kind, consts=PARAMETER_SETS[name], n=3000, seed=160 + 2 * sorted(PARAMETER_SETS).index(name))


def stress_update_against_the_reference(probe, pressure_kind, consts=None, n=10000, seed=60):
    """stress_update_r, 10 000 elements of the domain per pressure kind, against fast_math_ref.stress_cell under
        |sigma - ref| <= K_SIGMA u (|sigma| + (|2 eta eps| + |(zeta - eta) div| + |P_r / 2| + |sigma|) / gamma),   |alpha - ref| <= K_ALPHA u alpha
    (K_SIGMA = 594, K_ALPHA = 168: derived in fast_math_ref.py, never fitted).  Where the exact gamma^2 lies beyond a clamp by more than
    its own error bound alpha must be alpha+- exactly; ice-free cells / corners keep sigma bit for bit.
    Power: the reference evaluated once more with e^-2, hk1 or hkc off by 2^-40 must violate a bound somewhere."""
    k = R.stress_constants(pressure_kind=pressure_kind, **(consts or {}))
    amin, amax = k["amin"], k["amax"]
    rows = stress_inputs(probe, n, seed=seed + pressure_kind, own_set_apart=True, consts=None if consts is None else k)
    assert ((rows[6] == 0) & (rows[8] >= DBL_MIN)).sum() > n // 100 and ((rows[7] == 0) & (rows[9] >= DBL_MIN)).sum() > n // 100   # P = 0 under ice
    out = launch(probe.fmp_stress, (0, stress_consts(k)), rows, 8)
    assert np.isfinite(out).all()
    args = lambda i: [rows[q][i] for q in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 16)]

    def evaluate(idx, **pert):
        ref = {name: [] for name in ("s11", "s22", "s12", "alpha")}
        bnd = {name: [] for name in ("s11", "s22", "s12", "alpha")}
        with R.hp():
            for i in idx:
                r = R.stress_cell(k, *args(i), **pert)
                for q, name, Nq, g in ((0, "s11", r[4], r[7]), (1, "s22", r[5], r[7]), (2, "s12", r[6], r[8])):
                    ref[name].append(r[q])
                    bnd[name].append(R.stress_bound(rows[14 + q][i], Nq, g))
                ref["alpha"].append(r[3])
                bnd["alpha"].append(R.DU * r[3])
        return ref, bnd
    idx = range(n)
    ref, bnd = evaluate(idx)
    KK = dict(s11=R.K_SIGMA, s22=R.K_SIGMA, s12=R.K_SIGMA, alpha=R.K_ALPHA)
    col = dict(s11=0, s22=1, s12=2, alpha=3)
    worst = {name: ratios(out[col[name]], ref[name], bnd[name], KK[name]) for name in KK}
    between = sum(1 for a in ref["alpha"] if amin < a < amax)
    print(f"stress_update_r, pressure kind {pressure_kind}: worst error / bound " + ", ".join(f"{name} {worst[name][0]:.4f}" for name in KK)
          + f" ({between} of {n} cells with alpha between the clamps)")
    assert between > n // 10
    for name in KK:
        assert worst[name][0] <= 1.0, (name, worst[name], [rows[q][worst[name][1]] for q in range(17)])
    # plateaus: alpha exactly alpha+- wherever the exact gamma^2 is beyond the clamp by more than the error bound of the computed one
    margin = float((R.RSQ_U + R.RCP_U + 5.5) * 2 * U)
    on_plateau = 0
    with R.hp():
        for i in idx:
            zc = D(float(out[4][i])) / 2
            if rows[8][i] > 0:
                g2 = float(zc * 2 * D(float(rows[12][i])) / D(float(rows[8][i])) / D(amax ** 2)) if zc > 0 else 0.0
                if g2 > 1 + margin:
                    assert out[3][i] == amax, i
                    on_plateau += 1
                elif g2 < (amin / amax) ** 2 * (1 - margin):
                    assert out[3][i] == amin, i
                    on_plateau += 1
            else:
                assert out[3][i] == amax, i
    assert on_plateau > n // 10
    free_c, free_f = rows[8] <= 0, rows[9] <= 0
    assert free_c.sum() > n // 100 and free_f.sum() > n // 100
    assert same_bits(out[0][free_c], rows[14][free_c]) and same_bits(out[1][free_c], rows[15][free_c]) and same_bits(out[2][free_f], rows[16][free_f])
    # power of the test
    sub = range(min(2500, n))
    with R.hp():
        eps = 1 + D(2) ** -40
        perturbed = dict(em2=dict(em2=D(k["em2"]) * eps), hk1=dict(hk1=(1 - D(k["em2"])) / 2 * eps), hkc=dict(hkc_scale=eps))
    for what, pert in perturbed.items():
        pref, pbnd = evaluate(sub, **pert)
        w = max(ratios(out[col[name]][:len(sub)], pref[name], pbnd[name], KK[name])[0] for name in KK)
        print(f"  reference with {what} off by 2^-40: worst error / bound {w:.2f}")
        assert w > 1.0, what


@pytest.mark.parametrize("pressure_kind", [0, 1])
def test_stress_update_at_the_decisions(probe, pressure_kind):
    """Delta at, just below and just above Delta_min; gamma^2 at and one ulp around alpha-^2 and alpha+^2.  Delta_min = 2^-29 and
    hkc = 2^-30 with m = 1 and no strain make the exact gamma^2 = P / 2, so P = 2 alpha^2 (1 -+ ulp) puts it where it is wanted; the same
    bounds as everywhere (the clamps are continuous), and alpha is alpha+- exactly on the plateau side.  Both pressure kinds: at
    Delta ~ Delta_min the replacement pressure P / (1 + Delta_min / Delta) is half the ice strength."""
    Dmin = 2.0 ** -29
    k = R.stress_constants(Dmin=Dmin, pressure_kind=pressure_kind)
    up, dn = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    cells = []
    for half in (dn(Dmin / 2), Dmin / 2, up(Dmin / 2), 0.0):                       # e11 = e22 = half: Delta = 2 half against Delta_min
        for P in (27500.0, 1e-3):
            cells.append(dict(e11c=half, e22c=half, e11f=half, e22f=half, Pc=P, Pf=P, mc=270.0, mf=270.0, hkc=1.5e-4, hkf=1.5e-4, s11=-3.0, s22=2.0, s12=0.5))
    expect_alpha = {}
    for a in (50.0, 300.0):
        for f in (1 - 1e-12, 1.0, 1 + 1e-12):
            for P in (dn(2 * a * a * f), 2 * a * a * f, up(2 * a * a * f)):
                # 1e-12 is beyond the knee by more than the error bound of the computed gamma^2 ((R + C + 5.5) u = 3.7e-14): there alpha is
                # alpha+- exactly; at the knee itself and one ulp around it the bound holds and alpha stays inside [alpha-, alpha+]
                expect_alpha[len(cells)] = a if ((a == 300.0 and f > 1) or (a == 50.0 and f < 1)) else None
                cells.append(dict(Pc=P, Pf=P, mc=1.0, mf=1.0, hkc=2.0 ** -30, hkf=2.0 ** -30, s11=10.0, s22=-20.0, s12=5.0))
    n = len(cells)
    rows = np.zeros((17, n))
    for i, c in enumerate(cells):
        for name, v in c.items():
            rows[STRESS_ROWS.index(name)][i] = v
    rows[10], rows[11] = primitives(probe, rows[8])[2], primitives(probe, rows[9])[2]
    out = launch(probe.fmp_stress, (0, stress_consts(k)), rows, 8)
    with R.hp():
        for i in range(n):
            r = R.stress_cell(k, *[rows[q][i] for q in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 16)])
            for q, Nq, g in ((0, r[4], r[7]), (1, r[5], r[7]), (2, r[6], r[8])):
                assert abs(D(float(out[q][i])) - r[q]) <= R.K_SIGMA * R.stress_bound(rows[14 + q][i], Nq, g), (i, q)
            assert abs(D(float(out[3][i])) - r[3]) <= R.K_ALPHA * R.DU * r[3], i
            assert 50.0 <= out[3][i] <= 300.0, (i, out[3][i])
            if expect_alpha.get(i) is not None:
                assert out[3][i] == expect_alpha[i] and r[3] == D(expect_alpha[i]), (i, out[3][i])


def test_subnormal_mass_under_zero_ice_strength(probe):
    """The set the random comparisons with the reference leave out, and the mass boundary of the "same bits" claim: masses 2^e and
    1.5 x 2^e for every e from -1074 to -1016 (subnormal up to the first normal binades), at the cell and at the corner, under an ice
    strength of 0 and of 27500.

    fm::rcp(m) is NaN where 1 / m overflows the seed.  With P > 0 that is harmless: gamma^2 is beyond alpha+^2 either way.  With P == 0
    the reference has gamma^2 = 0 / m = 0 and alpha-, FAST has 0 * NaN, which the minNum clamp sends to alpha+ like the NaN of m = 0
    (evp_fast_math.h documents it; it takes a thickness below 1e-319 m).  Asserted for stress_update_r:
      * where rcp(m) is finite, and where P > 0: the reference's result under the bounds of everywhere else;
      * where rcp(m) is NaN and P == 0: the reference's result WITH alpha- := alpha+, under the same bounds -- and the reference proper has
        alpha- there, so the deviation is the documented one and nothing else.
    stress_update (rcp inside) has stress_update_r's bits everywhere.  stress_update_s scales the corner's mass by 4, so rcp(4 m) can be
    finite where rcp(m) is not: the two forms may differ ONLY for P == 0 under a subnormal corner mass (asserted); where they do is
    printed (profiles/r20_fast_math_probe.md, the comment of stress_update_s)."""
    k = R.stress_constants()
    ex = np.arange(-1074, -1015)
    m = np.concatenate([np.ldexp(1.0, ex), np.ldexp(1.5, ex[1:])])
    m = np.concatenate([m, m])
    n = m.size
    P = np.where(np.arange(n) < n // 2, 0.0, 27500.0)
    rows = np.zeros((17, n))
    rows[0], rows[1], rows[2], rows[3], rows[4], rows[5] = 1e-7, -3e-8, 2e-8, 5e-8, -1e-8, 1e-8
    rows[6], rows[7], rows[8], rows[9] = P, P, m, m
    rows[12], rows[13] = 1.5e-4, 1.5e-4
    rows[14], rows[15], rows[16] = 1000.0, -2000.0, 500.0
    rows[10] = rows[11] = primitives(probe, m)[2]
    r = launch(probe.fmp_stress, (0, stress_consts(k)), rows, 8)
    p = launch(probe.fmp_stress, (2, stress_consts(k)), rows, 8)
    s = launch(probe.fmp_stress, (1, stress_consts(k)), scaled_for_sums(probe, rows), 8)
    assert np.isfinite(r).all() and np.isfinite(s).all()
    assert same_bits(r, p)
    lost = np.isnan(rows[10])
    assert lost.any() and not lost[m >= DBL_MIN].any()
    print(f"fm::rcp(m) is NaN for m <= {m[lost].max()!r} (2^{np.log2(m[lost].max()):.2f}), finite from {m[~lost].min()!r} (2^{np.log2(m[~lost].min()):.2f}) on")
    k_plus = dict(k, amin=k["amax"])
    deviating = 0
    with R.hp():
        for i in range(n):
            args = [rows[q][i] for q in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 16)]
            ref = R.stress_cell(k, *args)
            if lost[i] and P[i] == 0:
                assert ref[3] == 50 and r[3][i] == 300.0, (i, m[i], r[3][i])
                ref = R.stress_cell(k_plus, *args)
                deviating += 1
            for q, Nq, g in ((0, ref[4], ref[7]), (1, ref[5], ref[7]), (2, ref[6], ref[8])):
                assert abs(D(float(r[q][i])) - ref[q]) <= R.K_SIGMA * R.stress_bound(rows[14 + q][i], Nq, g), (i, q, m[i], P[i])
            assert abs(D(float(r[3][i])) - ref[3]) <= R.K_ALPHA * R.DU * ref[3], (i, m[i], P[i])
    assert deviating == int((lost & (P == 0)).sum()) > 0
    differ = (bits(r) != bits(s)).any(axis=0)
    where = np.sort(m[differ])
    print(f"stress_update_s != stress_update_r on {int(differ.sum())} of {n} elements" +
          (f": P = 0 and corner mass from {where[0]!r} to {where[-1]!r} (2^{np.log2(where[0]):.2f} .. 2^{np.log2(where[-1]):.2f}); outputs "
           + ", ".join(OUT8[q] for q in range(8) if (bits(r[q]) != bits(s[q])).any()) if differ.any() else ""))
    assert not differ[(P > 0) | (m >= DBL_MIN)].any()


def test_ext_stress_against_the_reference(probe):
    """kinds 1 - 3; kind 3 under K_EXT u |.|; ice moving exactly with the ocean (n2 = 0): finite, rhoCd sqrt_fast(DBL_MIN), at the stated
    distance from the reference's 0."""
    rng = np.random.default_rng(70)
    n = 20000
    e = np.stack([logmag(rng, n, 1e-6, 10.0), np.full(n, 1026.0 * 5.5e-3), logmag(rng, n, 1e-12, 1e2), logmag(rng, n, 1e-12, 1e2),
                  logmag(rng, n, 1e-12, 1e2), logmag(rng, n, 1e-12, 1e2)])
    e[1][n // 2:] = 1.3 * 1.2e-3
    e[4][:50], e[5][:50] = e[2][:50], e[3][:50]                               # w = we, wbar = webar: n2 = 0
    still = (e[2] == e[4]) & (e[3] == e[5])
    moving = np.nonzero(~still)[0]
    for kind in (1, 2):
        o = launch(probe.fmp_ext_stress, (kind,), e, 4)
        assert same_bits(o[0], e[0]) and (bits(o[1]) == 0).all()
    o = launch(probe.fmp_ext_stress, (3,), e, 4)
    assert np.isfinite(o).all()
    floor = primitives(probe, np.array([DBL_MIN]))[4][0]
    assert same_bits(o[1][still], e[1][still] * floor) and same_bits(o[0][still], o[1][still] * e[2][still])
    dist = float(D(float(o[1][still].max())))
    print(f"ext_stress at n2 = 0: im = rhoCd x {floor!r} (max {dist:.4e}); the reference's is 0")
    assert floor <= 1.4917e-154 * (1 + (R.RSQ_U + 1) * U) and dist <= e[1].max() * 1.4917e-154 * (1 + (R.RSQ_U + 1) * U)
    ref_ex, ref_im = [], []
    with R.hp():
        for i in moving:
            ex, im = R.ext_stress_cell(3, *[e[q][i] for q in range(6)])
            ref_ex.append(ex)
            ref_im.append(im)
        w_ex = R.worst_ratio(o[0][moving], ref_ex, [R.K_EXT * R.DU * abs(v) for v in ref_ex])
        w_im = R.worst_ratio(o[1][moving], ref_im, [R.K_EXT * R.DU * abs(v) for v in ref_im])
    print(f"ext_stress kind 3: worst error / bound ex {w_ex[0]:.4f}, im {w_im[0]:.4f}")
    assert w_ex[0] <= 1.0 and w_im[0] <= 1.0, (w_ex, w_im)


def vel_reference(rows, idx, fd, **pert):
    ref, bnd, what = [], [], []
    with R.hp():
        for i in idx:
            a = [rows[q][i] for q in range(16)]
            r, w, cond = R.vel_cell(VK, a[0], a[1], a[2], a[4], a[6], a[8], a[9], a[10], a[11], a[12], a[13], a[14] != 0, a[15] if fd else None, **pert)
            ref.append(r)
            what.append(w)
            bnd.append(R.DU * cond if (w == R.ACTIVE and a[14] == 0) else D(0))
    return ref, bnd, what


@pytest.mark.parametrize("fd", [False, True])
def test_velocity_update_against_the_reference(probe, fd):
    """vel_update_avg / vel_update_avg_fd, 20 000 elements, against fast_math_ref.vel_cell under K_VEL u N / D (K_VEL = 402, derived in
    fast_math_ref.py for imb >= imt).  The active / marginal / zero decisions must be the reference's exactly: marginal ice gets the
    free-drift velocity bit for bit (0 without one), no ice and peripheral points get +0.  (The reference's `sel * active` keeps the sign
    of sel in a peripheral zero; FAST writes +0.)  Power: the reference with dt off by 2^-40 must violate the bound somewhere."""
    n = 20000
    rows = vel_inputs(n, seed=80 + fd, ordered_drag=True)
    rows[2] = np.where(np.arange(n) % 2 == 0, 10.0 ** np.random.default_rng(82).uniform(-1, 4, n), rows[2])     # more active ice
    # the decisions: mi and ai at and one ulp around min_mass, min_conc and eps
    up, dn = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    edge = 0
    for m in (dn(1.0), 1.0, up(1.0), dn(R.EPS64), R.EPS64, up(R.EPS64), 5.0, 0.0, 5e-324):
        for a in (dn(1e-3), 1e-3, up(1e-3), dn(R.EPS64), R.EPS64, up(R.EPS64), 0.5, 0.0, 1.0):
            rows[2][edge], rows[4][edge], rows[14][edge], rows[15][edge] = m, a, 0.0, 0.123456789
            edge += 1
    got = launch(probe.fmp_vel, (1 if fd else 0, vel_consts(VK)), rows, 1)[0]
    assert np.isfinite(got).all()
    ref, bnd, what = vel_reference(rows, range(n), fd)
    what = np.array(what)
    assert all((what[:edge] == w).sum() >= 9 for w in (R.ZERO, R.ACTIVE, R.MARGINAL))
    per = rows[14] != 0
    assert (bits(got[per]) == 0).all() and (bits(got[what == R.ZERO]) == 0).all()
    marg = (what == R.MARGINAL) & ~per
    assert same_bits(got[marg], rows[15][marg] if fd else np.zeros(marg.sum()))
    act = (what == R.ACTIVE) & ~per
    assert act.sum() > n // 4 and (got[act] != 0).all()
    w = ratios(got, ref, bnd, R.K_VEL)
    print(f"vel_update_avg{'_fd' if fd else ''}: worst error / bound {w[0]:.4f} over {int(act.sum())} active points")
    assert w[0] <= 1.0, (w, [rows[q][w[1]] for q in range(16)])
    with R.hp():
        pdt = D(VK["dt"]) * (1 + D(2) ** -40)
    pref, pbnd, _ = vel_reference(rows, range(3000), fd, dt=pdt)
    pw = ratios(got[:3000], pref, pbnd, R.K_VEL)
    print(f"  reference with dt off by 2^-40: worst error / bound {pw[0]:.2f}")
    assert pw[0] > 1.0


def test_fast_mode_refuses_a_plastic_stress_floor_of_zero():
    """Delta_min = 0 with an ice-free cell at rest: rsqrt(0) = inf, P * inf = NaN and fma(NaN, 0, sigma) = NaN where the reference leaves
    sigma alone.  FAST refuses the configuration (CSI_ERR_UNSUPPORTED, include/csi.h); STRICT takes it."""
    import cases
    import climaseaice_jl_amd as csi
    c = cases.make_case(Nx=16, Ny=12, substeps=2, random_uv=0.02)
    for mode, refused in (("fast", True), ("strict", False)):
        m = cases.csi_model(c, mode=mode)
        d, r = m.dynamics, m.dynamics.rheology
        p = csi._lib.EvpParams(r.ice_compressive_strength, r.ice_compaction_hardening, r.yield_curve_eccentricity, 0.0,
                               r.min_relaxation_parameter, r.max_relaxation_parameter, r.relaxation_strength, csi._lib.PRESSURE_REPLACEMENT,
                               1, float(d.coriolis.f), d.minimum_concentration, d.minimum_mass, m.sea_ice_density)
        m.ctx.call("csi_evp_params_set", C.byref(p))
        if refused:
            with pytest.raises(csi._lib.CsiError) as err:
                csi.time_step_momentum(m, c["dt"])
            assert "CSI_MODE_FAST does not support" in str(err.value)
        else:
            csi.time_step_momentum(m, c["dt"])          # (what it computes with Delta = 0 is the reference's business)
            m.synchronize()
