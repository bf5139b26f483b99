"""CPU side of the per-face advection tests (no GPU): tests/advect_ref.py against everything it can be held to without a kernel.

  * its coefficient tables against the exact rational derivation of tests/test_weno_published.py;
  * its float32 weights against the oracle's f32-weight mode, bit for bit (ora_test_weno(100 + order));
  * its restatement of the order reduction and of the STRICT functions against ora_weno_flux_x / _y, bit for bit at every face of the
    grids the GPU test uses -- and a deliberately wrong reduction decision is seen by that comparison;
  * the derived bound: valid under an 80-digit emulation in which EVERY operation errs by a full u (common sign, alternating, random
    -- not the per-operation worst signs, which are not enumerable: see the test), sharp
    enough to see any literal constant off by 2^-40, and not vacuous on the input families (the share of sharp faces);
  * the FAST function as written with one constant off by 2^-40 fails the comparison the GPU test makes.
"""
from fractions import Fraction as Fr

import numpy as np
import pytest

import advect_ref as A
import cases
import fast_math_ref as R
from advect_ref import D
from test_weno_published import _hook, _published

NX, NY, H = 130, 26, 4
TOPOS = {"pp": ("periodic", "periodic"), "bb": ("bounded", "bounded"), "pb": ("periodic", "bounded")}
P40 = 1 + Fr(1, 2 ** 40)


# ---- inputs: made once, never written to --------------------------------------------------------------------------------------------
_FIELDS = {}


def fields(f32=False):
    if f32 not in _FIELDS:
        FX, FY, rows, cols = A.family_fields(NX, NY, seed=77 if f32 else 7, f32=f32)
        for a in (FX, FY):
            a.setflags(write=False)
        _FIELDS[f32] = (FX, FY, rows, cols)
    return _FIELDS[f32]


def stencils_by_family(order, f32=False, per_family=None):
    """{family: [stencil tuples]} of 2B - 1 consecutive values along the family lines of FX (periodic wrap), both directions"""
    FX, _, rows, _ = fields(f32)
    n = order
    out = {}
    for j, name in enumerate(rows):
        line = np.concatenate([FX[j], FX[j][:n]])
        for i in range(NX):
            p = tuple(float(v) for v in line[i:i + n])
            out.setdefault(name, []).extend([p, p[::-1]])
    if per_family:
        rng = np.random.default_rng(order)
        out = {k: [v[t] for t in rng.choice(len(v), per_family, replace=False)] for k, v in out.items()}
    return out


# ---- 1. the tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [3, 5, 7])
def test_tables_are_the_exact_rational_derivation(order):
    """Candidate coefficients, linear weights, every beta coefficient and the UpwindBiased combination of advect_ref.py equal the
    Jiang-Shu / Balsara-Shu integrals derived in rationals (test_weno_published._published); WENO7's indicators x 240 / 1000."""
    r = A.B_OF[order]
    q, d, beta, big = _published(r)
    for s in range(r):
        for k in range(order):
            assert Fr(A.QN[order][s][k]) * A.QD[order] == q[s][k], (order, s, k)
        assert A.LIN[order][s] == d[s], (order, s)
        scale = (Fr(240, 1000) if order == 7 else Fr(1))
        for i in range(order):
            for j in range(i, order):
                want = scale * (beta[s][i][j] if i == j else beta[s][i][j] + beta[s][j][i])
                assert A.BETA[order][s].get((i, j), Fr(0)) * A.BD[order] == want, (order, s, i, j)
    if order in A.UPW:
        c, dd = A.UPW[order]
        assert [Fr(v) * dd for v in c] == list(big)
    # tau: the combination that vanishes on polynomials of degree <= r - 1 for every candidate pair (asserted on the oracle in
    # test_weno_published.py); here: the literal
    assert A.TAU[order] == {3: [1, -1], 5: [1, 0, -1], 7: [1, 3, -3, -1]}[order]
    assert Fr(A.EPS) == Fr(1e-8)


# ---- 2. float32 weights --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [3, 5, 7])
def test_float_weights_equal_the_oracles_bit_for_bit(order, oracle_lib):
    """beta, tau, the unnormalised weights (numpy.float32, advect_ref.weights_f32) against weno*_parts_f32 of the C oracle on every family
    of the f32 input set, 1e-30 (float squares underflow) and 1e3 included; the value against the oracle's within the STRICT bound."""
    worst = 0.0
    for name, sts in stencils_by_family(order, f32=True, per_family=60).items():
        for p in sts:
            a, S, b, tau = A.weights_f32(p, order)
            o = _hook(oracle_lib, 100 + order, np.array(p))
            assert np.array_equal(a.astype(np.float64), o["alpha"]), (order, name, p, a, o["alpha"])
            assert np.array_equal(b.astype(np.float64), o["beta"]) and float(tau) == o["tau"], (order, name, p)
            v, bound = A.weno_f32_exact(p, order, "strict")
            with R.hp():
                err = abs(D(float(o["value"])) - v)
                assert err <= bound, (order, name, p, float(err), float(bound))
                if bound:
                    worst = max(worst, float(err / bound))
    print(f"WENO{order} f32 weights: oracle value against the exact one, worst error / STRICT bound {worst:.3f}")


# ---- 3. order reduction and the STRICT functions against the oracle, face by face --------------------------------------------------------
def lines_of(c, p):
    s = p.s
    active = None
    if c.get("mask") is not None:
        active = p._mask.astype(bool)
    return A.Lines(s.Nx, s.Ny, s.Hx, s.Hy, c["topo"][0] == "bounded", c["topo"][1] == "bounded", active)


def immersed_mask():
    """hand-placed land on the 130 x 26 grid: single cells, a bar and a block, so that wet faces sit at every distance 1 .. 4 from land
    on either side along x and along y, alone and (bounded topology) together with a wall"""
    wet = np.ones((NY, NX), dtype=bool)
    for j, i in ((12, 10), (12, 13), (12, 18), (12, 24), (12, 32),          # gaps of 2, 4, 5, 7 wet cells along x
                 (3, 40), (5, 40), (9, 40), (14, 40), (21, 40),              # gaps of 1, 3, 4, 6 along y
                 (12, 1), (12, 3), (1, 60), (3, 60), (12, 128), (12, 125), (24, 70), (21, 70), (2, 90), (23, 90)):   # next to the walls
        wet[j, i] = False
    wet[6:9, 100:104] = False
    wet[18, 50:58] = False
    # five wet cells between a wall and land: their inner faces have the wall at 1 .. 4 on one side and land at 4 .. 1 on the other
    wet[15, 5] = wet[15, NX - 6] = wet[5, 115] = wet[NY - 6, 115] = False
    return wet


def face_surroundings(wet, walls):
    """{direction: {(dl, what, dr, what)}} over the open faces of a mask: the number of wet cells below / above the face up to the first
    inactive one (counted to 5: "further than any stencil") and what ends the run: "land", "wall" or None.  Written apart from
    advect_ref.Lines: this is about the mask, not about the rule."""
    out = {}
    for along_y in (False, True):
        N = wet.shape[0 if along_y else 1]
        found = set()
        for m in range(wet.shape[1 if along_y else 0]):
            line = wet[:, m] if along_y else wet[m, :]

            def run(k, step):
                d = 0
                while d < 5:
                    if k < 0 or k >= N:
                        if walls:
                            return d, "wall"
                        k %= N
                    if not line[k]:
                        return d, "land"
                    d, k = d + 1, k + step
                return 5, None
            for f in range(N + 1 if walls else N):                 # face f lies between cells f - 1 and f
                lo, hi = run(f - 1, -1), run(f, 1)
                if lo[0] and hi[0]:
                    found.add(lo + hi)
        out["y" if along_y else "x"] = found
    return out


@pytest.mark.parametrize("walls", [True, False])
def test_land_mask_offers_every_distance_on_either_side(walls):
    """The hand-placed land, pinned: along x and along y there are open faces with land 1, 2, 3 and 4 wet cells away on the low side and
    nothing within five cells on the high side, the same with the sides exchanged, and (bounded grid) with a wall 1 .. 4 cells away on
    the other side, in both arrangements."""
    for direction, found in face_surroundings(immersed_mask(), walls).items():
        for d in (1, 2, 3, 4):
            assert (d, "land", 5, None) in found and (5, None, d, "land") in found, (direction, d, "alone")
            if walls:
                assert any(t[:2] == (d, "land") and t[3] == "wall" for t in found), (direction, d, "land below, wall above")
                assert any(t[2:] == (d, "land") and t[1] == "wall" for t in found), (direction, d, "wall below, land above")


_CASES = {}


def comb_case(topo, land=False, f32=False):
    key = (topo, land, f32)
    if key not in _CASES:
        c = cases.make_case(Nx=NX, Ny=NY, H=H, topo=TOPOS[topo], spacing=1.0, substeps=2, patches=False, noise=0.0)
        if land:
            c["mask"] = immersed_mask()
        _CASES[key] = c
    return _CASES[key]


def set_comb(p, L, FX, FY, along_y, parity, flip):
    u, v, sign = A.comb(L, along_y, parity, flip)
    F = FY if along_y else FX
    p.interior("h")[...] = F
    p.interior("aice")[...] = np.roll(F, 5, axis=1 if along_y else 0)
    p.interior("u")[...] = u
    p.interior("v")[...] = v
    p.update_state()
    return sign


def strict_twin(L, parent, scheme, faces, along_y, blunder=None):
    """the face values as the Python rule and the as-written STRICT functions give them, in doubles"""
    out = []
    for i, j, s in faces:
        if L.closed(i, j, along_y):
            out.append(0.0)
            continue
        B = L.buffer_at(scheme, i, j, along_y, s > 0, blunder)
        p = L.stencil(parent, B, i, j, along_y, s > 0)
        out.append(p[0] if B == 1 else A.as_written(p, (2 * B - 1) * (1 if scheme > 0 else -1), "strict"))
    return np.array(out)


def oracle_faces(p, scheme, name, faces, along_y):
    fn = p.L.ora_weno_flux_y if along_y else p.L.ora_weno_flux_x
    fs = p.field_struct(name)
    return np.array([s * fn(p.ptr, scheme, fs, i, j) for i, j, s in faces])


@pytest.mark.parametrize("topo,land", [("pp", False), ("bb", False), ("pb", False), ("bb", True), ("pp", True)])
def test_python_rule_and_strict_functions_equal_the_oracle_at_every_face(topo, land, oracle_lib):
    """Every face of the grids of the GPU test, both directions, both biases, all six schemes: rule + stencil + function in Python equal
    ora_weno_flux_x / _y bit for bit.  This pins advect_ref's order reduction (topological and immersed, closed faces) to the oracle."""
    c = comb_case(topo, land)
    p = cases.oracle_problem(c)
    L = lines_of(c, p)
    FX, FY, _, _ = fields()
    seen = set()
    for along_y in (False, True):
        for parity in (0, 1):
            for flip in (False, True):
                sign = set_comb(p, L, FX, FY, along_y, parity, flip)
                faces = A.faces_of(L, sign, along_y)
                for scheme in A.SCHEMES:
                    for name in ("h", "aice"):
                        got = strict_twin(L, p.f[name], scheme, faces, along_y)
                        want = oracle_faces(p, scheme, name, faces, along_y)
                        assert A.same_bits(got + 0.0, want + 0.0), (topo, land, along_y, parity, flip, scheme, name,
                                                                    [f for f, g, w in zip(faces, got, want) if g != w][:4])
                    seen.update((scheme, L.buffer_at(scheme, i, j, along_y, s > 0)) for i, j, s in faces if not L.closed(i, j, along_y))
    if topo != "pp" or land:
        assert {(7, B) for B in (1, 2, 3, 4)} <= seen and {(5, B) for B in (1, 2, 3)} <= seen      # every reduced order occurred
    if land:
        assert any(L.closed(i, j, False) for i in range(1, NX + 1) for j in range(1, NY + 1))


def test_a_wrong_reduction_decision_is_seen_by_the_strict_comparison(oracle_lib):
    """One face next to the west wall takes the unreduced WENO7 stencil (it reads the halo): the twin differs from the oracle there and
    nowhere else.  The GPU test makes this comparison with the kernel's value in the twin's place."""
    c = comb_case("bb")
    p = cases.oracle_problem(c)
    L = lines_of(c, p)
    FX, FY, _, _ = fields()
    sign = set_comb(p, L, FX, FY, False, 0, False)
    faces = A.faces_of(L, sign, False)
    bad = next((i, j, False) for i, j, s in faces if i == 2 and s > 0 and FX[j - 1, 0] != FX[j - 1, 1])
    got = strict_twin(L, p.f["h"], 7, faces, False, blunder=bad)
    want = oracle_faces(p, 7, "h", faces, False)
    differs = [(i, j) for (i, j, s), g, w in zip(faces, got, want) if g != w]
    assert differs == [bad[:2]], differs


# ---- 4. the bound -------------------------------------------------------------------------------------------------------------------
def sign_policies(seed):
    rng = np.random.default_rng(seed)
    state = {"k": 0}

    def alternating():
        state["k"] += 1
        return 1 if state["k"] % 2 else -1
    return {"all up": lambda: 1, "all down": lambda: -1, "alternating": alternating, "random": lambda: 1 if rng.random() < 0.5 else -1}


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("scheme", [7, 5, 3, -5, -3])
def test_bound_holds_when_every_operation_errs_by_a_full_u(scheme, mode):
    """The function as written (advect_ref.as_written) evaluated at 80 digits with EVERY operation's result multiplied by (1 +- u), every
    reciprocal's by (1 +- RCP_U u) and every non-double constant by (1 +- u): all signs up, all down, alternating, random.  The
    distance to the exact value stays under the bound on 25 stencils of every family (300 per scheme), and the largest ratio is printed:
    the bound is within an order of magnitude of what this model of the arithmetic can reach.

    Two departures from "exact rational emulation, every rounding at its worst sign", stated: the emulation runs at 80 digits, not in
    rationals (its own error, 1e-80 per operation, is 64 orders below u; rationals of this depth cost seconds per stencil), and the
    four sign patterns are NOT the per-operation worst signs -- those depend on the data through the nonlinear weights and are not
    enumerable (2^150 patterns for WENO7).  What the patterns reach is printed: 0.93 - 1.00 of the FAST bound, 0.47 - 0.86 of the STRICT
    one, so the worst pattern can add little."""
    order = abs(scheme)
    worst, where = 0.0, None
    for name, sts in stencils_by_family(order, per_family=25).items():
        for n, p in enumerate(sts):
            if scheme > 0:
                e = A.weno_exact(p, order)
                exact, bound = e["value"], A.weno_bound(e, order, mode)
            else:
                exact, ab = A.linear_exact(p, order)
                bound = A.linear_bound(ab, order)
            for pol, signs in sign_policies(n).items():
                with R.hp():
                    got = A.as_written([A.Emu(v, signs) for v in p], scheme, mode).v
                    err = abs(got - exact)
                    assert err <= bound, (scheme, mode, name, pol, p, float(err), float(bound))
                    if bound and name not in A.ILL and float(err / bound) > worst:
                        worst, where = float(err / bound), (name, pol)
    print(f"scheme {scheme} {mode}: worst emulated error / bound {worst:.3f} at {where}")
    assert worst > (0.02 if scheme > 0 else 0.1), (scheme, mode, worst)


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("scheme", [7, 5, 3, -5, -3])
def test_doubles_as_written_stay_under_the_bound(scheme, mode):
    """The same functions in IEEE doubles (the unfused stand-in for the kernel) on 100 stencils of every family."""
    order = abs(scheme)
    worst = 0.0
    for name, sts in stencils_by_family(order, per_family=100).items():
        for p in sts:
            v, b, _ = A.reconstruct_exact(p, scheme, A.B_OF[scheme])
            got = A.as_written(p, scheme, mode)
            with R.hp():
                err = abs(D(got) - v)
                assert err <= b[mode], (scheme, mode, name, p, float(err), float(b[mode]))
                if b[mode]:
                    worst = max(worst, float(err / b[mode]))
    print(f"scheme {scheme} {mode}: doubles as written, worst error / bound {worst:.4f}")


# (scheme, constant) -> the smallest k at which a relative perturbation 2^-k is seen, where that is not 40; with the reason
COARSENED = {}


@pytest.mark.parametrize("scheme", [7, 5, 3, -5, -3])
def test_every_literal_constant_off_by_2_to_the_minus_40_is_seen(scheme):
    """Each literal of the function, multiplied by (1 + 2^-40) in the REFERENCE, moves the exact value of at least one stencil of the
    committed input set by more than twice that stencil's FAST bound (the larger of the two): had the kernel that constant, the GPU
    comparison would fail there whatever its roundings did."""
    order = abs(scheme)
    pool = stencils_by_family(order, per_family=40)
    order_of_search = [k for k in ("step", "step2", "rand", "mixed", "spike", "big", "smooth", "tiny") if k in pool]
    base = {}
    unseen = []
    for name in A.literal_constants(scheme):
        T = A.Tables(scheme, {name: P40})
        seen = False
        for fam in order_of_search:
            for p in pool[fam]:
                if p not in base:
                    v, b, _ = A.reconstruct_exact(p, scheme, A.B_OF[scheme])
                    base[p] = (v, b["fast"])
                v0, b0 = base[p]
                with R.hp():
                    v1 = A.weno_exact(p, order, T)["value"] if scheme > 0 else A.linear_exact(p, order, T)[0]
                    if abs(v1 - v0) > 2 * b0:
                        seen = True
                        break
            if seen:
                break
        if not seen:
            unseen.append(name)
    assert unseen == sorted(k for s, k in COARSENED if s == scheme), (scheme, unseen)


@pytest.mark.parametrize("scheme", [7, 5, 3, -5, -3])
def test_fast_function_with_one_constant_off_fails_the_gpu_comparison(scheme):
    """Sharpness, independently of any kernel: the FAST function as written in doubles passes the comparison the GPU test makes (error
    <= FAST bound at every stencil); with ONE constant off by 2^-40 -- a candidate coefficient, a linear weight, a beta coefficient,
    eps -- it fails it."""
    order = abs(scheme)
    pool = [p for fam, sts in stencils_by_family(order, per_family=40).items() if fam not in A.ILL for p in sts]

    def fails(pert):
        for p in pool:
            v, b, _ = A.reconstruct_exact(p, scheme, A.B_OF[scheme])
            with R.hp():
                if abs(D(A.as_written(p, scheme, "fast", pert)) - v) > b["fast"]:
                    return True
        return False
    assert not fails(None)
    names = A.literal_constants(scheme)
    picks = [names[0], names[len(names) // 2], names[-1]] + ([k for k in names if k[0] == "lin"][:1] + [k for k in names if k[0] == "b"][:1])
    for name in picks:
        assert fails({name: P40}), (scheme, name)


@pytest.mark.parametrize("scheme", [7, 5, 3, -5, -3])
def test_share_of_sharp_faces_per_family(scheme):
    """Against vacuity: in every family except the two eps-scale ones at least half of the stencils have a FAST bound <= 1e-13 of
    max |stencil| (from the reference alone).  The eps-scale families' figures are printed, not capped."""
    order = abs(scheme)
    for fam, sts in stencils_by_family(order, per_family=100).items():
        rel = []
        for p in sts:
            _, b, m = A.reconstruct_exact(p, scheme, A.B_OF[scheme])
            rel.append(float(b["fast"]) / m if m else 0.0)
        rel = np.array(rel)
        share = float((rel <= 1e-13).mean())
        print(f"scheme {scheme} {fam:9s}: sharp share {share:.2f}, median bound / max|stencil| {np.median(rel):.2e}, largest {rel.max():.2e}")
        if fam not in A.ILL:
            assert share >= 0.5, (scheme, fam, share)


# ---- 5. the tracer update's restatement against the oracle ------------------------------------------------------------------------------
def branch_table(n=48):
    """cells enumerating the branches of _dynamic_step_tracers! / dynamic_step_snow!: (hn, an, Gh, Ga, sn, Ghs), dt = 1"""
    rows = [(0.5, 0.5, -1.0, 0.1, 0.2, 0.0),         # h+ < 0
            (0.5, 0.5, 0.1, -1.0, 0.2, 0.1),         # a+ < 0, snow over a <= 0
            (0.5, 0.5, -0.5, 0.1, 0.2, 0.0),         # h+ == 0 exactly, a+ > 0
            (0.5, 0.5, 0.1, -0.5, 0.2, 0.0),         # a+ == 0 exactly, h+ > 0
            (0.5, 0.9, 0.1, 0.3, 0.2, 0.1),          # a+ > 1: ridging
            (0.5, 0.5, 0.1, 0.1, 0.2, -1.0),         # plain, snow clipped
            (-0.0, 0.5, -0.0, 0.1, 0.0, -0.0),       # -0.0 in h+
            (0.5, -0.0, 0.1, -0.0, 0.1, 0.1),        # -0.0 in a+
            (0.5, 0.5, np.nan, 0.1, 0.2, 0.0), (0.5, 0.5, 0.1, np.nan, 0.2, np.nan), (np.nan, np.nan, 0.0, 0.0, 0.1, 0.0),
            (0.5, 0.5, np.inf, 0.1, 0.2, 0.0), (0.5, 0.5, 0.1, np.inf, 0.2, np.inf), (0.5, 0.5, -np.inf, 0.1, 0.2, -np.inf),
            (0.5, 0.5, 0.1, -np.inf, 0.2, 0.0), (0.0, 0.5, 0.0, np.inf, 0.0, 0.0), (0.5, 0.5, np.inf, np.inf, 0.1, 0.1),
            (1e-320, 0.5, 0.0, 0.0, 1e-320, 0.0), (0.5, 1.0, 0.0, 5e-17, 0.1, 0.0), (0.0, 0.0, 0.0, 0.0, 0.3, 0.0)]
    t = np.array([rows[k % len(rows)] for k in range(n)]).T
    return [np.ascontiguousarray(r) for r in t]


@pytest.mark.parametrize("from_cache", [False, True])
def test_tracer_update_restatement_equals_the_oracle_on_the_branch_table(from_cache, oracle_lib):
    Nx, Ny = 12, 8
    c = cases.make_case(Nx=Nx, Ny=Ny, H=4, spacing=1.0, substeps=2, patches=False, noise=0.0)
    hn, an, Gh, Ga, sn, Ghs = [r[:Nx * Ny].reshape(Ny, Nx) for r in branch_table(Nx * Ny)]
    p = cases.oracle_problem(c)
    p.s.has_snow = 1
    base = ("hm", "am", "hsm") if from_cache else ("h", "aice", "hs")
    for name, val in zip(base + ("Gh", "Ga", "Ghs"), (hn, an, sn, Gh, Ga, Ghs)):
        p.interior(name)[...] = val
    p.dynamic_step_tracers(1.0, from_cache)
    h1, a1, s1, taken = A.tracer_update(hn, an, Gh, Ga, 1.0, sn, Ghs)
    for name, want in (("h", h1), ("aice", a1), ("hs", s1)):
        assert A.same_bits(p.interior(name), want), (name, p.interior(name), want)
    for b in A.BRANCHES:
        assert taken[b].any(), b
