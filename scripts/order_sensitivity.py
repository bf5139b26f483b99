"""How far apart the two orders of a sub-step pair are, on the CPU oracle: what tests/test_gpu_pair_ufirst.py relies on.

A pair of sub-steps that starts on an even sub-step steps u before v, then v before u; one that starts on an odd sub-step does
the opposite (split_explicit_momentum_equations.jl:178-187).  A kernel that ran the wrong order would give the other answer, so a
comparison with the oracle detects it only where the oracle's two answers differ by much more than the comparison's bound
(1e-13 max|u, v| on the velocities, 1e-10 max|sigma| on the stresses).  This script prints, relative to those maxima,

  * for every case of test_even_start_two_substeps_vs_oracle: oracle sub-steps (2, 3) against (1, 2) from the initial state;
  * for every case of test_even_start_along_the_oracle_cycle: the SMALLEST such difference over the states s = 2, 4, .. 118 of the
    120-sub-step cycle (sub-steps (s, s + 1) against (s + 1, s + 2) from the same state);
  * for every case of tests/pair_matrix.py (tests/test_gpu_pair_matrix.py): the distance between the two orders, and the distance between
    the oracle's answer and its answer with the case's distinguishing ingredient removed (pair_matrix.ingredient_removed: ocean
    velocity -> 0, ice_strength -> replacement, arrays -> numbers, free drift off, model.forcing off, ...) -- what tells a CF1 kernel from
    one that ignores the ocean velocity, or a force_w kernel from one that ignores the wind arrays.  A matrix case at or below 1e-10
    of max|u, v| on either distance makes the script fail.

No GPU is needed:  python scripts/order_sensitivity.py [--markdown] [--matrix]      (--matrix: the last table only)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle  # noqa: E402
import cases  # noqa: E402
from test_gpu_pair_ufirst import ORDER_CASES as CASES, ORACLE_CASES, CYCLE_CASES  # noqa: E402

STATE = ("u", "v", "s11", "s22", "s12", "P", "un", "vn")


def rel_diff(a, b):
    vmax = max(np.abs(a.f["u"]).max(), np.abs(a.f["v"]).max(), 1e-30)
    smax = max(np.abs(a.f[k]).max() for k in ("s11", "s22", "s12"))
    smax = max(smax, 1e-30)
    return (np.abs(a.f["u"] - b.f["u"]).max() / vmax, np.abs(a.f["v"] - b.f["v"]).max() / vmax,
            max(np.abs(a.interior(k) - b.interior(k)).max() for k in ("s11", "s22", "s12")) / smax)


def from_initial_state(name):
    c = cases.make_case(substeps=2, **CASES[name])
    out = []
    for first in (2, 1):
        p = cases.oracle_problem(c)
        p.initialize_rheology()
        p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
        p.subcycle(c["dt"], first, first + 1)
        out.append(p)
    return rel_diff(*out)


def along_the_cycle(name):
    c = cases.make_case(substeps=120, **CASES[name])
    p, q = cases.oracle_problem(c), cases.oracle_problem(c)
    p.initialize_rheology(); q.initialize_rheology()
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    p.subcycle(c["dt"], 1, 1)
    least = [np.inf, np.inf, np.inf]
    for s in range(2, 120, 2):
        for k in STATE:
            q.f[k][...] = p.f[k]
        p.subcycle(c["dt"], s, s + 1)
        q.subcycle(c["dt"], s + 1, s + 2)
        least = [min(a, b) for a, b in zip(least, rel_diff(p, q))]
    return least


def two_substeps(kw, first):
    c = cases.make_case(substeps=2, **kw)
    p = cases.oracle_problem(c)
    p.initialize_rheology()
    p.L.ora_fill_halo_u(p.ptr); p.L.ora_fill_halo_v(p.ptr)
    p.subcycle(c["dt"], first, first + 1)
    assert all(np.all(np.isfinite(p.f[k])) for k in STATE), kw
    return p


def matrix_table(md):
    """tests/pair_matrix.py: per case and first sub-step, the distance between the oracle's two orders and the distance between the oracle's
    answer and its answer without the case's distinguishing ingredient (du, dv relative to max|u, v|: the larger of the two)"""
    import pair_matrix as pm
    print("the case matrix (tests/pair_matrix.py), two oracle sub-steps from the initial state, max(du, dv) / max|u,v|:\n"
          "other order; ingredient removed, first = 1; ingredient removed, first = 2; which ingredient")
    if md:
        print("\n| case | instantiation (untiled, v-first) | other order | ingredient removed, first = 1 | first = 2 | ingredient |\n|---|---|---|---|---|---|")
    blind = []
    for name, kw in pm.MATRIX.items():
        what, without = pm.ingredient_removed(kw)
        p1, p2 = two_substeps(kw, 1), two_substeps(kw, 2)
        order = max(rel_diff(p2, p1)[:2])
        gone = [max(rel_diff(p, two_substeps(without, first))[:2]) for first, p in ((1, p1), (2, p2))]
        if min(order, *gone) <= 1e-10:
            blind.append(name)
        key = pm.expected_key(kw)
        print(f"| {name} | `{key}` | {order:.1e} | {gone[0]:.1e} | {gone[1]:.1e} | {what} |" if md else
              f"{name:26s} {key:38s} {order:9.1e} {gone[0]:9.1e} {gone[1]:9.1e}  {what}")
    print("matrix cases at or below 1e-10 on one of the distances (they must be changed or dropped):", blind or "none")
    return blind


def main():
    oracle.build()
    md = "--markdown" in sys.argv
    if "--matrix" in sys.argv:
        return 1 if matrix_table(md) else 0
    row = (lambda n, d: f"| {n} | {d[0]:.1e} | {d[1]:.1e} | {d[2]:.1e} |") if md else (lambda n, d: f"{n:34s} {d[0]:9.1e} {d[1]:9.1e} {d[2]:9.1e}")
    blind = []
    print("two oracle sub-steps from first = 2 against first = 1, initial state: du / max|u,v|, dv / max|u,v|, dsigma / max|sigma|")
    for name in ORACLE_CASES:
        d = from_initial_state(name)
        if max(d[0], d[1]) <= 1e-10:
            blind.append(name)
        print(row(name, d))
    print("the same along the 120-sub-step cycle: smallest difference over s = 2, 4, .. 118")
    for name in CYCLE_CASES:
        d = along_the_cycle(name)
        if max(d[0], d[1]) <= 1e-10:
            blind.append(name + " (cycle)")
        print(row(name, d))
    print("cases whose two orders agree within 1e-10 on the velocities (they cannot detect a swapped order there):", blind or "none")
    return 1 if matrix_table(md) else 0


if __name__ == "__main__":
    sys.exit(main())
