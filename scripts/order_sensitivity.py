"""How far apart the two orders of a sub-step pair are, on the CPU oracle: what tests/test_gpu_pair_ufirst.py relies on.

A pair of sub-steps that starts on an even sub-step steps u before v, then v before u; one that starts on an odd sub-step does
the opposite (split_explicit_momentum_equations.jl:178-187).  A kernel that ran the wrong order would give the other answer, so a
comparison with the oracle detects it only where the oracle's two answers differ by much more than the comparison's bound
(1e-13 max|u, v| on the velocities, 1e-10 max|sigma| on the stresses).  This script prints, relative to those maxima,

  * for every case of test_even_start_two_substeps_vs_oracle: oracle sub-steps (2, 3) against (1, 2) from the initial state;
  * for every case of test_even_start_along_the_oracle_cycle: the SMALLEST such difference over the states s = 2, 4, .. 118 of the
    120-sub-step cycle (sub-steps (s, s + 1) against (s + 1, s + 2) from the same state).

No GPU is needed:  python scripts/order_sensitivity.py [--markdown]
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


def main():
    oracle.build()
    md = "--markdown" in sys.argv
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
