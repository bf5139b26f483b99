"""That the comparisons of tests/test_gpu_advect_layouts.py can fail, on the CPU oracle.

A block shape whose tile is 63 or 64 columns wide and 7, 8 or 11 rows high goes wrong at its seams first: a thread that reads or
stores one column or row off.  The tests compare with the oracle to G_TOL = 1e-12 of max|G| (FAST; STRICT bit for bit), so they see
such a slip only where it moves the oracle's answer by much more than that.  For every grid and topology of the forced matrix and
every scheme this prints how far the oracle's Gh moves, relative to max|Gh|, when one interior column (63, 64, 126) or row (7, 8, 11)
of h takes its neighbour's values -- the smallest over the six schemes -- and, for the snow cases, how far Ghs lies from Gh and Ga
(a kernel that stored the wrong tracer's tendency).  Any figure at or below 1e-9 makes the script fail: change that case's input.

No GPU is needed:  python scripts/advect_layout_sensitivity.py [--markdown]
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
import advect_layouts as al  # noqa: E402
from test_gpu_advect_layouts import forced_case, snow_case, oracle_tendencies, oracle_snow  # noqa: E402

COLUMNS, ROWS = (63, 64, 126), (7, 8, 11)
FLOOR = 1e-9


def shifted(c, column=None, row=None):
    """the case with one column / row (1-based) of h holding the values of the next one"""
    d = dict(c)
    h = c["h"].copy()
    if column is not None:
        h[:, column - 1] = c["h"][:, column]
    else:
        h[row - 1, :] = c["h"][row, :]
    d["h"] = h
    return d


def moved(c, key, **where):
    least = np.inf
    for scheme in al.SCHEMES:
        want = oracle_tendencies(key, c, scheme)["Gh"]
        p = cases.oracle_problem(shifted(c, **where))
        p.compute_tracer_tendencies(scheme)
        least = min(least, np.abs(p.interior("Gh") - want).max() / np.abs(want).max())
    return least


def main():
    oracle.build()
    md = "--markdown" in sys.argv
    low = []
    print("max|dGh| / max|Gh| when one column / row of h takes its neighbour's values, smallest over the six schemes")
    head = ["grid", "topology"] + [f"column {k}" for k in COLUMNS] + [f"row {k}" for k in ROWS]
    print("| " + " | ".join(head) + " |\n|" + "---|" * len(head) if md else " ".join(f"{x:>11s}" for x in head))
    for Nx, Ny in al.FORCED_GRIDS:
        for topo in al.TOPOS:
            key, c = forced_case(Nx, Ny, topo)
            vals = [moved(c, key, column=k) if k < Nx else None for k in COLUMNS] + [moved(c, key, row=k) if k < Ny else None for k in ROWS]
            low += [(Nx, Ny, topo, v) for v in vals if v is not None and v <= FLOOR]
            cells = [f"{Nx} x {Ny}", "/".join(al.TOPOS[topo])] + ["--" if v is None else f"{v:.1e}" for v in vals]
            print("| " + " | ".join(cells) + " |" if md else " ".join(f"{x:>11s}" for x in cells))
    print("\nthe snow cases: max|Ghs - Gh| / max|Gh|, max|Ghs - Ga| / max|Ga|, smallest over the schemes (f32 weights included)")
    for topo in al.TOPOS:
        key, c, hs0 = snow_case(topo)
        d = [np.inf, np.inf]
        for scheme, w32 in [(s, False) for s in al.SCHEMES] + [(s, True) for s in al.WENO]:
            w = oracle_snow(key, c, hs0, scheme, w32)
            d = [min(d[0], np.abs(w["Ghs"] - w["Gh"]).max() / np.abs(w["Gh"]).max()), min(d[1], np.abs(w["Ghs"] - w["Ga"]).max() / np.abs(w["Ga"]).max())]
        low += [(al.SNOW_GRID, topo, v) for v in d if v <= FLOOR]
        print(f"| {al.SNOW_GRID[0]} x {al.SNOW_GRID[1]} | {'/'.join(al.TOPOS[topo])} | {d[0]:.1e} | {d[1]:.1e} |" if md else
              f"{al.SNOW_GRID[0]} x {al.SNOW_GRID[1]} {'/'.join(al.TOPOS[topo]):>20s} {d[0]:9.1e} {d[1]:9.1e}")
    print(f"figures at or below {FLOOR:g} (the comparison could not see that slip there):", low or "none")
    return 1 if low else 0


if __name__ == "__main__":
    sys.exit(main())
