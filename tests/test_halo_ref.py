"""tests/halo_ref.py (the local halo fill in gather form) against the C oracle, on the CPU: BIT FOR BIT ON EVERY CELL of the parent,
the CORNER_UNSPECIFIED cells included -- halo_ref restates the oracle's pass order, so there is nothing to tolerate.

The halos start from distinct finite sentinels (one per cell, different from every interior value), so a cell that a fill must not
touch, or copies from the wrong place, shows.  Matrix: the four locations; (P,P), (P,B), (B,P), (B,B), (P,RightFolded); halos (4,4),
(3,5), (5,2); Nx and Ny each from {H, H+1, 2H-1, 2H, 2H+1} of their own direction plus one size above 64; ValueBoundaryConditions on
u's y walls and v's x walls, low and high separately; both fold signs."""
import numpy as np
import pytest

import halo_ref as R
import oracle as O

TOPOS = {"PP": (O.PERIODIC, O.PERIODIC), "PB": (O.PERIODIC, O.BOUNDED), "BP": (O.BOUNDED, O.PERIODIC), "BB": (O.BOUNDED, O.BOUNDED),
         "PF": (O.PERIODIC, O.RIGHT_FOLDED)}
HALOS = [(4, 4), (3, 5), (5, 2)]
LOCS = {"h": (R.CENTER, R.CENTER), "u": (R.FACE, R.CENTER), "v": (R.CENTER, R.FACE), "s12": (R.FACE, R.FACE)}     # one oracle field per location
VALUES = [(None, None), (0.375, None), (None, -1.25), (0.375, -1.25)]


def sizes(H, big):
    return sorted({H, H + 1, 2 * H - 1, 2 * H, 2 * H + 1, big})


def problem(Nx, Ny, Hx, Hy, topo):
    return O.Problem(Nx, Ny, Hx, Hy, TOPOS[topo])


def seed_field(p, name, seed):
    """Random interior in (0.5, 1.5), sentinel halos; returns the untouched copy."""
    a = p.f[name]
    Hx, Hy = p.s.Hx, p.s.Hy
    rng = np.random.default_rng(seed)
    a[...] = R.sentinel_parent(a.shape, Hx, Hy, 0.5 + rng.random((a.shape[0] - 2 * Hy, a.shape[1] - 2 * Hx)), seed=seed)
    return a.copy()


def assert_same(got, exp, cls, what):
    bad = ~R.same_bits(got, exp)
    if bad.any():
        j, i = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {bad.sum()} cells differ, first at array [{j}, {i}] ({R.CLASS_NAMES[int(cls[j, i])]}): "
                             f"{got[j, i]!r} vs oracle {exp[j, i]!r}")


@pytest.mark.parametrize("halo", HALOS, ids=lambda h: f"H{h[0]}x{h[1]}")
@pytest.mark.parametrize("topo", list(TOPOS))
def test_fill_matches_the_oracle_on_every_cell(topo, halo):
    Hx, Hy = halo
    n = 0
    for Nx in sizes(Hx, 70):
        for Ny in sizes(Hy, 67):
            p = problem(Nx, Ny, Hx, Hy, topo)
            for name, loc in LOCS.items():
                for sign in ((1, -1) if topo == "PF" else (1,)):
                    before = seed_field(p, name, seed=n)
                    p.L.ora_fill_halo_loc(p.ptr, p.field_struct(name), loc[0], loc[1], sign)
                    got, cls = R.fill(before, Nx, Ny, Hx, Hy, loc, topo, fold_sign=sign)
                    assert_same(got, p.f[name], cls, f"{name} {topo} N=({Nx},{Ny}) H={halo} sign {sign}")
                    # the classes say what changed: points never, UNTOUCHED cells never
                    keep = (cls == R.INTERIOR) | (cls == R.UNTOUCHED)
                    assert np.all(R.same_bits(got, before)[keep])
                    # ... and every cell with a source no longer holds its sentinel
                    assert not np.any(R.same_bits(got, before)[(cls == R.SPECIFIED) | (cls == R.CORNER_UNSPECIFIED)])
                    n += 1
    assert n == len(sizes(Hx, 70)) * len(sizes(Hy, 67)) * 4 * (2 if topo == "PF" else 1)      # (H = 2: H + 1 == 2H - 1)


@pytest.mark.parametrize("halo", HALOS, ids=lambda h: f"H{h[0]}x{h[1]}")
@pytest.mark.parametrize("topo", list(TOPOS))
def test_velocity_fills_with_value_boundary_conditions_match_the_oracle(topo, halo):
    """ora_fill_halo_u / _v: ValueBoundaryCondition numbers on u's y walls and v's x walls, low and high separately (on a side that is no
    wall the oracle ignores them, and so must the reference); the fold with the velocities' sign."""
    Hx, Hy = halo
    n = 0
    for Nx in sizes(Hx, 70):
        for Ny in sizes(Hy, 67):
            p = problem(Nx, Ny, Hx, Hy, topo)
            for vals in VALUES:
                for side in (0, 1):
                    p.set_value_bc("u", side, vals[side])
                    p.set_value_bc("v", side, vals[side])
                bu, bv = seed_field(p, "u", seed=2 * n), seed_field(p, "v", seed=2 * n + 1)
                p.L.ora_fill_halo_u(p.ptr)
                p.L.ora_fill_halo_v(p.ptr)
                what = f"{topo} N=({Nx},{Ny}) H={halo} values {vals}"
                got, cls = R.fill(bu, Nx, Ny, Hx, Hy, LOCS["u"], topo, fold_sign=-1, value_y=vals)
                assert_same(got, p.f["u"], cls, "u " + what)
                got, cls = R.fill(bv, Nx, Ny, Hx, Hy, LOCS["v"], topo, fold_sign=-1, value_x=vals)
                assert_same(got, p.f["v"], cls, "v " + what)
                n += 1
    assert n == len(sizes(Hx, 70)) * len(sizes(Hy, 67)) * len(VALUES)


def test_classification_names_the_corner_set():
    """What the classes are, spelled out on one grid: u (Face, Center) on (Bounded, Periodic) with H = (3, 2), N = (5, 4)."""
    Nx, Ny, Hx, Hy = 5, 4, 3, 2
    cls = R.classify(Nx, Ny, Hx, Hy, LOCS["u"], "BP")
    assert cls.shape == (Ny + 2 * Hy, Nx + 2 * Hx + 1)
    rows_halo = [0, 1, Hy + Ny, Hy + Ny + 1]
    assert np.all(cls[Hy:Hy + Ny, Hx:Hx + Nx + 1] == R.INTERIOR)                   # the wall-face column Nx + 1 is a point
    assert np.all(cls[Hy:Hy + Ny, :Hx] == R.UNTOUCHED) and np.all(cls[Hy:Hy + Ny, Hx + Nx + 1:] == R.UNTOUCHED)
    assert np.all(cls[rows_halo, Hx:Hx + Nx + 1] == R.SPECIFIED)
    assert np.all(cls[rows_halo, :Hx] == R.CORNER_UNSPECIFIED) and np.all(cls[rows_halo, Hx + Nx + 1:] == R.CORNER_UNSPECIFIED)
    # a ValueBoundaryCondition side images one cell: the deeper columns have no image, and their y-halo cells are the corner set
    cls = R.classify(Nx, Ny, Hx, Hy, LOCS["v"], "BP", value_x=(0.5, None))
    assert np.all(cls[Hy:Hy + Ny, Hx - 1] == R.SPECIFIED) and np.all(cls[Hy:Hy + Ny, :Hx - 1] == R.UNTOUCHED)
    assert np.all(cls[rows_halo, :Hx - 1] == R.CORNER_UNSPECIFIED) and np.all(cls[rows_halo, Hx - 1:] == R.SPECIFIED)
    # connected sides: no local image at all
    cls = R.classify(Nx, Ny, Hx, Hy, LOCS["h"], "CC")
    assert np.all((cls == R.INTERIOR) | (cls == R.UNTOUCHED)) and (cls == R.INTERIOR).sum() == Nx * Ny


def test_narrower_than_the_halo_has_no_single_source():
    assert not R.supported(3, 8, 4, 4, LOCS["h"], "PP") and not R.supported(8, 3, 4, 4, LOCS["h"], "BB")
    assert R.supported(3, 8, 4, 4, LOCS["u"], "BP")                    # Face on walls: no image in x, any Nx
    assert not R.supported(3, 8, 4, 4, LOCS["v"], "BP") and R.supported(1, 1, 4, 4, LOCS["h"], "CC")
    assert R.supported(8, 4, 4, 4, LOCS["v"], "PF") and not R.supported(8, 4, 4, 4, LOCS["h"], "PF") and R.supported(8, 5, 4, 4, LOCS["h"], "PF")
    with pytest.raises(AssertionError, match="interior point"):
        R.fill(np.zeros((8 + 8, 3 + 8)), 3, 8, 4, 4, LOCS["h"], "PP")
