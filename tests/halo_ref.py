"""The local halo fill (fill_halo_regions!(...; only_local_halos = true)) in GATHER form, in numpy.  TEST INFRASTRUCTURE ONLY.

The device code (csrc/csi_dev.h store_with_images and its specialisations) states which halo images an interior cell HAS and stores
them from the owner's thread.  This module states the same rule the other way round: for every parent column (row) a 1-D table says
which interior column (row) its value comes from and how it is changed on the way -- copied, or reflected about a
ValueBoundaryCondition number (2 * value - c) -- and the passes are applied as whole-array gathers in the oracle's and upstream's order:

    1. x over the rows that hold points: 1 .. Ny, plus the wall-face row Ny + 1 of a Face-in-y field on a y wall;
    2. y over the whole stored x extent (halo columns and the extra Face column included);
    3. the north fold (grids.fold_north, pinned to the C oracle by tests/test_oracle_properties.py) with its own periodic x images.

Because step 2 covers the stored x extent, it copies whatever an x-halo column WITHOUT an image holds (Face on a wall, the deeper cells
of a ValueBoundaryCondition side) into the y halo: a stale value.  The library writes corners only as the product of an x image and a y
image and leaves those cells alone.  `classify` names them CORNER_UNSPECIFIED; tests/test_halo_ref.py pins `fill` to the C oracle on
every cell, those included, and tests/test_gpu_halo_fill.py asserts that the library does not store there.

Arrays are parents in the oracle's layout: a[j + Hy - 1, i + Hx - 1] is element (i, j) of the reference's 1-based indexing.

Topologies (one letter per direction): "P" Periodic, "B" Bounded, "F" RightFolded (y only: wall below, north fold above), "C"
FullyConnected (both sides left to the halo exchange: no local image; unlike the oracle's x pass, which on a tile runs over the rows
beyond a connected y side as well, nothing is gathered there -- the library's local fill does not touch those rows either).
A grid must be at least as wide as its halo in a direction that has images (N >= H): the rule needs ONE interior source per halo
cell, and `gather_table` asserts it.  On the fold a Center-in-y field's row Ny + Hy is the image of row Ny - Hy, a point only when
Ny >= Hy + 1; at Ny == Hy the oracle reads row 0 there, itself the mirror image of row 1, and `fill` follows it.  `supported` states
what the library accepts: N >= H where there are images, and that fold source row among the points.
"""
import numpy as np

from climaseaice_jl_amd import fold_north

INTERIOR, SPECIFIED, UNTOUCHED, CORNER_UNSPECIFIED = 0, 1, 2, 3
CLASS_NAMES = {INTERIOR: "INTERIOR", SPECIFIED: "SPECIFIED", UNTOUCHED: "UNTOUCHED", CORNER_UNSPECIFIED: "CORNER_UNSPECIFIED"}
CENTER, FACE = 0, 1
WRAP, MIRROR, VALUE, NONE, FOLD = "wrap", "mirror", "value", "none", "fold"


def side_modes(topo, loc, values=(None, None)):
    """(low, high) image mode of one direction for a field at `loc` there; values: ValueBoundaryCondition numbers (low, high), which
    replace the no-flux mirror of a Center location on a wall."""
    def wall(v):
        if loc == FACE:
            return NONE
        return MIRROR if v is None else VALUE
    if topo == "P":
        return WRAP, WRAP
    if topo == "B":
        return wall(values[0]), wall(values[1])
    if topo == "F":
        return wall(values[0]), FOLD
    if topo == "C":
        return NONE, NONE
    raise ValueError(f"unknown topology {topo!r}")


def extra_point(topo, loc):
    """1 where a Face location has one more point on the high wall of a Bounded direction."""
    return 1 if (topo == "B" and loc == FACE) else 0


def parent_shape(Nx, Ny, Hx, Hy, loc, topo):
    return (Ny + 2 * Hy + extra_point(topo[1], loc[1]), Nx + 2 * Hx + extra_point(topo[0], loc[0]))


def supported(Nx, Ny, Hx, Hy, loc, topo, value_x=(None, None), value_y=(None, None)):
    """Every halo cell that has an image has its source among the points of the field."""
    mx, my = side_modes(topo[0], loc[0], value_x), side_modes(topo[1], loc[1], value_y)
    ok = not (any(m in (WRAP, MIRROR) for m in mx) and Nx < Hx)
    ok &= not (any(m in (WRAP, MIRROR) for m in my) and Ny < Hy)
    if my[1] == FOLD:
        ok &= Nx >= Hx and Ny >= Hy + (0 if loc[1] == FACE else 1)
    return bool(ok)


def gather_table(N, H, extra, modes):
    """The 1-D rule.  For the n = N + 2H + extra stored indices k = 1 - H .. N + H + extra of one direction:
    kind[t] INTERIOR / SPECIFIED / UNTOUCHED, src[t] the ARRAY position (0-based) the value comes from, refl[t] True where it is
    reflected (2 * value - c) instead of copied.  A fold side has no entry here (UNTOUCHED): it is the third pass."""
    n = N + 2 * H + extra
    kind = np.full(n, UNTOUCHED, dtype=np.int8)
    src = np.arange(n)
    refl = np.zeros(n, dtype=bool)
    lo, hi = modes
    for t in range(n):
        k = t - H + 1
        s = None
        if 1 <= k <= N + extra:
            kind[t] = INTERIOR
            continue
        if k < 1:
            depth = 1 - k                       # 1 = the halo cell next to the edge
            if lo == WRAP:
                s = N + 1 - depth
            elif lo == MIRROR:
                s = depth
            elif lo == VALUE and depth == 1:
                s, refl[t] = 1, True
        else:
            depth = k - N
            if hi == WRAP:
                s = depth
            elif hi == MIRROR:
                s = N + 1 - depth
            elif hi == VALUE and depth == 1:
                s, refl[t] = N, True
        if s is not None:
            assert 1 <= s <= N, ("the source of a halo cell must be an interior point", k, s, N, H)
            kind[t] = SPECIFIED
            src[t] = s + H - 1
    return kind, src, refl


def _tables(Nx, Ny, Hx, Hy, loc, topo, value_x, value_y):
    mx, my = side_modes(topo[0], loc[0], value_x), side_modes(topo[1], loc[1], value_y)
    tx = gather_table(Nx, Hx, extra_point(topo[0], loc[0]), mx)
    ty = gather_table(Ny, Hy, extra_point(topo[1], loc[1]), my)
    return mx, my, tx, ty


def classify(Nx, Ny, Hx, Hy, loc, topo, value_x=(None, None), value_y=(None, None)):
    """The class of every parent cell, from the topology and the sizes alone."""
    mx, my, (kx, _, _), (ky, _, _) = _tables(Nx, Ny, Hx, Hy, loc, topo, value_x, value_y)
    ky = ky.copy()
    if my[1] == FOLD:
        ky[Hy + Ny:Hy + Ny + Hy] = SPECIFIED            # the fold rows; x is Periodic there, every column has its image
    cls = np.full((ky.size, kx.size), UNTOUCHED, dtype=np.int8)
    rows_in, rows_img = (ky == INTERIOR)[:, None], (ky == SPECIFIED)[:, None]
    cols_in, cols_img, cols_none = (kx == INTERIOR)[None, :], (kx == SPECIFIED)[None, :], (kx == UNTOUCHED)[None, :]
    cls[rows_in & cols_in] = INTERIOR
    cls[rows_in & cols_img] = SPECIFIED
    cls[rows_img & (cols_in | cols_img)] = SPECIFIED
    cls[rows_img & cols_none] = CORNER_UNSPECIFIED
    # where the oracle's pass order and the library differ: only in the Hx x Hy corner blocks (the high block starts one column
    # further out where a Face field has its extra column), and nowhere when both x sides image all of their Hx halo columns
    ex = extra_point(topo[0], loc[0])
    corner = np.zeros_like(cls, dtype=bool)
    for rows in (slice(0, Hy), slice(Hy + Ny, Hy + Ny + Hy)):
        corner[rows, :Hx] = True
        corner[rows, Hx + Nx + ex:] = True
    assert not np.any((cls == CORNER_UNSPECIFIED) & ~corner), "CORNER_UNSPECIFIED outside the corner blocks"
    if all(m in (WRAP, MIRROR) for m in mx):
        assert not np.any(cls == CORNER_UNSPECIFIED), "CORNER_UNSPECIFIED although both x sides have images"
    return cls


def fill(parent, Nx, Ny, Hx, Hy, loc, topo, fold_sign=1, value_x=(None, None), value_y=(None, None)):
    """(filled copy of `parent`, classification).  loc = (LX, LY), CENTER / FACE; topo = two letters; value_x / value_y:
    ValueBoundaryCondition numbers per side (low, high) of the x / y walls, None for the default."""
    a = np.array(parent, dtype=np.float64, copy=True)
    assert a.shape == parent_shape(Nx, Ny, Hx, Hy, loc, topo), (a.shape, parent_shape(Nx, Ny, Hx, Hy, loc, topo))
    mx, my, (kx, sx, rx), (ky, sy, ry) = _tables(Nx, Ny, Hx, Hy, loc, topo, value_x, value_y)
    # 1. x: every halo column that has an image, on the rows that hold points, from the untouched input
    rows = np.flatnonzero(ky == INTERIOR)
    for t in np.flatnonzero(kx == SPECIFIED):
        v = a[rows, sx[t]]
        if rx[t]:
            v = 2 * float(value_x[0] if t < Hx else value_x[1]) - v
        a[rows, t] = v
    # 2. y: every halo row that has an image, over the whole stored x extent, from the result of 1.
    for t in np.flatnonzero(ky == SPECIFIED):
        v = a[sy[t], :]
        if ry[t]:
            v = 2 * float(value_y[0] if t < Hy else value_y[1]) - v
        a[t, :] = v
    # 3. the fold
    if my[1] == FOLD:
        a = fold_north(a, Nx, Ny, Hx, Hy, loc[0] == FACE, loc[1] == FACE, fold_sign)
    return a, classify(Nx, Ny, Hx, Hy, loc, topo, value_x, value_y)


def sentinel_parent(shape, Hx, Hy, interior, seed=0):
    """A parent whose points hold `interior` (shape minus the halos) and whose halo cells hold distinct finite sentinels: one per cell,
    negative and beyond -1e6, so different from every interior value a test uses (all of which are > -1e6)."""
    nj, ni = shape
    a = -(1.0e6 + 1000.0 * seed + np.arange(nj * ni, dtype=np.float64).reshape(nj, ni) + 0.25)
    assert interior.shape == (nj - 2 * Hy, ni - 2 * Hx) and np.all(interior > -1.0e6)
    a[Hy:nj - Hy, Hx:ni - Hx] = interior
    return a


def same_bits(x, y):
    """Element-wise bit equality of two float64 arrays (-0.0 differs from 0.0, NaN equals the same NaN)."""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) == np.ascontiguousarray(y, dtype=np.float64).view(np.uint64)
