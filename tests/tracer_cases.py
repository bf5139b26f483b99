"""The grids that tests/test_gpu_tracer_shapes.py holds the tracer kernels (csrc/tracers.hip) to, and the store choice of k_tracer_finish,
stated once; tests/test_tracer_cases_table.py proves the coverage without a GPU.

k_tracer_finish gives one thread the cells (i, i + 1), i odd, of row j of tracer k.  It stores the pair with ONE 16-byte store (and a
second one into the source-free copy an RK3 stage keeps) where the pair has two cells, both addresses are 16-byte aligned and neither
cell has a halo image (csrc/csi_dev.h has_halo_images); otherwise cell by cell through store_with_images.  `finish_path` restates that
choice from the parent geometry the library uses:

    ld = Nx + 2 Hx, nj = Ny + 2 Hy; element (i, j) (1-based) of a parent lies (i + Hx - 1) + (j + Hy - 1) ld doubles behind its base;
    the free copy of tracer k starts k * plane doubles, plane = ld * nj, behind a 16-byte boundary; a tracer array c_offset_doubles
    behind one (0: an allocation of its own; 1: bound by hand one double further); aice on a boundary.

`store_parent` restates store_with_images in SCATTER form -- the owner of (i, j) writes the point and its images -- with the mistakes
the comparisons must be able to see as switches; tests/halo_ref.py states the same rule in gather form and the table test ties the two.
"""
from collections import namedtuple

import numpy as np

PAIR = 2                       # cells per thread of k_tracer_finish
ALIGN_MASK = 15                # ((cp | fp) & 15) == 0: the wide store's alignment
TILE = (63, 7)                 # cells per block of k_tracer_tendencies (TTX, TTY)
FINISH_BLOCK = (128, 4)        # cells per block of k_tracer_finish: 64 threads x 2 cells, 4 rows

WIDE_C, WIDE_C_FREE, SCALAR_C, SCALAR_FREE, SCALAR_IMAGES, LONE = "wide_c", "wide_c_free", "scalar_c_misaligned", "scalar_free_misaligned", "scalar_images", "lone_last"
PATHS = (WIDE_C, WIDE_C_FREE, SCALAR_C, SCALAR_FREE, SCALAR_IMAGES, LONE)
WIDE = (WIDE_C, WIDE_C_FREE)

TOPOS = {"pp": ("periodic", "periodic"), "bb": ("bounded", "bounded"), "pb": ("periodic", "bounded"), "bp": ("bounded", "periodic"),
         "pf": ("periodic", "folded")}
# whether tracer k of tests/test_gpu_tracers.py SPECS8 has a source (the GPU file asserts that this is SPECS8's)
SOURCED8 = (False, True, True, True, True, False, False, True)

FinishPaths = namedtuple("FinishPaths", "paths aice_pair")      # both [row j - 1][pair p]: the pair starts at i = 1 + 2 p


def has_halo_images(i, j, Nx, Ny, Hx, Hy, fold):
    """csrc/csi_dev.h has_halo_images: within H of an edge, one row more below a north fold"""
    in_x, in_y = 1 <= i <= Nx, 1 <= j <= Ny
    near_x = in_x and (i <= Hx or i > Nx - Hx)
    near_y = in_y and (j <= Hy or j > Ny - Hy - (1 if fold else 0))
    return near_x or near_y


def element_offset(i, j, Nx, Hx, Hy):
    return (i + Hx - 1) + (j + Hy - 1) * (Nx + 2 * Hx)


def finish_path(Nx, Ny, Hx, Hy, topo, c_offset_doubles=0, k=0, sourced=False, rk=False):
    """The choice of k_tracer_finish for every pair of every row, and whether aice was loaded as a pair (two cells, aligned address).
    A pair that is scalar for two reasons is named after the first that holds in the order: c misaligned, only the free copy
    misaligned, images -- so SCALAR_IMAGES names the pairs that ONLY the has_halo_images test keeps from the wide store."""
    ld, nj = Nx + 2 * Hx, Ny + 2 * Hy
    plane, fold = ld * nj, topo[1] == "folded"
    free = rk and sourced
    paths, aice_pair = [], []
    for j in range(1, Ny + 1):
        row, arow = [], []
        for i in range(1, Nx + 1, PAIR):
            two = i + 1 <= Nx
            off = element_offset(i, j, Nx, Hx, Hy)
            c_aligned = (8 * (c_offset_doubles + off)) & ALIGN_MASK == 0
            f_aligned = (8 * (k * plane + off)) & ALIGN_MASK == 0 if free else True       # (no free copy: a null pointer, aligned)
            arow.append(two and (8 * off) & ALIGN_MASK == 0)
            if not two:
                row.append(LONE)
            elif not c_aligned:
                row.append(SCALAR_C)
            elif not f_aligned:
                row.append(SCALAR_FREE)
            elif has_halo_images(i, j, Nx, Ny, Hx, Hy, fold) or has_halo_images(i + 1, j, Nx, Ny, Hx, Hy, fold):
                row.append(SCALAR_IMAGES)
            else:
                row.append(WIDE_C_FREE if free else WIDE_C)
        paths.append(row)
        aice_pair.append(arow)
    return FinishPaths(paths, aice_pair)


def path_counts(Nx, Ny, Hx, Hy, topo, **kw):
    out = dict.fromkeys(PATHS, 0)
    for row in finish_path(Nx, Ny, Hx, Hy, topo, **kw).paths:
        for p in row:
            out[p] += 1
    return out


# ---- store_with_images, scatter form ----------------------------------------------------------------------------------------------------------
def _modes(t):
    return {"periodic": ("wrap", "wrap"), "bounded": ("mirror", "mirror"), "folded": ("mirror", "fold")}[t]


def _lo(mode, i, N, H):
    """(has, index) of the LOW-side halo image of interior index i (csi_dev.h image_lo)"""
    if mode == "wrap":
        return i > N - H, i - N
    if mode == "mirror":
        return i <= H, 1 - i
    return False, 0


def _hi(mode, i, N, H):
    if mode == "wrap":
        return i <= H, i + N
    if mode == "mirror":
        return i > N - H, 2 * N + 1 - i
    return False, 0


def image_flags(i, j, Nx, Ny, Hx, Hy, topo):
    """(hxl, hxh, hyl, hyh) of store_with_images for a Center, Center field at interior cell (i, j)"""
    mx, my = _modes(topo[0]), _modes(topo[1])
    return (_lo(mx[0], i, Nx, Hx)[0], _hi(mx[1], i, Nx, Hx)[0], _lo(my[0], j, Ny, Hy)[0], _hi(my[1], j, Ny, Hy)[0])


MISTAKES = ("halos_transposed", "second_x_image_dropped", "second_y_image_dropped", "corner_dropped", "pair_without_images")


def store_parent(parent, interior, Nx, Ny, Hx, Hy, topo, mistake=None, paths=None):
    """What k_tracer_finish leaves in `parent` (a copy) after storing `interior`: every cell's point and images, in any order (no two
    cells write one element with different values).  mistake: one of MISTAKES --
      halos_transposed         Hx and Hy swapped in the image rule (the addresses stay right)
      second_x_image_dropped   a cell with an image on both x sides stores only the low one (second_y likewise)
      corner_dropped           the y images of a cell's x images are not stored
      pair_without_images      the wide store taken on the alignment alone: the pairs `paths` names SCALAR_IMAGES store no image"""
    a = np.array(parent, dtype=np.float64, copy=True)
    assert a.shape == (Ny + 2 * Hy, Nx + 2 * Hx) and interior.shape == (Ny, Nx)
    mx, my = _modes(topo[0]), _modes(topo[1])
    rx, ry = (Hy, Hx) if mistake == "halos_transposed" else (Hx, Hy)          # the widths the RULE uses

    def put(i, j, v):
        jj, ii = j + Hy - 1, i + Hx - 1
        if 0 <= jj < a.shape[0] and 0 <= ii < a.shape[1]:      # (a transposed rule may aim beyond the parent: the test only needs a difference)
            a[jj, ii] = v
    for j in range(1, Ny + 1):
        for i in range(1, Nx + 1):
            v = interior[j - 1, i - 1]
            put(i, j, v)
            if mistake == "pair_without_images" and paths[j - 1][(i - 1) // PAIR] == SCALAR_IMAGES:
                continue
            if not has_halo_images(i, j, Nx, Ny, rx, ry, my[1] == "fold"):
                continue
            if my[1] == "fold":
                jt = 2 * Ny - j
                if Ny < jt <= Ny + ry:
                    it = Nx - i + 1
                    put(it, jt, v)
                    if it <= rx:
                        put(it + Nx, jt, v)
                    if it > Nx - rx:
                        put(it - Nx, jt, v)
            (hxl, xl), (hxh, xh) = _lo(mx[0], i, Nx, rx), _hi(mx[1], i, Nx, rx)
            (hyl, yl), (hyh, yh) = _lo(my[0], j, Ny, ry), _hi(my[1], j, Ny, ry)
            if mistake == "second_x_image_dropped" and hxl and hxh:
                hxh = False
            if mistake == "second_y_image_dropped" and hyl and hyh:
                hyh = False
            if hxl:
                put(xl, j, v)
            if hxh:
                put(xh, j, v)
            for has, y in ((hyl, yl), (hyh, yh)):
                if has:
                    put(i, y, v)
                    if mistake != "corner_dropped":
                        if hxl:
                            put(xl, y, v)
                        if hxh:
                            put(xh, y, v)
    return a


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# metric: 0 rectilinear, 1 latitude-longitude, 2 curvilinear (tests/test_gpu_tracers.py METRICS); land: hand-placed land and an open-water
# patch (flow_case) where the grid can hold them; group: what the row is in the table for
Case = namedtuple("Case", "id Nx Ny halo topo scheme metric land group")
LAND_MIN = (9, 6)              # flow_case's land: a 3 x 5 block, cells on the first and last column and row


def _rows():
    r = []

    def add(group, Nx, Ny, halo, scheme, topo=None):
        n = len(r)
        t = topo or ("pp", "bb", "pb", "bp")[n % 4]
        r.append(Case(f"{group}-{Nx}x{Ny}-H{halo[0]}{halo[1]}-{t}-s{scheme}", Nx, Ny, halo, t, scheme, 2 if t == "pf" else n % 3,
                      Nx >= LAND_MIN[0] and Ny >= LAND_MIN[1] and t != "pf", group))
    add("baseline", 37, 29, (4, 4), 7)
    add("baseline", 128, 24, (4, 4), 7, "bp")
    # unequal and odd halos: odd Hx with even Nx (no pair of c aligned in any row), odd Hx with odd Nx, odd Nx with odd Ny (plane odd)
    for halo in ((5, 4), (6, 4), (4, 6), (5, 5)):
        add("halo", 40, 28, halo, 7)
        add("halo", 29, 41, halo, 5)
    add("halo", 40, 28, (3, 2), 3)
    add("halo", 29, 41, (3, 2), -3)
    add("halo", 40, 28, (2, 3), -3)
    add("halo", 29, 41, (2, 3), 3)
    add("halo", 38, 27, (1, 1), 1)
    # narrow in x, ordinary in y: N in {H, H + 1, 2H - 1, 2H, 2H + 1}
    for halo, scheme in (((4, 4), 7), ((3, 2), 3)):
        Hx = halo[0]
        for Nx in (Hx, Hx + 1, 2 * Hx - 1, 2 * Hx, 2 * Hx + 1):
            add("narrow_x", Nx, 41, halo, scheme)
    for Nx in (6, 11, 13):
        add("narrow_x", Nx, 40, (6, 4), 5)
    # narrow in y, ordinary in x
    for halo, scheme in (((4, 4), 7), ((4, 6), 5)):
        Hy = halo[1]
        for Ny in (Hy, Hy + 1, 2 * Hy - 1, 2 * Hy, 2 * Hy + 1):
            add("narrow_y", 40 if Ny % 2 else 39, Ny, halo, scheme)
    # narrow in both
    add("narrow_xy", 4, 4, (4, 4), 7)
    add("narrow_xy", 5, 9, (4, 4), 7)
    add("narrow_xy", 9, 5, (6, 4), 7)
    add("narrow_xy", 7, 7, (4, 4), 5)
    add("narrow_xy", 8, 8, (4, 4), -5)
    add("narrow_xy", 3, 2, (3, 2), 3)
    add("narrow_xy", 2, 5, (2, 3), -3)
    for t in ("pp", "bb", "pb"):
        add("narrow_xy", 1, 1, (1, 1), 1, t)
    # the 63 x 7 stencil tile's edges
    add("tile", 62, 6, (4, 4), 7)
    add("tile", 63, 7, (5, 4), 7)
    add("tile", 64, 8, (4, 4), 5)
    add("tile", 126, 21, (4, 6), 7)
    add("tile", 127, 22, (4, 4), -5)
    # the 128 x 4 finish block's edges (Ny < 4: a halo that narrow)
    add("finish", 127, 3, (3, 2), 3)
    add("finish", 128, 4, (3, 2), -3)
    add("finish", 129, 5, (2, 3), 3)
    # the north fold with Hx != Hy, curvilinear and masked
    add("fold", 40, 28, (6, 4), 7, "pf")
    add("fold", 40, 28, (4, 6), 5, "pf")
    return tuple(r)


CASES = _rows()
BY_ID = {c.id: c for c in CASES}


def build(case, seed=5):
    """The inputs of a row: tests/test_gpu_tracers.py flow_case with the row's halo.  Where the grid is too small for flow_case's
    open-water patch (two rows of six cells from the middle on: all of a 1 x 1 grid) the concentration is drawn again over the wet
    cells with ONE open-water cell; the fold rows take the mirror-symmetric seeded land of cases.make_case, as
    test_masked_north_fold_against_the_oracles_snow_thickness does."""
    import cases
    from test_gpu_tracers import flow_case
    Nx, Ny, topo = case.Nx, case.Ny, TOPOS[case.topo]
    if case.topo == "pf":
        c = flow_case(Nx, Ny, topo, 0, land=False, seed=seed, H=case.halo, curvilinear=0.04)
        c2 = cases.make_case(Nx=Nx, Ny=Ny, H=case.halo, topo=topo, spacing=1000.0, patches=False, noise=0.0, land=0.2, curvilinear=0.04,
                             top=None, bottom=None, coriolis=None)
        wet = c2["mask"].astype(bool)
        return dict(c, g=c2["g"], mask=c2["mask"], a=np.where(wet, c["a"], 0.0), h=np.where(wet, c["h"], 0.0),
                    values=[np.where(wet, v, 0.0) for v in c["values"]])
    c = flow_case(Nx, Ny, topo, case.metric, land=case.land, seed=seed, H=case.halo)
    if Nx < 12 or Ny < 4:
        rng = np.random.default_rng(seed + 100)
        wet = np.ones((Ny, Nx), bool) if c["mask"] is None else c["mask"].astype(bool)
        a = np.where(wet, 0.2 + 0.7 * rng.random((Ny, Nx)), 0.0)
        if Nx * Ny >= 6:
            a[Ny // 2, Nx // 2] = 0.0
        c["a"] = a
        c["h"] = np.where(a > 0, 0.3 + 0.2 * rng.random((Ny, Nx)), 0.0)
    return c


def no_wide_store(c):
    """every pair of the grid holds a cell with an image: Nx <= 2 Hx + 1 (the one column beyond both halos pairs with one inside), or
    every row within Hy of an edge"""
    return c.Nx <= 2 * c.halo[0] + 1 or c.Ny <= 2 * c.halo[1] + (1 if c.topo == "pf" else 0)


def narrow(c):
    return c.Nx <= 2 * c.halo[0] + 1 or c.Ny <= 2 * c.halo[1] + 1


def unequal(c):
    return c.halo[0] != c.halo[1]


# ---- the edge values of the point-wise halves (tests/test_gpu_tracer_branches.py) ----------------------------------------------------------------
# 37 x 5 cells, periodic, zero velocities.  Cell n = (i - 1) + 37 (j - 1) has kind n % 96 -- (aice^-, Ga) by kind % 8, the second half's
# aice by (kind // 8) % 6, immersed where kind >= 48 -- and in round r the base value BRANCH_C[(n + r) % 12]: twelve rounds put every value
# in every kind of cell (96 and 37 - 1 are multiples of 12).  0 * Inf is NaN, so a non-finite value makes the upwind fluxes of its own
# faces NaN, and with them G of its west and south neighbours: the non-finite values sit together at the end of BRANCH_C and the value
# before them is a repeated one, as is the (aice^-, Ga) pair before the NaN one (which is NaN through Ga, so that aice * c stays finite).
BRANCH_GRID = (37, 5)
BRANCH_DT = 2.0
BRANCH_C = (1.5, -1.5, 0.0, -0.0, 5e-324, 1e300, 1.5, -1.5, 0.0, np.inf, -np.inf, np.nan)
BRANCH_C_DISTINCT = 9
# (aice^-, Ga) -> aice* = aice^- + 2 Ga: ordinary, above 1, +0.0, -0.0, negative, subnormal, ordinary again, NaN
BRANCH_ASTAR = ((0.5, 0.05), (0.9, 0.1), (0.5, -0.25), (-0.0, -0.0), (0.5, -0.5), (5e-324, 0.0), (0.25, 0.125), (0.5, np.nan))
BRANCH_ANOW = (0.5, 0.0, -0.0, 5e-324, -0.1, np.nan)
BRANCH_TRACERS = tuple((nn, src) for nn in (1, 0) for src in (0.0, 2.0, -2e-3))      # (nonnegative, source), plain or weighted: one model each
BRANCH_ROUNDS = 12


def branch_round(r, shift=0):
    """(c^-, aice^-, Ga, aice of the second half, active) as (5, 37) interiors for round r; shift moves the kinds (a second RK3 stage)"""
    Nx, Ny = BRANCH_GRID
    n = np.arange(Nx * Ny).reshape(Ny, Nx)
    kind = (n + shift) % 96
    pair = np.array(BRANCH_ASTAR)[kind % 8]
    return (np.array(BRANCH_C)[(n + r) % 12], np.ascontiguousarray(pair[..., 0]), np.ascontiguousarray(pair[..., 1]),
            np.array(BRANCH_ANOW)[(kind // 8) % 6], kind < 48)


def branch_combinations(rounds=BRANCH_ROUNDS):
    """the set of (bits of c^-, bits of aice*, bits of the second half's aice, active) the rounds hold (any NaN counts as one value)"""
    def key(x):
        return "nan" if np.isnan(x) else int(np.float64(x).view(np.uint64))
    seen = set()
    for r in range(rounds):
        c, ab, Ga, an, act = branch_round(r)
        with np.errstate(invalid="ignore"):
            astar = ab + BRANCH_DT * Ga
        seen |= {(key(a), key(b), key(d), bool(e)) for a, b, d, e in zip(c.ravel(), astar.ravel(), an.ravel(), act.ravel())}
    return seen
