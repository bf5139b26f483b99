"""The table of tests/tracer_cases.py, checked without a GPU: its constants are the ones csrc/tracers.hip and csrc/csi_dev.h state, its
cases reach every store path of k_tracer_finish and every image combination of store_with_images that has both sides of a direction,
and the comparisons the GPU matrix makes (whole parents, bit for bit) can fail: each image mistake changes the expected parent."""
import os
import re

import numpy as np
import pytest

import halo_ref
import tracer_cases as tc
import tracers_ref as tr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "climaseaice.jl_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- the constants, against the source text ----------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    t, d, h, x = _text("tracers.hip"), _text("csi_dev.h"), _text("csi_tracers.hip"), _text("csi_ctx.h")
    m = re.search(r"constexpr int TTX = (\d+), TTY = (\d+);", t)
    assert (int(m.group(1)), int(m.group(2))) == tc.TILE
    assert "dim3 b(trc::TTX + 1, trc::TTY + 1, 1);" in t and "(T.g.Nx + trc::TTX - 1) / trc::TTX" in t and "(T.g.Ny + trc::TTY - 1) / trc::TTY" in t
    # the pair: two cells per thread from an odd i
    m = re.search(r"const int i = 1 \+ (\d+) \* \(int\)\(blockIdx\.x \* blockDim\.x \+ threadIdx\.x\), j = 1 \+ blockIdx\.y \* blockDim\.y \+ threadIdx\.y, k = blockIdx\.z;", t)
    assert int(m.group(1)) == tc.PAIR == 2 and "const bool two = i + 1 <= g.Nx;" in t
    # the finish block: 64 threads x 2 cells, 4 rows
    m = re.search(r"void launch_tracers_finish\(const TracersDev& T, hipStream_t s\) \{\s*dim3 b\((\d+), (\d+)\);\s*hipLaunchKernelGGL\(trc::k_tracer_finish, "
                  r"dim3\(\(unsigned\)\(\(T\.g\.Nx \+ (\d+)\) / (\d+)\), \(unsigned\)\(\(T\.g\.Ny \+ (\d+)\) / (\d+)\), \(unsigned\)T\.n\)", t)
    bx, by, rx, dx, ry, dy = (int(v) for v in m.groups())
    assert (bx * tc.PAIR, by) == tc.FINISH_BLOCK == (dx, dy) and (rx, ry) == (dx - 1, dy - 1)
    # the store choice and the aice pair
    m = re.search(r"if \(two && \(\(\(uintptr_t\)cp \| \(uintptr_t\)fp\) & (\d+)\) == 0 && !has_halo_images\(g, T\.im, i, j\) && !has_halo_images\(g, T\.im, i \+ 1, j\)\) \{", t)
    assert int(m.group(1)) == tc.ALIGN_MASK
    m = re.search(r"if \(two && \(\(uintptr_t\)ap & (\d+)\) == 0\) \{ const double2 a", t)
    assert int(m.group(1)) == tc.ALIGN_MASK
    assert "double* cp = T.c[k] + i + (long)j * T.ld;" in t
    assert "double* fp = T.cfree[k] ? T.cfree[k] + i + (long)j * T.ld : nullptr;" in t
    # the rule of has_halo_images
    assert "const bool in_x = (i >= 1) & (i <= g.Nx), in_y = (j >= 1) & (j <= g.Ny);" in d
    assert "const bool near_x = in_x & ((i <= g.Hx) | (i > g.Nx - g.Hx));" in d
    assert "const bool near_y = in_y & ((j <= g.Hy) | (j > g.Ny - g.Hy - (im.yhi == IMG_FOLD ? 1 : 0)));" in d
    assert "return near_x | near_y;" in d
    # the geometry: the origin of a parent, the plane of the free copy, when a tracer has one
    assert "return parent + (c->Hx - 1) + (int64_t)(c->Hy - 1) * ld; }" in x
    assert "const size_t plane = (size_t)R.shape.ld * (size_t)R.shape.nj;" in h
    assert "double* fr = sourced ? origin_of(c, R.free_.get() + (size_t)k * plane, R.shape.ld) : nullptr;" in h
    assert "const bool sourced = R.t.source[k] != 0.0 && R.free_;" in h and "T.cfree[k] = R.star_from_cache ? fr : nullptr;" in h


def test_the_rule_by_hand():
    """a few pairs worked out on paper"""
    # 8 x 9, halo (4, 4): ld = 16, element (1, 1) at 4 + 4 * 16 = 68 doubles: aligned in every row; rows 5 is the only one without y images,
    # and no column is without x images
    f = tc.finish_path(8, 9, 4, 4, ("periodic", "periodic"))
    assert all(p == tc.SCALAR_IMAGES for row in f.paths for p in row) and all(all(r) for r in f.aice_pair)
    # 10 x 9: columns 5, 6 of row 5 have no image -- the one wide store
    f = tc.finish_path(10, 9, 4, 4, ("periodic", "periodic"))
    assert [(j + 1, 1 + 2 * p) for j, row in enumerate(f.paths) for p, v in enumerate(row) if v == tc.WIDE_C] == [(5, 5)]
    # ... below a fold row Ny - Hy has images too
    assert tc.path_counts(10, 9, 4, 4, ("periodic", "folded"))[tc.WIDE_C] == 0
    # odd Hx, even Nx: ld even, element (1, j) at an odd offset in every row: no pair of c is aligned; one double behind a boundary, all
    f = tc.finish_path(40, 28, 5, 4, ("periodic", "periodic"))
    assert all(p == tc.SCALAR_C for row in f.paths for p in row) and not any(any(r) for r in f.aice_pair)
    assert tc.path_counts(40, 28, 5, 4, ("periodic", "periodic"), c_offset_doubles=1)[tc.SCALAR_C] == 0
    # odd Nx: alternating rows; the last cell alone
    f = tc.finish_path(37, 29, 4, 4, ("periodic", "periodic"))
    assert [row[8] for row in f.paths[4:8]] == [tc.WIDE_C, tc.SCALAR_C, tc.WIDE_C, tc.SCALAR_C] and all(row[-1] == tc.LONE for row in f.paths)
    # odd Nx and odd Ny: plane odd, so the free copy of an odd-numbered tracer has the other alignment
    assert (37 + 8) * (29 + 8) % 2 == 1
    g = tc.finish_path(37, 29, 4, 4, ("periodic", "periodic"), k=1, sourced=True, rk=True)
    assert [row[8] for row in g.paths[4:8]] == [tc.SCALAR_FREE, tc.SCALAR_C, tc.SCALAR_FREE, tc.SCALAR_C]
    g = tc.finish_path(37, 29, 4, 4, ("periodic", "periodic"), k=2, sourced=True, rk=True)
    assert [row[8] for row in g.paths[4:8]] == [tc.WIDE_C_FREE, tc.SCALAR_C, tc.WIDE_C_FREE, tc.SCALAR_C]
    # no free copy without a source, or outside an RK3 stage
    assert tc.finish_path(37, 29, 4, 4, ("periodic", "periodic"), k=1, sourced=False, rk=True).paths == f.paths
    assert tc.finish_path(37, 29, 4, 4, ("periodic", "periodic"), k=1, sourced=True, rk=False).paths == f.paths


# ---- what the table covers ---------------------------------------------------------------------------------------------------------------------
# pairs by path class over CASES x tracers 0..7 (tests/test_gpu_tracers.py SPECS8) x {ForwardEuler, an RK3 stage}: README.md and
# profiles/r32_tracer_coverage.md quote these


def table_counts():
    total = dict.fromkeys(tc.PATHS, 0)
    for c in tc.CASES:
        for k in range(8):
            for rk in (False, True):
                for p, n in tc.path_counts(c.Nx, c.Ny, *c.halo, tc.TOPOS[c.topo], k=k, sourced=tc.SOURCED8[k], rk=rk).items():
                    total[p] += n
    return total


def test_what_the_issue_asks_of_the_table():
    C = tc.CASES
    assert len(C) == len({c.id for c in C}) == 58
    assert max(c.Nx for c in C) <= 130 and max(c.Ny for c in C) <= 45
    halos = {c.halo for c in C}
    assert {(4, 4), (5, 4), (6, 4), (4, 6), (5, 5), (3, 2), (2, 3), (1, 1)} <= halos
    for halo, schemes in (((5, 4), {7, 5}), ((6, 4), {7, 5}), ((4, 6), {7, 5}), ((5, 5), {7, 5}), ((3, 2), {3, -3}), ((2, 3), {3, -3}), ((1, 1), {1})):
        assert schemes <= {c.scheme for c in C if c.halo == halo}, halo
    need = {7: 4, 5: 3, -5: 3, 3: 2, -3: 2, 1: 1}
    assert all(min(c.halo) >= need[c.scheme] for c in C)
    assert {c.scheme for c in C} == set(need)
    # widths and heights with images on both sides, narrow in one direction (the other about 40) and in both; 1 x 1
    for Hx in (4, 3):
        assert {Hx, Hx + 1, 2 * Hx - 1, 2 * Hx, 2 * Hx + 1} <= {c.Nx for c in C if c.halo[0] == Hx and c.group == "narrow_x" and c.Ny >= 40}
    for Hy in (4, 6):
        assert {Hy, Hy + 1, 2 * Hy - 1, 2 * Hy, 2 * Hy + 1} <= {c.Ny for c in C if c.halo[1] == Hy and c.group == "narrow_y" and c.Nx >= 39}
    both = [c for c in C if c.Nx <= 2 * c.halo[0] + 1 and c.Ny <= 2 * c.halo[1] + 1]
    assert {(c.Nx, c.Ny, c.halo) for c in both} >= {(4, 4, (4, 4)), (5, 9, (4, 4)), (9, 5, (6, 4)), (3, 2, (3, 2)), (2, 5, (2, 3)), (1, 1, (1, 1))}
    assert all(c.Nx >= c.halo[0] and c.Ny >= c.halo[1] + (1 if c.topo == "pf" else 0) for c in C)      # fill_width_check accepts every row
    # the stencil tile's and the finish block's edges
    assert {62, 63, 64, 126, 127} <= {c.Nx for c in C} and {6, 7, 8, 21, 22} <= {c.Ny for c in C}
    assert {127, 128, 129} <= {c.Nx for c in C} and {3, 4, 5} <= {c.Ny for c in C}
    assert any(c.Nx < tc.TILE[0] and c.Ny < tc.TILE[1] for c in C)
    assert any(c.Nx % tc.TILE[0] == 0 and c.Ny % tc.TILE[1] == 0 for c in C) and any(c.Nx % tc.TILE[0] == 1 for c in C) and any(c.Ny % tc.TILE[1] == 1 for c in C)
    # alignment classes
    assert any(c.halo[0] % 2 and c.Nx % 2 == 0 for c in C) and any(c.halo[0] % 2 and c.Nx % 2 for c in C)
    assert any(((c.Nx + 2 * c.halo[0]) * (c.Ny + 2 * c.halo[1])) % 2 for c in C)
    # topologies, metric kinds, land
    assert {c.topo for c in C} == {"pp", "bb", "pb", "bp", "pf"}
    assert all(c.halo[0] != c.halo[1] and c.metric == 2 for c in C if c.topo == "pf") and sum(c.topo == "pf" for c in C) == 2
    for t in ("pp", "bb", "pb", "bp"):
        assert {c.metric for c in C if c.topo == t} == {0, 1, 2}, t
    assert all(c.land == (c.Nx >= 9 and c.Ny >= 6 and c.topo != "pf") for c in C) and sum(c.land for c in C) > 20


def test_every_store_path_occurs_and_narrow_grids_take_no_wide_store():
    total = table_counts()
    print("pairs by path class:", total)
    assert all(total[p] > 0 for p in tc.PATHS), total
    assert total[tc.WIDE_C] > 0 and total[tc.WIDE_C_FREE] > 0
    assert total == {tc.WIDE_C: 49577, tc.WIDE_C_FREE: 19136, tc.SCALAR_C: 105600, tc.SCALAR_FREE: 7857, tc.SCALAR_IMAGES: 105350, tc.LONE: 11104}, total
    narrow = [c for c in tc.CASES if tc.narrow(c)]
    assert len(narrow) >= 30
    for c in narrow:
        for k in range(8):
            for rk in (False, True):
                for off in (0, 1):
                    f = tc.finish_path(c.Nx, c.Ny, *c.halo, tc.TOPOS[c.topo], c_offset_doubles=off, k=k, sourced=tc.SOURCED8[k], rk=rk)
                    wide_rows = {j + 1 for j, row in enumerate(f.paths) if any(p in tc.WIDE for p in row)}
                    if tc.no_wide_store(c):
                        assert not wide_rows, (c.id, k, rk, off)
                    else:              # Ny == 2 Hy + 1: the middle row alone
                        assert wide_rows <= {c.halo[1] + 1}, (c.id, k, rk, off, wide_rows)
    # both aice loads occur, and a pair of aice next to scalar stores of c (a free copy of the other alignment)
    seen = set()
    for c in tc.CASES:
        for k in (0, 1):
            f = tc.finish_path(c.Nx, c.Ny, *c.halo, tc.TOPOS[c.topo], k=k, sourced=tc.SOURCED8[k], rk=True)
            seen |= {(a, p) for ar, pr in zip(f.aice_pair, f.paths) for a, p in zip(ar, pr)}
    assert {(True, tc.WIDE_C), (True, tc.WIDE_C_FREE), (True, tc.SCALAR_FREE), (True, tc.SCALAR_IMAGES), (False, tc.SCALAR_C), (False, tc.LONE)} <= seen


def test_every_image_combination_with_both_sides_of_a_direction_occurs():
    """(hxl, hxh, hyl, hyh) of store_with_images: four combinations with both x images and four with both y images; all four images
    belongs to both, so seven different ones"""
    want = {(1, 1, a, b) for a in (0, 1) for b in (0, 1)} | {(a, b, 1, 1) for a in (0, 1) for b in (0, 1)}
    assert len(want) == 7
    seen = {}
    for c in tc.CASES:
        for j in range(1, c.Ny + 1):
            for i in range(1, c.Nx + 1):
                fl = tuple(int(v) for v in tc.image_flags(i, j, c.Nx, c.Ny, *c.halo, tc.TOPOS[c.topo]))
                seen.setdefault(fl, c.id)
                # the rule of has_halo_images covers the images: no image without it (it is wider only below a fold)
                assert not any(fl) or tc.has_halo_images(i, j, c.Nx, c.Ny, *c.halo, c.topo == "pf")
    assert want <= set(seen), want - set(seen)
    assert len(seen) == 16          # and every other combination as well


# ---- the comparisons can fail ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fe_steps(oracle_lib):
    """one ForwardEuler step of a plain tracer on every narrow or unequal-halo case: (case, parent before, parent after)"""
    from test_gpu_tracers import ref_of, specs_of
    out = []
    for c in tc.CASES:
        if tc.narrow(c) or tc.unequal(c):
            case = tc.build(c)
            p, ts = ref_of(case, specs_of(1))
            before = ts[0]["c"].copy()
            tr.step_fe(p, ts, case["dt"], c.scheme, True)
            out.append((c, before, ts[0]["c"].copy()))
    return out


def applicable(c, mistake):
    """whether the rule says the mistake touches any cell of the case"""
    cells = [tc.image_flags(i, j, c.Nx, c.Ny, *c.halo, tc.TOPOS[c.topo]) for j in range(1, c.Ny + 1) for i in range(1, c.Nx + 1)]
    if mistake == "halos_transposed":
        return tc.unequal(c)
    if mistake == "second_x_image_dropped":
        return any(f[0] and f[1] for f in cells)
    if mistake == "second_y_image_dropped":
        return any(f[2] and f[3] for f in cells)
    if mistake == "corner_dropped":
        return any((f[0] or f[1]) and (f[2] or f[3]) for f in cells)
    return tc.path_counts(c.Nx, c.Ny, *c.halo, tc.TOPOS[c.topo])[tc.SCALAR_IMAGES] > 0


def test_image_mistakes_change_the_expected_parent(fe_steps):
    """The scatter form of tests/tracer_cases.py reproduces the oracle's parent and the gather form of tests/halo_ref.py; with a mistake
    switched on at least one parent element differs, in EVERY case the mistake can touch: Hx and Hy transposed in every unequal-halo
    case, the second x (y) image dropped wherever a cell has both, the corner dropped and a pair stored without its images wherever the
    rule names such a cell or pair.  (A transposition with Hx == Hy, or a second image where no cell has two, is no mistake at all: the
    condition is stated per mistake, from the rule, before any value is looked at.)"""
    assert len(fe_steps) >= 40
    letters = {"periodic": "P", "bounded": "B", "folded": "F"}
    hit = dict.fromkeys(tc.MISTAKES, 0)
    for c, before, after in fe_steps:
        topo = tc.TOPOS[c.topo]
        Hx, Hy = c.halo
        inner = after[Hy:Hy + c.Ny, Hx:Hx + c.Nx]
        assert not np.array_equal(inner, before[Hy:Hy + c.Ny, Hx:Hx + c.Nx]) or c.Nx * c.Ny == 1, c.id
        right = tc.store_parent(before, inner, c.Nx, c.Ny, Hx, Hy, topo)
        assert tr.same_bits(right, after), (c.id, np.argwhere(right != after)[:4])
        gathered, cls = halo_ref.fill(right, c.Nx, c.Ny, Hx, Hy, (halo_ref.CENTER, halo_ref.CENTER), letters[topo[0]] + letters[topo[1]])
        assert tr.same_bits(gathered, after) and not np.any(cls == halo_ref.CORNER_UNSPECIFIED), c.id
        paths = tc.finish_path(c.Nx, c.Ny, Hx, Hy, topo).paths
        can = [m for m in tc.MISTAKES if applicable(c, m)]
        if c.Nx * c.Ny == 1:
            continue                      # (G == 0: the one cell keeps its value, and so does every image of it)
        # the conditions, from the rule alone
        assert "corner_dropped" in can and len(can) >= 2, (c.id, can)
        assert ("halos_transposed" in can) == tc.unequal(c)
        assert ("second_x_image_dropped" in can) == (c.Nx < 2 * Hx) and ("second_y_image_dropped" in can) == (c.Ny < 2 * Hy and c.topo != "pf")
        assert ("pair_without_images" in can) == (c.Nx >= 2 and not (Hx % 2 == 1 and c.Nx % 2 == 0))
        for m in can:
            wrong = tc.store_parent(before, inner, c.Nx, c.Ny, Hx, Hy, topo, mistake=m, paths=paths)
            n = int(np.sum(~halo_ref.same_bits(wrong, after)))
            assert n > 0, (c.id, m)
            hit[m] += 1
    print("cases in which each mistake shows:", hit)
    assert all(n >= 5 for n in hit.values()), hit


# ---- Julia's max ---------------------------------------------------------------------------------------------------------------------------------
def test_jmax_table():
    bits = lambda v: np.float64(v).view(np.uint64)      # noqa: E731
    assert bits(tr.jmax(0.0, -0.0)) == bits(0.0) and not np.signbit(tr.jmax(0.0, -0.0))
    assert bits(tr.jmax(0.0, 0.0)) == bits(0.0)
    assert np.isnan(tr.jmax(0.0, np.nan)) and np.isnan(tr.jmax(np.nan, 1.0))
    for x in (5e-324, 1e-300, 1.5, 1e300):
        assert bits(tr.jmax(0.0, -x)) == bits(0.0) and bits(tr.jmax(0.0, x)) == bits(x)
    assert tr.jmax(0.0, np.inf) == np.inf and bits(tr.jmax(0.0, -np.inf)) == bits(0.0)
    # element-wise, and what it replaced: the two agree everywhere but on the sign of a zero
    x = np.array([-0.0, 0.0, -1.0, 2.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324])
    got = tr.jmax(0.0, x)
    assert tr.same_bits(got, np.array([0.0, 0.0, 0.0, 2.0, np.nan, np.inf, 0.0, 5e-324, 0.0]))
    assert np.array_equal(got, np.maximum(0.0, x), equal_nan=True)
    # the halves use it: a clipped -0.0 leaves +0.0 in c and in the source-free copy
    act = np.ones(3, bool)
    star = np.array([-0.0, -1.0, 0.25])
    assert tr.same_bits(tr.second_half(star, np.ones(3), act, 2.0, True, 0.0), np.array([0.0, 0.0, 0.25]))
    assert tr.same_bits(tr.free_half(star, np.ones(3), act, True), np.array([0.0, 0.0, 0.25]))
    assert tr.same_bits(tr.free_half(star, np.ones(3), act, False), np.array([-0.0, -1.0, 0.25]))            # unclipped: the zero keeps its sign
    assert tr.same_bits(tr.second_half(star, np.ones(3), act, 2.0, False, 0.0), np.array([0.0, -1.0, 0.25]))     # ... until -0.0 + dt * 0.0
    assert not tr.same_bits(np.array([-0.0]), np.array([0.0])) and tr.same_bits(np.array([np.nan, -0.0]), np.array([-np.nan, -0.0]))
