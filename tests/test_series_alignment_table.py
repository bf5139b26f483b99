"""The table of tests/series_alignment_cases.py, checked without a GPU: its block constants and its alignment class are the ones the
sources state, and the cases of tests/test_gpu_series_alignment.py reach every alignment class, shape edge and source alignment that
k_time_series and k_time_series_regrid decide their control flow from.  Nothing is omitted silently: the cases are counted."""
import os
import re

import pytest

import series_alignment_cases as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "climaseaice.jl_amd", "csrc")
CLASSES = {0, 1, 2, 3}


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def slots(kernel=None, backend=None, route=None):
    for c in T.CASES:
        if (kernel is None or c.kernel == kernel) and (backend is None or c.backend == backend) and (route is None or c.route == route):
            for s in c.slots:
                yield c, s


@pytest.mark.parametrize("unit", ["time_series.hip", "time_series_regrid.hip"])
def test_block_constants_and_guards_are_the_sources(unit):
    text = _text(unit)
    assert "constexpr int kRows = 2;" in text and "constexpr int kBx = 64, kBy = 4;" in text
    assert (T.BLOCK_X, T.BLOCK_Y, T.ROW_STEP) == (2 * 64, 4 * 2, 4)
    # what the cases with an even nx and a row that starts odd are for: the guard and the grid size leave room for one pair more
    assert "if (2 * pair - 1 >= D.nx || jb >= D.ny) return;" in text
    assert "const int pairs = nx / 2 + 1;" in text
    assert "const int head = (int)((reinterpret_cast<uintptr_t>(D.dst + jj * D.ldd) >> 3) & 1);" in text


def test_alignment_class_is_regrid_variant():
    text = _text("csi_time_series.hip")
    assert "return (int)((((uintptr_t)dst) >> 3) & 1) * 2 + (int)(ld & 1);" in text
    assert "const int head = ((variant >> 1) + (variant & 1) * j) & 1;" in text
    assert "S.ring_off = (like && ((((uintptr_t)like) ^ ((uintptr_t)S.ring.get())) & 15)) ? 1 : 0;" in text
    # the restatement from (base offset, halo, ld) equals the one from the address, for a base on or one double behind a boundary
    for c, s in slots():
        nj, ni, ld = T.parent(c, s)
        for boundary in (0, 256, 4096 + 16):
            address = boundary + 8 * T.first_offset(c, s)
            assert T.class_of_address(address, ld) == T.alignment_class(c, s)
        heads = T.row_heads(c, s)
        v = T.alignment_class(c, s)
        assert heads == [((v >> 1) + (v & 1) * j) & 1 for j in range(len(heads))]      # map_upload's row rule
        assert s.base_off in (0, 1) and s.ld_extra in (0, 1) and ld >= ni


def test_the_cases_are_counted():
    """(two kernels x two backends) x ten layouts + the shared-map case per backend; every id is one case"""
    assert len(T.LAYOUTS) == 10 and len(T.CASES) == 2 * 2 * 10 + 2 == 42
    assert len({c.id for c in T.CASES}) == len(T.CASES)
    for c in T.CASES:
        assert c.kernel in T.KERNELS and c.backend in T.BACKENDS and c.route in ("halo", "hand") and c.halo in T.HALOS
        assert (c.route == "halo") == all(s.base_off == 0 and s.ld_extra == 0 for s in c.slots) or c.shared
        assert all(T.SLOT_LOC[s.name] == s.loc for s in c.slots) and len({s.name for s in c.slots}) == len(c.slots)
    assert {c.halo for c in T.CASES if c.route == "halo"} == set(T.HALOS)
    assert {(s.base_off, s.ld_extra) for c, s in slots(route="hand") if not c.shared} == {(1, 0), (1, 1)}


def test_shapes_are_the_short_list():
    used = {(c.Nx, c.Ny) for c in T.CASES}
    assert used == set(T.SHAPES) and 8 <= len(T.SHAPES) <= 9
    assert {nx for nx, _ in T.SHAPES} == set(T.NXS) and {ny for _, ny in T.SHAPES} == set(T.NYS)
    # one pair, one block of columns less / exactly / more, more than two blocks; a block of rows, one row more
    assert T.BLOCK_X - 1 in T.NXS and T.BLOCK_X in T.NXS and T.BLOCK_X + 1 in T.NXS and 2 * T.BLOCK_X + 1 in T.NXS
    assert T.BLOCK_Y in T.NYS and T.BLOCK_Y + 1 in T.NYS


@pytest.mark.parametrize("backend", T.BACKENDS)
@pytest.mark.parametrize("kernel", T.KERNELS)
def test_every_class_at_every_location(kernel, backend):
    for loc in T.LOCS:
        got = {T.alignment_class(c, s) for c, s in slots(kernel, backend) if s.loc == loc}
        assert got == CLASSES, (kernel, backend, loc, got)


def test_every_class_through_a_halo_and_through_a_hand_bound_array():
    for kernel in T.KERNELS:
        for backend in T.BACKENDS:
            for route in ("halo", "hand"):
                got = {T.alignment_class(c, s) for c, s in slots(kernel, backend, route)}
                assert got == CLASSES, (kernel, backend, route, got)
    # the halo (4, 4) of every other test of the two kernels reaches classes 0 and 1 only
    assert {T.alignment_class(c, s) for c, s in slots(route="halo") if c.halo == (4, 4)} == {0, 1}


@pytest.mark.parametrize("kernel", T.KERNELS)
def test_rows_that_start_odd_with_an_even_width(kernel):
    """the cases in which `2 * pair >= nx` or a grid of (nx + 1) / 2 pairs drops the last column"""
    for backend in T.BACKENDS:
        got = {T.interior(c, s)[1] for c, s in slots(kernel, backend) if 1 in T.row_heads(c, s) and T.interior(c, s)[1] % 2 == 0}
        assert {2, 128, 256} <= got, (kernel, backend, got)
        # ... where the last pair is the first one of a further block of columns
        assert any(T.interior(c, s)[1] in (128, 256) and all(T.row_heads(c, s)) for c, s in slots(kernel, backend))


@pytest.mark.parametrize("kernel", T.KERNELS)
def test_row_counts_without_and_with_a_second_row(kernel):
    nys = {T.interior(c, s)[0] for c, s in slots(kernel)}
    assert any(ny < T.ROW_STEP for ny in nys) and any(T.ROW_STEP < ny < T.BLOCK_Y for ny in nys)
    assert any(ny == T.BLOCK_Y for ny in nys) and any(ny > T.BLOCK_Y for ny in nys)      # exactly one block of rows, two


def test_one_launch_carries_three_interior_shapes():
    for c in T.CASES:
        if not c.shared:
            shapes = {T.interior(c, s) for s in c.slots}
            assert len(shapes) == 3, c.id
            # the launch is sized by the largest: some slot is narrower, another one shorter
            ny, nx = max(s[0] for s in shapes), max(s[1] for s in shapes)
            assert any(s[1] < nx for s in shapes) and any(s[0] < ny for s in shapes)
    # surplus BLOCKS, not only surplus threads: a slot one block of columns narrower, a slot one block of rows shorter
    blocks_x = lambda nx: (nx // 2 + 1 + 63) // 64      # noqa: E731
    blocks_y = lambda ny: (ny + T.BLOCK_Y - 1) // T.BLOCK_Y      # noqa: E731
    for kernel in T.KERNELS:
        cases = [c for c in T.CASES if c.kernel == kernel]
        assert any(len({blocks_x(T.interior(c, s)[1]) for s in c.slots}) > 1 for c in cases), kernel
        assert any(len({blocks_y(T.interior(c, s)[0]) for s in c.slots}) > 1 for c in cases), kernel


def test_source_rows_with_the_destinations_alignment_and_with_the_other():
    """k_time_series, DEVICE backend: 16-byte loads and lone 8-byte loads, in every class; pad and base offset both vary"""
    seen = {v: set() for v in CLASSES}
    for c, s in slots("series", "device"):
        for rows in T.source_rows_aligned(c, s):
            seen[T.alignment_class(c, s)] |= set(rows)
    assert all(seen[v] == {True, False} for v in CLASSES), seen
    assert {s.src_off for _, s in slots("series", "device")} == {0, 1} and {s.pad for _, s in slots("series", "device")} == {0, 1, 2}
    # a slot whose rows are ALL aligned like the destination's, one whose rows all are not
    every = [all(all(r) for r in T.source_rows_aligned(c, s)[:1]) for c, s in slots("series", "device")]
    none = [not any(any(r) for r in T.source_rows_aligned(c, s)[:1]) for c, s in slots("series", "device")]
    assert any(every) and any(none)


@pytest.mark.parametrize("backend", T.BACKENDS)
def test_regrid_classes_with_three_and_with_five_planes(backend):
    for role in ("scalar", "pair_x", "pair_y"):
        got = {T.alignment_class(c, s) for c, s in slots("regrid", backend) if s.role == role}
        assert got == CLASSES, (backend, role, got)
    assert all(s.role == "series" for _, s in slots("series")) and all(s.role != "series" for _, s in slots("regrid"))
    assert all(s.loc == "fc" for _, s in slots("regrid") if s.role == "pair_x") and all(s.loc == "cf" for _, s in slots("regrid") if s.role == "pair_y")


def test_one_map_serves_arrays_of_two_classes():
    shared = [c for c in T.CASES if c.shared]
    assert [c.backend for c in shared] == list(T.BACKENDS)
    for c in shared:
        assert c.kernel == "regrid" and len(c.slots) == 2 and {s.loc for s in c.slots} == {"cc"}
        a, b = (T.alignment_class(c, s) for s in c.slots)
        assert a != b and (a >> 1) != (b >> 1) and (a & 1) != (b & 1)      # first row and row stride both differ
