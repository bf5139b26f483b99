"""The table of tests/advect_layouts.py, checked without a GPU: its thresholds and tile constants are the ones csrc/advect.hip states,
its rule is the one adv_two_tracers / adv_shape spell, and the GPU matrix launches every one of the nine forms of k_tendencies."""
import os
import re

import pytest

import advect_layouts as al

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "climaseaice.jl_amd", "csrc", "advect.hip")


@pytest.fixture(scope="module")
def text():
    with open(SRC) as f:
        return f.read()


def test_tile_constants(text):
    assert int(re.search(r"#define CSI_ADV_TX (\d+)", text).group(1)) == al.TX
    assert int(re.search(r"#define CSI_ADV_TY (\d+)", text).group(1)) == al.TY2
    m = re.search(r"constexpr int TX = CSI_ADV_TX, TY2 = CSI_ADV_TY, TY3 = (\d+);", text)
    assert int(m.group(1)) == al.TY3
    # a block has (tile_x + 1) x (tile_y + 1) threads per tracer plane: within 1024 for every form
    for stage, snow, (nt, tx, ty) in al.LAUNCH_FORMS:
        assert (tx + 1) * (ty + 1) * (3 if snow else (2 if nt == 1 else 1)) <= 1024


def test_thresholds(text):
    assert int(re.search(r"#define CSI_ADV_NT2_CELLS (\d+)L", text).group(1)) == al.NT2_CELLS
    m = re.search(r"return cells < (\d+)L \? SHAPE_64x8 : \(cells < (\d+)L \? SHAPE_63x7 : SHAPE_63x11\);", text)
    assert (int(m.group(1)), int(m.group(2))) == al.SHAPE_CELLS
    m = re.search(r"enum \{ SHAPE_64x8 = (\d), SHAPE_63x7 = (\d), SHAPE_63x11 = (\d) \};", text)
    assert [int(v) for v in m.groups()] == [0, 1, 2]
    # CSI_ADV_SHAPE = the enum + 1; CSI_ADV_NT forces the tracers per thread; snow never takes two
    assert re.search(r"if \(A\.shape > 0\) return A\.shape - 1;", text)
    assert re.search(r"if \(A\.has_snow\) return false;\s*\n\s*if \(A\.nt > 0\) return A\.nt == 2;", text)
    assert re.search(r"return \(long\)A\.g\.Nx \* \(long\)A\.g\.Ny >= CSI_ADV_NT2_CELLS;", text)


def test_launch_code_spells_the_same_tiles(text):
    """the tile sizes of both launchers, and the template arguments <.., TY, W, 2, TXP> of the two-tracer instantiations"""
    assert text.count("const int tx = two ? (shape == SHAPE_64x8 ? 64 : 63) : adv::TX;") == 2
    assert text.count("(two ? (shape == SHAPE_64x8 ? 8 : (shape == SHAPE_63x7 ? 7 : 11)) : adv::TY2)") + \
        text.count("= two ? (shape == SHAPE_64x8 ? 8 : (shape == SHAPE_63x7 ? 7 : 11)) : adv::TY2;") == 2
    assert "const int ty = A.has_snow ? adv::TY3 :" in text
    for step in ("false", "true"):
        for cond, (tx, ty) in (("two && shape == SHAPE_64x8", al.SHAPES[1]), ("two && shape == SHAPE_63x7", al.SHAPES[2]), ("two", al.SHAPES[3])):
            assert f"if ({cond}) hipLaunchKernelGGL((adv::k_tendencies<S, FAST, {step}, {ty}, W, 2, {tx}>)" in text, (step, cond)
        assert f"else hipLaunchKernelGGL((adv::k_tendencies<S, FAST, {step}, adv::TY2, W>)" in text
    assert "if (A.has_snow) hipLaunchKernelGGL((adv::k_tendencies<S, FAST, false, adv::TY3, W>)" in text
    assert text.count("return AdvLayout{two ? 2 : 1, tx, ty};") == 2         # what csi_last_advection reports is what was launched


def test_rule_at_its_edges():
    e = al.expected_layout
    assert e(799, 250) == (1, 64, 6) and e(800, 250) == (2, 64, 8)
    assert e(999, 600) == (2, 64, 8) and e(1000, 600) == (2, 63, 7)
    assert e(2499, 1000) == (2, 63, 7) and e(2500, 1000) == (2, 63, 11)
    assert e(512, 512) == (2, 64, 8) and e(1024, 1024) == (2, 63, 7) and e(2048, 2048) == (2, 63, 11)      # the benchmarked sizes
    # the knobs: CSI_ADV_NT decides the tracers per thread at any size, CSI_ADV_SHAPE the shape where two are taken -- and only there
    assert e(127, 23, nt=2) == (2, 64, 8) and e(127, 23, nt=2, shape=2) == (2, 63, 7) and e(127, 23, nt=2, shape=3) == (2, 63, 11)
    assert e(127, 23, shape=3) == (1, 64, 6) and e(2500, 1000, nt=1, shape=2) == (1, 64, 6)
    assert e(2500, 1000, shape=1) == (2, 64, 8)
    assert e(2500, 1000, has_snow=True, nt=2, shape=3) == (1, 64, 4)
    for (Nx, Ny), _ in al.THRESHOLD_GRIDS.items():
        assert Nx * Ny in (al.NT2_CELLS, *al.SHAPE_CELLS) or Nx * Ny + Ny in (al.NT2_CELLS, *al.SHAPE_CELLS), (Nx, Ny)


def test_the_matrix_reaches_every_launch_form():
    assert len(al.LAUNCH_FORMS) == len(set(al.LAUNCH_FORMS)) == 9
    forms = al.matrix_forms()
    assert forms == set(al.LAUNCH_FORMS), (sorted(set(al.LAUNCH_FORMS) - forms), sorted(forms - set(al.LAUNCH_FORMS)))
    # 162 instantiations: nine forms x six schemes x two modes, + f32 weights for the three WENO orders
    assert len(al.LAUNCH_FORMS) * (len(al.SCHEMES) + len(al.WENO)) * len(al.MODES) == 162


def test_forced_grids_hit_the_tile_edges():
    """what the grids of the forced matrix were chosen for: a one-column last block, exact multiples, a grid shorter than a tile"""
    assert 127 % 63 == 1 and 23 % 7 == 2 and 23 % 8 == 7 and 23 % 11 == 1
    assert 126 % 63 == 0 and 77 % 7 == 0 and 77 % 11 == 0
    assert 128 % 64 == 0 and 24 % 8 == 0
    assert 9 < 11 and 130 > 2 * 64
    for g in ((127, 23), (126, 77), (128, 24), (130, 9)):
        assert g in al.FORCED_GRIDS
        assert g[0] * g[1] < al.NT2_CELLS           # (all forced: without CSI_ADV_NT they would take one tracer per thread)
