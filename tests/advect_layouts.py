"""Which layout of the advection kernel k_tendencies (csrc/advect.hip) a grid selects, stated once, and the case tables of
tests/test_gpu_advect_layouts.py.

The launch code picks among nine forms.  Tendencies only (launch_tendencies_mode): three tracers with snow (one tracer per thread,
64 x TY3 cells per tile), one tracer per thread (64 x TY2), two tracers per thread in tiles of 64 x 8, 63 x 7 or 63 x 11 cells.  A
whole RK stage in one launch (launch_stage_mode, advection-only RK3): the same without the snow form.  `expected_layout` mirrors
adv_two_tracers / adv_shape; tests/test_advect_layouts_table.py holds its numbers against the source text, and every GPU test asserts
what the library reports (csi_last_advection) against it.
"""
TX, TY2, TY3 = 64, 6, 4                       # CSI_ADV_TX, CSI_ADV_TY, TY3 (advect.hip)
NT2_CELLS = 200000                            # two tracers per thread from this many cells on (CSI_ADV_NT2_CELLS)
SHAPE_CELLS = (600000, 2500000)               # 64 x 8 below the first, 63 x 7 below the second, 63 x 11 from there on (adv_shape)
SHAPES = {1: (64, 8), 2: (63, 7), 3: (63, 11)}      # CSI_ADV_SHAPE -> cells of a tile


def expected_layout(Nx, Ny, has_snow=False, nt=0, shape=0):
    """(tracers per thread, tile_x, tile_y) of a tendency or stage launch on an Nx x Ny grid; nt / shape: CSI_ADV_NT / CSI_ADV_SHAPE
    (0: not set)."""
    cells = Nx * Ny
    if has_snow:
        return (1, TX, TY3)
    two = (nt == 2) if nt > 0 else cells >= NT2_CELLS
    if not two:
        return (1, TX, TY2)
    if shape == 0:
        shape = 1 if cells < SHAPE_CELLS[0] else (2 if cells < SHAPE_CELLS[1] else 3)
    return (2,) + SHAPES[shape]


# the nine launch forms: (whole stage in one launch, has_snow, layout)
LAUNCH_FORMS = [(False, True, (1, TX, TY3)), (False, False, (1, TX, TY2))] + [(False, False, (2,) + SHAPES[s]) for s in (1, 2, 3)] + \
               [(True, False, (1, TX, TY2))] + [(True, False, (2,) + SHAPES[s]) for s in (1, 2, 3)]

SCHEMES = (7, 5, -5, 3, -3, 1)                # WENO7, WENO5, Upwind5, WENO3, Upwind3, Upwind1 (CSI_ADVECT_*)
WENO = (7, 5, 3)                              # the schemes that have weights (f32 weight mode)
MODES = ("strict", "fast")
TOPOS = {"pp": ("periodic", "periodic"), "bb": ("bounded", "bounded"), "pb": ("periodic", "bounded")}

# (a) forced shapes on small grids, chosen for the tile edges: 127 = 2 * 63 + 1 (a one-column last block), 23 = 3 * 7 + 2 = 2 * 8 + 7
# = 2 * 11 + 1; 126 x 77: exact multiples of 63, 7 and 11; 128 x 24: exact for 64 x 8; 130 x 9: fewer rows than an 11-row tile
FORCED_GRIDS = ((127, 23), (126, 77), (128, 24), (130, 9))
FORCED_SHAPES = (1, 2, 3)
# one case each with shapes 2 and 3: per-row metrics, per-point metrics, north fold + mask (make_case keywords)
GEOMETRY_CASES = {
    "latlon_channel": dict(Nx=127, Ny=23, topo=("periodic", "bounded"), grid="latlon"),
    "curvilinear": dict(Nx=127, Ny=23, topo=("periodic", "periodic"), curvilinear=0.05),
    "folded_masked": dict(Nx=128, Ny=23, topo=("periodic", "folded"), curvilinear=0.04, land=0.2),
}
GEOMETRY_SHAPES = (2, 3)
# (b) f32 weights: tendencies and one RK3 step of the stage launch
F32_GRID, F32_TOPO = (127, 23), "bb"
# (c) stage launches: shapes 1 - 3 and the one-tracer layout, as (CSI_ADV_NT, CSI_ADV_SHAPE)
STAGE_GRIDS = ((127, 23), (130, 9))
STAGE_TOPOS = ("pp", "bb")
STAGE_LAYOUTS = {"nt1": (1, 0), "64x8": (2, 1), "63x7": (2, 2), "63x11": (2, 3)}
# (d) snow
SNOW_GRID = (130, 45)
# (e) the rule at its own thresholds, no environment: grid -> also one RK3 step of the stage launch
THRESHOLD_GRIDS = {(799, 250): False, (800, 250): False, (999, 600): False, (1000, 600): True, (2499, 1000): False, (2500, 1000): True}


def forced_env(nt, shape):
    """the environment that forces a layout (values a context reads when it is created)"""
    return {"CSI_ADV_NT": str(nt) if nt else "", "CSI_ADV_SHAPE": str(shape) if shape else ""}


def matrix_forms():
    """every (stage, has_snow, layout) the GPU matrix of tests/test_gpu_advect_layouts.py launches"""
    forms = set()
    for Nx, Ny in FORCED_GRIDS:
        for s in FORCED_SHAPES:
            forms.add((False, False, expected_layout(Nx, Ny, nt=2, shape=s)))
    for kw in GEOMETRY_CASES.values():
        for s in GEOMETRY_SHAPES:
            forms.add((False, False, expected_layout(kw["Nx"], kw["Ny"], nt=2, shape=s)))
    for s in FORCED_SHAPES:
        for stage in (False, True):
            forms.add((stage, False, expected_layout(*F32_GRID, nt=2, shape=s)))
    for Nx, Ny in STAGE_GRIDS:
        for nt, s in STAGE_LAYOUTS.values():
            for stage in (False, True):                        # (set_fusion(0): the same layout through the tendency launch)
                forms.add((stage, False, expected_layout(Nx, Ny, nt=nt, shape=s)))
    forms.add((False, True, expected_layout(*SNOW_GRID, has_snow=True, nt=2)))
    for (Nx, Ny), stage in THRESHOLD_GRIDS.items():
        forms.add((False, False, expected_layout(Nx, Ny)))
        if stage:
            forms.add((True, False, expected_layout(Nx, Ny)))
    return forms
