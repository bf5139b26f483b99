"""The alignment classes and shapes that tests/test_gpu_series_alignment.py holds k_time_series (csrc/time_series.hip) and
k_time_series_regrid (csrc/time_series_regrid.hip) to, stated once; tests/test_series_alignment_table.py proves its coverage without a GPU.

Both kernels decide their control flow from addresses.  A thread's pair of points starts at 2 * pair - head, head = 1 where the
destination row's interior starts 8 bytes behind a 16-byte boundary; the regrid map is uploaded in one of four layouts
(csi_time_series.hip regrid_variant); the ring of a HOST series is shifted by one double where the destination's alignment differs from
the allocation's.  All three follow from the ALIGNMENT CLASS of the bound array,

    class = 2 * ((first interior element's address >> 3) & 1) + (ld & 1)

restated here from the offset of the parent's base behind a 16-byte boundary (in doubles), the halo and the row stride.  A class is
produced in two ways: by the halo of a grid with ordinary csi.Field parents (base on a 16-byte boundary, ld = ni), or by an array bound
by hand on a bare context (csi_grid_set + csi_field_bind) whose base lies one double behind a boundary and whose ld is ni or ni + 1.
Every case's grid is Bounded x Bounded, so its (Face, Center), (Center, Face) and (Center, Center) slots have three different interior
shapes and ride in ONE launch, whose grid the largest sizes.
"""
from collections import namedtuple

KERNELS = ("series", "regrid")                # k_time_series / k_time_series_regrid
BACKENDS = ("device", "host")
LOCS = {"fc": (1, 0), "cf": (0, 1), "cc": (0, 0)}      # location -> (extra columns, extra rows) of the interior on a Bounded x Bounded grid
SLOT_LOC = dict(TOP_U="fc", TOP_V="cf", BOT_U="fc", BOT_V="cf", SNOWFALL="cc", TOP_HEAT_FLUX="cc")
HALOS = ((4, 4), (3, 2), (5, 3), (1, 1))
BLOCK_X, BLOCK_Y, ROW_STEP = 128, 8, 4        # columns and rows of a block; a thread's second row is ROW_STEP (kBy) rows up
# the smallest shapes at which that layout can go wrong: one point, one pair, one block less / exactly / one more / one pair more, two
# blocks, two blocks and a point; no second row, a second row for some threads, one block of rows, one more
NXS, NYS = (1, 2, 3, 127, 128, 129, 130, 256, 257), (1, 3, 5, 8, 9)
SHAPES = ((1, 1), (2, 3), (3, 5), (127, 9), (128, 8), (129, 3), (130, 5), (256, 9), (257, 1))
NT = 5                                        # slices of every series of the matrix

# role: "series" (k_time_series), "scalar" (three map planes), "pair_x" / "pair_y" (the components of a rotated pair: five planes).
# base_off: doubles between a 16-byte boundary and the parent's base; ld_extra: ld - ni.  pad / src_off: the series' own layout -- pad
# extra doubles per row and pad extra rows per slice, the base src_off doubles behind a 16-byte boundary.
Slot = namedtuple("Slot", "name loc role base_off ld_extra pad src_off")
# route: "halo" (csi.Field parents) / "hand" (csi_field_bind of offset arrays).  shared: the (Center, Center) slots use ONE map.
Case = namedtuple("Case", "id kernel backend route halo Nx Ny slots shared")

# (route, halo, base_off, ld_extra, shape): what the class of each location comes to is computed below, never written down
LAYOUTS = (
    ("halo", (4, 4), 0, 0, (130, 5)), ("halo", (4, 4), 0, 0, (129, 3)),      # first row aligned; ld even / odd by location
    ("halo", (3, 2), 0, 0, (128, 8)), ("halo", (3, 2), 0, 0, (127, 9)),      # first row 8 bytes behind
    ("halo", (5, 3), 0, 0, (256, 9)), ("halo", (1, 1), 0, 0, (2, 3)),
    ("hand", (4, 4), 1, 0, (257, 1)), ("hand", (4, 4), 1, 1, (1, 1)),
    ("hand", (3, 2), 1, 0, (3, 5)), ("hand", (3, 2), 1, 1, (130, 5)),
)
ROLES = {"series": (("TOP_U", "series"), ("TOP_V", "series"), ("SNOWFALL", "series")),
         "regrid": (("TOP_U", "pair_x"), ("TOP_V", "pair_y"), ("BOT_U", "scalar"), ("BOT_V", "scalar"), ("SNOWFALL", "scalar"))}


def _cases():
    out = []
    for kernel in KERNELS:
        for backend in BACKENDS:
            for n, (route, halo, off, extra, (Nx, Ny)) in enumerate(LAYOUTS):
                slots = tuple(Slot(name, SLOT_LOC[name], role, off, extra, (n // 2 + k) % 3, (n + k) % 2) for k, (name, role) in enumerate(ROLES[kernel]))
                out.append(Case(f"{kernel}-{backend}-{route}{halo[0]}{halo[1]}-off{off}-ld{extra}-{Nx}x{Ny}", kernel, backend, route, halo, Nx, Ny, slots, False))
    # two slots of ONE location through the same map from arrays of two different classes: both device layouts of the map alive at once
    for backend in BACKENDS:
        slots = (Slot("TOP_HEAT_FLUX", "cc", "scalar", 0, 0, 0, 0), Slot("SNOWFALL", "cc", "scalar", 1, 1, 1, 1))
        out.append(Case(f"regrid-{backend}-shared-map-128x8", "regrid", backend, "hand", (4, 4), 128, 8, slots, True))
    return tuple(out)


def interior(case, slot):
    """(ny, nx) of the slot's interior"""
    ex, ey = LOCS[slot.loc]
    return case.Ny + ey, case.Nx + ex


def parent(case, slot):
    """(nj, ni, ld) of the bound array"""
    ny, nx = interior(case, slot)
    ni = nx + 2 * case.halo[0]
    return ny + 2 * case.halo[1], ni, ni + slot.ld_extra


def first_offset(case, slot):
    """doubles between a 16-byte boundary and the first interior element"""
    return slot.base_off + case.halo[0] + case.halo[1] * parent(case, slot)[2]


def alignment_class(case, slot):
    """regrid_variant of csi_time_series.hip"""
    return 2 * (first_offset(case, slot) & 1) + (parent(case, slot)[2] & 1)


def class_of_address(address, ld):
    """... from the address of the first interior element itself"""
    return 2 * ((address >> 3) & 1) + (ld & 1)


def row_heads(case, slot):
    """head of every interior row: 1 where the row starts 8 bytes behind a 16-byte boundary"""
    first, ld = first_offset(case, slot), parent(case, slot)[2]
    return [(first + j * ld) & 1 for j in range(interior(case, slot)[0])]


def source_layout(case, slot, source_shape=None):
    """(ld, slice_stride) of the series' own layout; its slices have the interior's shape (a regridded one's: the source grid's)"""
    ny, nx = source_shape or interior(case, slot)
    return nx + slot.pad, (ny + slot.pad) * (nx + slot.pad)


def source_rows_aligned(case, slot):
    """k_time_series, DEVICE backend: per slice and row, whether the source row has the destination row's alignment (16-byte loads)
    or the other one (lone 8-byte loads)"""
    lds, stride = source_layout(case, slot)
    heads = row_heads(case, slot)
    return [[((slot.src_off + n * stride + j * lds) & 1) == h for j, h in enumerate(heads)] for n in range(NT)]


CASES = _cases()
