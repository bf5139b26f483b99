"""Every field slot through the C ABI: the extents csi_field_bind accepts, the name it prints, and which of csi_fill_halo_local and
csi_time_series_set take the slot.  Only API calls: nothing is launched.

The grid has unequal extents and halos (Nx = 5, Ny = 4, Hx = 2, Hy = 3, Bounded both ways), so the four locations have four different
parent extents and an x / y or a Center / Face mix-up in a slot's row shows.  The locations, display names and role lists below are
typed in from the behaviour of the library before it had a slot table (csrc/csi_slots.h, _lib.SLOTS); they are not read from either.
"""
import ctypes as C

import pytest
import torch

import climaseaice_jl_amd as csi

pytestmark = pytest.mark.gpu
L = csi._lib

NX, NY, HX, HY = 5, 4, 2, 3
EXTENTS = {"cc": (NX + 2 * HX, NY + 2 * HY), "fc": (NX + 2 * HX + 1, NY + 2 * HY), "cf": (NX + 2 * HX, NY + 2 * HY + 1),
           "ff": (NX + 2 * HX + 1, NY + 2 * HY + 1)}
# (display name, location) of slot id 0, 1, ..., 71
SLOTS = [("u", "fc"), ("v", "cf"), ("h", "cc"), ("aice", "cc"), ("sigma11", "cc"), ("sigma22", "cc"), ("sigma12", "ff"), ("un", "fc"),
         ("vn", "cf"), ("P", "cc"), ("alpha", "cc"), ("Delta", "cc"), ("zeta_f", "ff"), ("zeta_c", "cc"), ("Gh", "cc"), ("Gaice", "cc"),
         ("h-", "cc"), ("aice-", "cc"), ("u-", "fc"), ("v-", "cf"), ("top_u", "fc"), ("top_v", "cf"), ("bottom_u", "fc"),
         ("bottom_v", "cf"), ("mass_flux", "cc"), ("hs", "cc"), ("Ghs", "cc"), ("hs-", "cc"), ("mass_flux_snow", "cc"),
         ("intercepted_snowfall", "cc"), ("Tu", "cc"), ("Tu_snow", "cc"), ("forcing_u", "fc"), ("forcing_v", "cf"), ("Gu", "fc"),
         ("Gv", "cf"), ("top_heat_flux", "cc"), ("bottom_heat_flux", "cc"), ("snowfall", "cc"), ("free_drift_u", "fc"),
         ("free_drift_v", "cf"), ("divergence", "cc"), ("shear", "cc"), ("deformation", "cc"), ("speed", "cc"), ("sigma_I", "cc"),
         ("sigma_II", "cc"), ("stress_power", "cc"), ("coriolis_x", "fc"), ("coriolis_y", "cf"), ("top_x", "fc"), ("top_y", "cf"),
         ("bottom_x", "fc"), ("bottom_y", "cf"), ("internal_x", "fc"), ("internal_y", "cf"), ("forcing_x", "fc"), ("forcing_y", "cf"),
         ("flux_coefficient", "cc"), ("flux_reference_temperature", "cc"), ("bottom_salinity", "cc"), ("top_heat_flux_used", "cc"),
         ("bottom_heat_flux_used", "cc"), ("ocean_temperature", "cc"), ("ocean_temperature-", "cc"), ("ocean_surface_heat_flux", "cc"),
         ("ocean_coefficient", "cc"), ("ocean_reference_temperature", "cc"), ("ocean_deep_heat_flux", "cc"),
         ("ocean_surface_flux_used", "cc"), ("shortwave", "cc"), ("albedo_used", "cc")]
HALO_IDS = list(range(36)) + [39, 40]                                                   # csi_field_id and the two free-drift fields
SERIES_IDS = [20, 21, 22, 23, 32, 33, 39, 40] + [36, 37, 38] + [58, 59, 60] + [65, 66, 67, 68] + [70]
OK, INVALID, NOT_BOUND = 0, -1, -2


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    met = L.Metrics()
    met.dx, met.dy = 1.0, 1.0
    c.call("csi_grid_set", NX, NY, HX, HY, L.BOUNDED, L.BOUNDED, L.METRIC_UNIFORM, C.byref(met))
    yield c
    c.close()


def _rc(ctx, name, *args):
    rc = getattr(ctx.L, name)(ctx.h, *args)
    return rc, ctx.L.csi_last_error(ctx.h).decode()


def test_the_lists_cover_every_slot():
    assert len(SLOTS) == 72 and len(HALO_IDS) == 38 and len(SERIES_IDS) == 19
    assert len(set(n for n, _ in SLOTS)) == 72 and len(set(EXTENTS.values())) == 4


@pytest.mark.parametrize("fid", range(72))
def test_slot_binds_at_its_location_only_and_names_itself(ctx, fid):
    name, loc = SLOTS[fid]
    buf = torch.zeros(EXTENTS["ff"][0] * EXTENTS["ff"][1], dtype=torch.float64, device="cuda:0")      # large enough for any location
    ptr = C.c_void_p(buf.data_ptr())
    # 3. unbound: the halo entry points know the slot or do not
    assert _rc(ctx, "csi_field_bind", fid, None, 0, 0, 0)[0] == OK
    rc, msg = _rc(ctx, "csi_fill_halo_local", fid)
    if fid in HALO_IDS:
        assert rc == NOT_BOUND and msg.endswith(f"field not bound: {name}"), (rc, msg)
    else:
        assert rc == INVALID and "unknown field id" in msg, (rc, msg)
    # 2. the extents of every other location are refused, by the slot's name
    for other, (ni, nj) in EXTENTS.items():
        if other != loc:
            rc, msg = _rc(ctx, "csi_field_bind", fid, ptr, ni, ni, nj)
            assert rc == INVALID and f"field {name}:" in msg, (other, rc, msg)
    # 1. its own are accepted
    ni, nj = EXTENTS[loc]
    assert _rc(ctx, "csi_field_bind", fid, ptr, ni, ni, nj)[0] == OK
    # 4. a series may drive it or not (NULL removes the slot's series: nothing to remove, CSI_OK)
    rc, msg = _rc(ctx, "csi_time_series_set", fid, None)
    assert rc == (OK if fid in SERIES_IDS else INVALID), (rc, msg)
    assert _rc(ctx, "csi_field_bind", fid, None, 0, 0, 0)[0] == OK      # (the buffer goes away with this test)


@pytest.mark.parametrize("fid", [-1, 72])
def test_ids_outside_the_table_are_refused(ctx, fid):
    buf = torch.zeros(EXTENTS["ff"][0] * EXTENTS["ff"][1], dtype=torch.float64, device="cuda:0")
    ni, nj = EXTENTS["cc"]
    for call in (("csi_field_bind", fid, C.c_void_p(buf.data_ptr()), ni, ni, nj), ("csi_fill_halo_local", fid)):
        rc, msg = _rc(ctx, *call)
        assert rc == INVALID and "unknown field id" in msg, (call[0], rc, msg)
    rc, msg = _rc(ctx, "csi_time_series_set", fid, None)
    assert rc == INVALID and "time series: the slot is not one" in msg, (rc, msg)
