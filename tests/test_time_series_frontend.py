"""csi.FieldTimeSeries and where the front end accepts or refuses it, without a GPU: shapes (a Face field on a Bounded side is one
wider), global data cut to a tile, refusals by name.  Models themselves need a HIP device (tests/test_gpu_time_series.py)."""
import numpy as np
import pytest

import climaseaice_jl_amd as csi
import time_series_ref as ref
from climaseaice_jl_amd.model import check_heat_fluxes

FC, CF, CC = (csi.Face, csi.Center), (csi.Center, csi.Face), (csi.Center, csi.Center)


def _grid(topo=(csi.Bounded, csi.Periodic), size=(12, 10)):
    return csi.RectilinearGrid(size, x=(0.0, 12e3), y=(0.0, 10e3), topology=topo, halo=(4, 4))


def test_interior_shape_follows_the_location_and_topology():
    g = _grid()
    t = [0.0, 1.0, 4.0]
    assert csi.FieldTimeSeries(g, FC, t).data.shape == (3, 10, 13)           # Face on a Bounded side: one wider
    assert csi.FieldTimeSeries(g, CF, t).data.shape == (3, 10, 12)           # Face on a Periodic side: not
    assert csi.FieldTimeSeries(g, CC + (None,), t).data.shape == (3, 10, 12)
    gb = _grid((csi.Periodic, csi.Bounded))
    assert csi.FieldTimeSeries(gb, CF, t, np.ones((3, 11, 12))).interior_shape == (11, 12)
    with pytest.raises(ValueError, match=r"\(Nt, ny, nx\) = \(3, 10, 13\)"):
        csi.FieldTimeSeries(g, FC, t, np.zeros((3, 10, 12)))
    with pytest.raises(ValueError, match="strictly increasing"):
        csi.FieldTimeSeries(g, CC, [0.0, 2.0, 2.0])
    with pytest.raises(ValueError, match="strictly increasing"):
        csi.FieldTimeSeries(g, CC, [0.0])
    f = csi.FieldTimeSeries(g, CC, t)
    assert isinstance(f.time_indexing, csi.Linear) and f.backend.chunk_size is None and len(f) == 3


def test_time_indexing_and_backends():
    g = _grid()
    t = [0.0, 1.0, 4.0]
    assert csi.FieldTimeSeries(g, CC, t, time_indexing=csi.Cyclical()).plan(5.5) == ref.plan(t, ref.CYCLICAL, 0.0, 5.5) == (2, 0, 0.5)
    assert csi.FieldTimeSeries(g, CC, t, time_indexing=csi.Cyclical(8.0)).plan(6.0) == (2, 0, 0.5)
    assert csi.FieldTimeSeries(g, CC, t, time_indexing=csi.Clamp()).plan(9.0) == (2, 2, 0.0)
    assert csi.FieldTimeSeries(g, CC, t, time_indexing=csi.Linear()).plan(7.0) == (1, 2, 2.0)
    with pytest.raises(ValueError, match="longer than the span"):
        csi.FieldTimeSeries(g, CC, t, time_indexing=csi.Cyclical(4.0))
    with pytest.raises(ValueError, match="positive"):
        csi.Cyclical(-1.0)
    with pytest.raises(TypeError, match="time_indexing"):
        csi.FieldTimeSeries(g, CC, t, time_indexing="cyclical")
    assert csi.InMemory(3).chunk_size == 3
    for bad in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="n >= 2"):
            csi.InMemory(bad)
    with pytest.raises(NotImplementedError, match="from disk"):
        csi.FieldTimeSeries(g, CC, t, backend="OnDisk")


def test_global_data_is_cut_to_the_tile():
    G = csi.RectilinearGrid((16, 12), x=(0.0, 16e3), y=(0.0, 12e3), topology=(csi.Bounded, csi.Periodic), halo=(4, 4))
    t = [0.0, 1.0]
    for loc in (FC, CF, CC):
        nx, ny = G.interior_size(*loc)
        data = np.arange(2 * ny * nx, dtype=np.float64).reshape(2, ny, nx)
        seen = np.zeros((ny, nx), dtype=int)
        for rank in range(4):
            tg = csi.TileGrid(G, 2, 2, rank % 2, rank // 2)
            f = csi.FieldTimeSeries(tg, loc, t, data)
            lx, ly = tg.interior_size(*loc)
            assert f.interior_shape == (ly, lx)
            for n in range(2):
                assert np.array_equal(f.data[n], tg.local_interior(data[n], *loc))          # as _cell_field / local_interior cut arrays
            seen[tg.j_off:tg.j_off + ly, tg.i_off:tg.i_off + lx] += 1
            # data already of the tile's shape is taken as it is
            assert np.array_equal(csi.FieldTimeSeries(tg, loc, t, f.data.copy()).data, f.data)
        assert np.all(seen == 1)                                                            # (the wall face belongs to the last tile)
    tg = csi.TileGrid(G, 2, 2, 1, 0)
    assert csi.FieldTimeSeries(tg, FC, t, np.zeros((2, 12, 17))).interior_shape == (6, 9)


def test_series_of_numbers_and_other_locations_are_refused_by_name():
    g = _grid()
    with pytest.raises(NotImplementedError, match="time series of NUMBERS"):
        csi.FieldTimeSeries(g, (None, None, None), [0.0, 1.0])
    with pytest.raises(NotImplementedError, match="location"):
        csi.FieldTimeSeries(g, (csi.Face, csi.Face), [0.0, 1.0])


def test_series_on_quantities_that_no_series_drives_are_refused_by_name():
    g = _grid()
    cc, fc = csi.FieldTimeSeries(g, CC, [0.0, 1.0]), csi.FieldTimeSeries(g, FC, [0.0, 1.0])
    with pytest.raises(NotImplementedError, match="PrescribedTemperature"):
        csi.PrescribedTemperature(cc)
    with pytest.raises(NotImplementedError, match=r"set!\(h\).*FieldTimeSeries cannot drive"):
        csi.CenterField(g, None, "h").set(cc)
    with pytest.raises(NotImplementedError, match="nu must be a Number"):
        csi.ViscousRheology(nu=cc)
    ice = csi.SlabThermodynamics()
    ice.prescribed = cc
    with pytest.raises(NotImplementedError, match="PrescribedTemperature"):
        check_heat_fluxes(g, ice, None, None)
    # heat fluxes and snowfall: a (Center, Center) series of the grid's shape, one array term per side
    ice = csi.SlabThermodynamics(top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    check_heat_fluxes(g, ice, (csi.RadiativeEmission(), cc, 5.0), cc, snowfall=cc)
    with pytest.raises(ValueError, match="top_heat_flux"):
        check_heat_fluxes(g, ice, fc, None)
    with pytest.raises(NotImplementedError, match="at most one array"):
        check_heat_fluxes(g, ice, (cc, np.zeros((10, 12))), None)
    with pytest.raises(ValueError, match="snowfall"):
        check_heat_fluxes(g, ice, None, None, snowfall=fc)


def test_free_drift_takes_series_at_the_components_locations():
    g = _grid()
    u, v = csi.FieldTimeSeries(g, FC, [0.0, 1.0]), csi.FieldTimeSeries(g, CF, [0.0, 1.0])
    d = csi.SeaIceMomentumEquation(g, free_drift=dict(u=u, v=v), device="cpu")
    assert d.free_drift.u is u and d.free_drift.v is v
    assert csi.SeaIceMomentumEquation(g, free_drift=(u, 0.0), device="cpu").free_drift.u is u
    with pytest.raises(ValueError, match=r"free_drift\.v: a FieldTimeSeries at \(Center, Face\)"):
        csi.SeaIceMomentumEquation(g, free_drift=dict(u=u, v=u), device="cpu")
    # stresses keep what they are given: the model materialises them
    s = csi.SemiImplicitStress(ue=u, ve=v)
    assert s.ue is u and csi.SeaIceMomentumEquation(g, top_momentum_stress=(u, v), bottom_momentum_stress=s, device="cpu").external_momentum_stresses.top[0] is u
