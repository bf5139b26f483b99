"""The reference's examples/freezing_of_a_lake.jl with the MI355X library: four columns of a 10 m deep freshwater lake that start at
1 C under air of -20, -10, -5 and 0 C; the lake cools over its open water, and the heat deficit below freezing grows ice from above --
bare ice and, in a second model, ice under light snowfall.  The reference writes the lake into a FluxFunction closure that advances a
bucket of water as a side effect; here it is data: SlabOceanMixedLayer (include/csi.h, csi_mixed_layer_set), with
ice_ocean_exchange_velocity = 0 (the closure has no basal melt).  The top heat flux is the closure's bulk sensible heat flux, zero
where there is no ice: a LinearHeatFlux with the "ice_present" weighting.  dt = 10 minutes, 20 days (2 880 steps).  The reference's
grid is (4, Flat, Flat); here 4 x 1.

ONE DEPARTURE.  The reference's closure warms the lake with Qa / (rho_o c_o) * dt, without dividing by the depth, yet takes the frazil
heat from the full 10 m.  The port uses the depth in both places: the lake's heat capacity per area is rho_o c_o depth throughout, so
the lake cools ten times more slowly than in the reference's run and its heat budget closes.

    python examples/freezing_of_a_lake.py          (needs the GPU; prints the four columns of both models every two days)
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

ATMOSPHERE_TEMPERATURE = np.array([[-20.0, -10.0, -5.0, 0.0]])      # C, one value per column
ATMOSPHERE = dict(transfer_coefficient=1e-3, atmosphere_density=1.225, atmosphere_heat_capacity=1004, atmosphere_wind_speed=5)
LAKE = dict(depth=10.0, temperature=1.0, density=1000.0, heat_capacity=4000.0, ice_ocean_exchange_velocity=0.0)
SNOWFALL = 6e-5      # kg m^-2 s^-1


def build(snow=False, device="cuda:0"):
    grid = csi.RectilinearGrid((4, 1), x=(0.0, 1.0), y=(0.0, 1.0), topology=(csi.Periodic, csi.Periodic), halo=(1, 1))
    ice = csi.SlabThermodynamics(top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance(), ice_consolidation_thickness=0.05)
    # the same K and Ta serve the ice top and the open water
    top_heat_flux = csi.bulk_sensible_heat_flux(atmosphere_temperature=ATMOSPHERE_TEMPERATURE, area_weighting="ice_present", **ATMOSPHERE)
    lake = csi.SlabOceanMixedLayer(coefficient=top_heat_flux.coefficient, atmosphere_temperature=ATMOSPHERE_TEMPERATURE, **LAKE)
    kw = dict(snow_thermodynamics=csi.snow_slab_thermodynamics(grid), snowfall=SNOWFALL) if snow else {}
    model = csi.SeaIceModel(grid, ice_thermodynamics=ice, top_heat_flux=top_heat_flux, ocean=lake, timestepper="ForwardEuler",
                            device=device, **kw)
    csi.set_(model, h=0.0, aice=0.0, **(dict(hs=0.0) if snow else {}))
    return model


def columns(model):
    """(h, aice, Tu, To[, hs]) of the four columns; Tu is the snow surface's where there is a snow layer, To the lake's temperature."""
    model.synchronize()
    snow = model.snow_thickness is not None
    T = model.snow_top_temperature if snow else model.ice_thermodynamics.top_surface_temperature
    out = [model.ice_thickness.interior_numpy()[0], model.ice_concentration.interior_numpy()[0], T.interior_numpy()[0],
           model.ocean.temperature.interior_numpy()[0]]
    return out + ([model.snow_thickness.interior_numpy()[0]] if snow else [])


def run(model, steps=20 * 144, dt=600.0, every=288):
    series = []
    for n in range(steps):
        csi.time_step(model, dt)
        if (n + 1) % every == 0:
            series.append(((n + 1) * dt / 86400.0, [x.copy() for x in columns(model)]))
    return series


if __name__ == "__main__":
    for snow in (False, True):
        print("snow-covered lake ice" if snow else "bare lake ice")
        model = build(snow)
        for day, cols in run(model):
            print(f"day {day:5.1f}   " + "   ".join(f"{name} = " + " ".join(f"{v:8.4f}" for v in x)
                                                     for name, x in zip(("h", "aice", "Tu", "To", "hs"), cols)))
        assert all(np.all(np.isfinite(x)) for x in columns(model)), "a field is not finite"
