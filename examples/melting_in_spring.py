"""The reference's examples/melting_in_spring.jl with the MI355X library: four columns of 1 m ice under -600 ... -1200 W m^-2 of sun,
longwave emission and a bulk sensible heat flux Cs rho_a c_a u_a (Tu - Ta) aice -- the reference's FluxFunction closure, here data
(LinearHeatFlux) -- bare and under 20 cm of snow; dt = 10 minutes, 30 days.  The reference's grid is (4, Flat, Flat); here 4 x 1.

    python examples/melting_in_spring.py          (needs the GPU; prints the four columns of both models once per day)
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

SOLAR = np.array([[-600.0, -800.0, -1000.0, -1200.0]])      # W m^-2, one value per column
PARAMETERS = dict(transfer_coefficient=1e-3, atmosphere_density=1.225, atmosphere_heat_capacity=1004, atmosphere_wind_speed=5,
                  atmosphere_temperature=-5)


def build(snow=False, device="cuda:0"):
    grid = csi.RectilinearGrid((4, 1), x=(0.0, 1.0), y=(0.0, 1.0), topology=(csi.Periodic, csi.Periodic), halo=(1, 1))
    ice = csi.SlabThermodynamics(top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance(), ice_consolidation_thickness=0.05)
    top_heat_flux = (csi.RadiativeEmission(), SOLAR, csi.bulk_sensible_heat_flux(area_weighting="concentration", **PARAMETERS))
    kw = dict(snow_thermodynamics=csi.snow_slab_thermodynamics(grid)) if snow else {}
    model = csi.SeaIceModel(grid, ice_thermodynamics=ice, top_heat_flux=top_heat_flux, timestepper="ForwardEuler", device=device, **kw)
    csi.set_(model, h=1.0, aice=1.0, **(dict(hs=0.2) if snow else {}))       # 20 cm of snow, no precipitation
    return model


def columns(model):
    """(h, aice, Tu[, hs]) of the four columns; Tu is the snow surface's where there is a snow layer."""
    model.synchronize()
    snow = model.snow_thickness is not None
    T = model.snow_top_temperature if snow else model.ice_thermodynamics.top_surface_temperature
    out = [model.ice_thickness.interior_numpy()[0], model.ice_concentration.interior_numpy()[0], T.interior_numpy()[0]]
    return out + ([model.snow_thickness.interior_numpy()[0]] if snow else [])


def run(model, steps=30 * 144, dt=600.0, every=144):
    series = []
    for n in range(steps):
        csi.time_step(model, dt)
        if (n + 1) % every == 0:
            series.append(((n + 1) * dt / 86400.0, [x.copy() for x in columns(model)]))
    return series


if __name__ == "__main__":
    for snow in (False, True):
        print("snow-covered ice" if snow else "bare ice")
        for day, cols in run(build(snow)):
            print(f"day {day:5.1f}   " + "   ".join(f"{name} = " + " ".join(f"{v:8.4f}" for v in x)
                                                     for name, x in zip(("h", "aice", "Tu", "hs"), cols)))
