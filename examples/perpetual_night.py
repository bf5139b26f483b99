"""The reference's examples/perpetual_night.jl with the MI355X library: an ice slab that emits longwave radiation
(RadiativeEmission) and receives a constant -200 W m^-2 from above, under MeltingConstrainedFluxBalance, from h = 0.01 m;
dt = 1 hour, 40 days.  The reference's grid is Flat; here a small grid of identical columns.

    python examples/perpetual_night.py            (needs the GPU; prints thickness and top temperature once per day)
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import climaseaice_jl_amd as csi


def build(device="cuda:0", Nx=4, Ny=4):
    grid = csi.RectilinearGrid((Nx, Ny), x=(0.0, 1.0), y=(0.0, 1.0), topology=(csi.Periodic, csi.Periodic), halo=(1, 1))
    ice_thermodynamics = csi.SlabThermodynamics(top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    top_flux = csi.CenterField(grid, device, "top_flux")
    top_flux.set(-200.0)
    model = csi.SeaIceModel(grid, ice_thermodynamics=ice_thermodynamics, top_heat_flux=(csi.RadiativeEmission(), top_flux),
                            timestepper="ForwardEuler", device=device)
    csi.set_(model, h=0.01)
    return model


def run(model, steps=960, dt=3600.0, every=24):
    series = []
    for n in range(steps):
        csi.time_step(model, dt)
        if (n + 1) % every == 0:
            model.synchronize()
            T = model.ice_thermodynamics.top_surface_temperature.interior_numpy()[0, 0]
            series.append(((n + 1) * dt / 86400.0, float(model.ice_thickness.interior_numpy()[0, 0]), float(T)))
    return series


if __name__ == "__main__":
    m = build()
    for day, h, T in run(m):
        print(f"day {day:5.1f}   h = {h:.6f} m   Tu = {T:8.3f} degC")
