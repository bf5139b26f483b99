"""The reference's examples/arctic_basin_seasonal_cycle.jl (Semtner 1976) with the MI355X library: a column of Arctic sea ice under
the climatological monthly forcing of Fletcher (1965) -- shortwave, longwave, sensible and latent heat, twelve values each, every month
30 days long, repeated year after year with Cyclical time indexing and interpolated linearly at the model clock -- and its own radiative
emission with Semtner's 1.02 sigma.  Absorbed shortwave is Q (1 - alpha) with alpha = 0.75 below a surface temperature of -0.1 C and
0.64 from there on: the ice-albedo feedback.  The reference writes that into a FluxFunction closure; here it is data, a
ShortwaveRadiation term with a SteppedAlbedo (include/csi.h, csi_shortwave_set), so the secant solve of the surface temperature sees the
albedo change.  30 cm of ice to start with, dt = 8 hours, 30 years of 360 days (32 400 steps).  The reference's grid is a single point;
here 4 x 1, the smallest grid the library takes, four identical columns.

ONE DEPARTURE.  A side has at most one array term, so longwave, sensible and latent heat are summed into one series on the host,
longwave + (sensible + latent) month by month; linear interpolation commutes with the sum.  The reference adds the three interpolated
values to the emission one after the other, so the last bits of the top heat flux may differ.

    python examples/arctic_basin_seasonal_cycle.py      (needs the GPU; prints the thickness at the end of every fifth year, then the
                                                         last year's minimum, maximum and mean thickness)
"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

DAY = 86400.0
MONTH_DAYS = 30
YEAR = 12 * MONTH_DAYS * DAY
TIMES = np.arange(15, 360, 30) * DAY                    # mid-month
# Semtner (1976), Table 1, after Fletcher (1965): monthly totals in 1e4 kcal m^-2, downward, January to December
TABLE = dict(shortwave=[0, 0, 1.9, 9.9, 17.7, 19.2, 13.6, 9.0, 3.7, 0.4, 0, 0],
             longwave=[10.4, 10.3, 10.3, 11.6, 15.1, 18.0, 19.1, 18.7, 16.5, 13.9, 11.2, 10.9],
             sensible=[1.18, 0.76, 0.72, 0.29, -0.45, -0.39, -0.30, -0.40, -0.17, 0.1, 0.56, 0.79],
             latent=[0, -0.02, -0.03, -0.09, -0.46, -0.70, -0.64, -0.66, -0.39, -0.19, -0.01, -0.01])
# ... in W m^-2, positive upward: 4184 J per kcal over a month
FLUX = {k: (-np.array(v, dtype=np.float64) * 1e4) * (4184 / (MONTH_DAYS * DAY)) for k, v in TABLE.items()}
FLUX["others"] = FLUX["longwave"] + (FLUX["sensible"] + FLUX["latent"])
SIGMA = 5.67e-8 * 1.02                                  # Semtner's value, about 2 % high, kept for comparison as the reference does
ALBEDO = dict(cold=0.75, warm=0.64, threshold=-0.1)
DT = 8 * 3600.0
YEARS = 30


def build(device="cuda:0", timestepper="SplitRungeKutta3", h0=0.3):
    grid = csi.RectilinearGrid((4, 1), x=(0.0, 1.0), y=(0.0, 1.0), topology=(csi.Periodic, csi.Periodic), halo=(1, 1))
    series = lambda values: csi.FieldTimeSeries(grid, (csi.Center, csi.Center), TIMES, np.broadcast_to(values[:, None, None], (12, 1, 4)).copy(),
                                                time_indexing=csi.Cyclical())       # (the period is inferred: 360 days)
    top_heat_flux = (csi.ShortwaveRadiation(series(FLUX["shortwave"]), albedo=csi.SteppedAlbedo(**ALBEDO)),
                     series(FLUX["others"]),
                     csi.RadiativeEmission(emissivity=1.0, stefan_boltzmann_constant=SIGMA))
    ice = csi.SlabThermodynamics(top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    model = csi.SeaIceModel(grid, ice_thermodynamics=ice, top_heat_flux=top_heat_flux, timestepper=timestepper, device=device)
    csi.set_(model, h=h0, aice=1.0)
    return model


def column(model):
    """(h, aice, Tu, albedo) of the first column."""
    model.synchronize()
    return tuple(float(f.interior_numpy()[0, 0]) for f in (model.ice_thickness, model.ice_concentration,
                                                           model.ice_thermodynamics.top_surface_temperature, model.albedo_used))


def run(model, years=YEARS, dt=DT):
    """Steps `years` years; returns the thickness after every step of the last one."""
    per_year = int(round(YEAR / dt))
    model.albedo_used
    last = []
    for year in range(years):
        for n in range(per_year):
            csi.time_step(model, dt)
            if year == years - 1:
                last.append(column(model)[0])
        if (year + 1) % 5 == 0:
            h, a, Tu, alpha = column(model)
            print(f"year {year + 1:2d}   h = {h:7.4f} m   aice = {a:6.4f}   Tu = {Tu:8.4f} C   albedo = {alpha:4.2f}")
    return np.array(last)


if __name__ == "__main__":
    model = build()
    t0 = time.perf_counter()
    last = run(model)
    wall = time.perf_counter() - t0
    assert np.all(np.isfinite(last)) and all(np.isfinite(x) for x in column(model)), "a field is not finite"
    print(f"last year: thickness min = {last.min():.4f} m   max = {last.max():.4f} m   mean = {last.mean():.4f} m   "
          f"({YEARS} years, {YEARS * int(round(YEAR / DT))} steps in {wall:.1f} s)")
