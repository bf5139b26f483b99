"""Port of the reference's examples/diffusive_ice_column_model.jl: one column of 20 levels resolved with the enthalpy method, molecular
diffusivity that differs between ice and water, a daily cycle with a cooling trend on top and a slowly cooling ocean below; ten days
of explicit steps of 0.1 dz^2 / kappa = 25 s.

The two boundary functions are sampled into ColumnTimeSeries at the step times (the clock's own times: one addition per step), so the
series returns the functions' values at every step exactly.  The run advances an hour -- 144 steps, three launches of the on-chip
kernel -- per call, and takes the ice thickness and the profiles hourly.  update_state() comes first, as run! calls it.

  python examples/diffusive_ice_column_model.py [--days 10] [--plot out.png]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import climaseaice_jl_amd as csi      # noqa: E402

DAY, HOUR = 86400.0, 3600.0


def air_ice_temperature(t):
    return (-0.5 / DAY) * t + 5 * np.sin(2 * np.pi * t / DAY) + -5


def ice_ocean_temperature(t):
    return (-0.1 / DAY) * t + 1.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=float, default=10.0)
    ap.add_argument("--plot", default=None)
    a = ap.parse_args()

    grid = csi.ColumnGrid(20, z=(-1, 0), topology=(csi.Flat, csi.Flat, csi.Bounded))
    closure = csi.MolecularDiffusivity(kappa_ice=1e-5, kappa_water=1e-6)
    dt = 0.1 * grid.minimum_zspacing() ** 2 / 1e-5
    per_hour = int(round(HOUR / dt))                       # 144
    hours = int(round(a.days * 24))
    nsteps = hours * per_hour

    # the step times as the clock forms them, and the two functions sampled there
    times = np.empty(nsteps + 2)
    times[0] = 0.0
    for k in range(1, times.size):
        times[k] = times[k - 1] + dt
    T_bcs = csi.FieldBoundaryConditions(top=csi.ValueBoundaryCondition(csi.ColumnTimeSeries(grid, times, air_ice_temperature(times))),
                                        bottom=csi.ValueBoundaryCondition(csi.ColumnTimeSeries(grid, times, ice_ocean_temperature(times))))
    model = csi.EnthalpyMethodSeaIceModel(grid, closure=closure, boundary_conditions=dict(T=T_bcs))
    model.set(T=1.1)
    model.update_state()

    th, ht, profiles, launches = [], [], [], 0
    t0 = time.perf_counter()
    for _ in range(hours):
        model.time_steps(dt, per_hour)
        launches += model.last_launch()["launches"]
        th.append(model.clock.time)
        ht.append(float(model.ice_thickness(melting_temperature=-0.1)[0, 0]))
        profiles.append({k: f.interior_numpy()[:, 0, 0].copy() for k, f in model.fields().items()})
    wall = time.perf_counter() - t0
    form = model.last_launch()["form"]
    print(f"{nsteps} steps of {dt:.3f} s ({a.days:g} days) in {wall:.3f} s wall: {launches} launches of the {form} kernel, "
          f"{hours} thickness launches; final thickness {ht[-1]:.4f} m, frozen levels {int(profiles[-1]['phi'].sum())} of {grid.Nz}")
    for h in range(23, hours, 24):
        print(f"  day {(h + 1) // 24:2d}: thickness {ht[h]:.4f} m, top cell {profiles[h]['T'][-1]:8.3f} C, bottom cell {profiles[h]['T'][0]:6.3f} C")
    if a.plot:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        fig, ax = plt.subplots(1, 2, figsize=(10, 4))
        for h in range(23, hours, 48):
            ax[0].plot(profiles[h]["T"], grid.z_centers, label=f"day {(h + 1) // 24}")
        ax[0].set_xlabel("Temperature (C)"), ax[0].set_ylabel("z (m)"), ax[0].legend()
        ax[1].plot(np.array(th) / HOUR, ht)
        ax[1].set_xlabel("Time (hours)"), ax[1].set_ylabel("Ice thickness (m)")
        fig.savefig(a.plot, dpi=120)
    return ht


if __name__ == "__main__":
    main()
