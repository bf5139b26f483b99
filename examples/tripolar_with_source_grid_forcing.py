"""A small TripolarGrid driven by forcing "as downloaded": a synthetic 3-hourly wind on a 64 x 32 periodic longitude-latitude grid and
an ocean surface current from a second, coarser product that carries NaN on its land -- filled once with csi.fill_missing.  Both are
vectors in geographic axes; the library regrids them on the device at every step (time at the four surrounding source points, then
bilinear in space) and rotates them into the grid's local axes in the bipolar cap, where the grid's x direction is not east.  Nothing is
downloaded; nothing is regridded on the host.

    python examples/tripolar_with_source_grid_forcing.py [hours]       (needs the GPU)
"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

hours = float(sys.argv[1]) if len(sys.argv) > 1 else 12.0
dt = 600.0
grid = csi.TripolarGrid((64, 48), southernmost_latitude=-80.0, halo=(4, 4))
wet = grid.analytic_land()

# the atmosphere product: 10 m wind, eight 3-hourly slices that repeat daily, on 64 x 32 points
atm = csi.SourceGrid(np.arange(64) * 5.625 - 180.0, np.linspace(-88.6, 88.6, 32), periodic_x=True)
t_atm = np.arange(8) * 3 * 3600.0
lam, phi, n = np.deg2rad(atm.x)[None, None, :], np.deg2rad(atm.y)[None, :, None], np.arange(8)[:, None, None]
wind = csi.RegriddedVectorTimeSeries(grid, atm, t_atm, east=8.0 * np.cos(phi) * np.cos(lam + 2 * np.pi * n / 8) + 2.0 * np.sin(3 * phi),
                                     north=3.0 * np.sin(2 * lam - 2 * np.pi * n / 8) * np.cos(phi), time_indexing=csi.Cyclical(), backend=csi.InMemory(3))

# the ocean product: daily surface currents on 40 x 24 points, NaN on its land (a band of longitudes and the far south)
ocn = csi.SourceGrid(np.arange(40) * 9.0 - 175.5, np.linspace(-86.0, 89.0, 24), periodic_x=True, period=360.0)
t_ocn = np.arange(3) * 86400.0
lam, phi, n = np.deg2rad(ocn.x)[None, None, :], np.deg2rad(ocn.y)[None, :, None], np.arange(3)[:, None, None]
uo, vo = 0.08 * np.sin(2 * phi) * np.cos(lam) * (1 + 0.1 * n), 0.05 * np.cos(phi) * np.sin(2 * lam + 0.2 * n)
sea = np.ones(ocn.shape, dtype=bool)
sea[:, 10:14] = False
sea[:3, :] = False
uo, vo = np.where(sea, uo, np.nan), np.where(sea, vo, np.nan)
current = csi.RegriddedVectorTimeSeries(grid, ocn, t_ocn, csi.fill_missing(uo, sea), csi.fill_missing(vo, sea), time_indexing=csi.Clamp())

dyn = csi.SeaIceMomentumEquation(grid, coriolis=csi.PointwiseCoriolis(*grid.coriolis_planes()), rheology=csi.ElastoViscoPlasticRheology(),
                                 top_momentum_stress=csi.SemiImplicitStress(ue=wind.x, ve=wind.y, rho_e=1.3, Cd=1.2e-3),
                                 bottom_momentum_stress=csi.SemiImplicitStress(ue=current.x, ve=current.y),
                                 solver=csi.SplitExplicitSolver(substeps=60))
model = csi.SeaIceModel(grid, dynamics=dyn, advection=csi.WENO(order=7), timestepper="SplitRungeKutta3")
model.set_mask(wet)
_, lat = grid.nodes_2d(csi.Center, csi.Center)
icy = wet & (np.abs(lat) > 60.0)
csi.set_(model, h=np.where(icy, 1.0, 0.0), aice=np.where(icy, 0.9, 0.0))
steps = int(hours * 3600 / dt)
t0 = time.perf_counter()
for _ in range(steps):
    csi.time_step(model, dt)
model.synchronize()
wall = time.perf_counter() - t0
launches, maps = model.ctx.regrid_stats()
u, v = model.velocities.u.interior_numpy(), model.velocities.v.interior_numpy()
ua = model.external_stress_field("TOP", "U").interior_numpy()
cos_u, sin_u = grid.rotation(csi.Face, csi.Center)
print(f"{steps} steps of {dt:.0f} s on TripolarGrid(64 x 48) in {wall:.2f} s; path {model.ctx.last_path()}")
print(f"{maps} maps (two source grids x two locations), {launches} regridding launches for {len(model._series)} slots; "
      f"wind window: {model.time_series_status('TOP_U')}")
print(f"grid-x wind in [{ua.min():.2f}, {ua.max():.2f}] m/s; the cap turns x by up to {np.degrees(np.abs(np.arctan2(sin_u, cos_u))).max():.0f} degrees")
print(f"max |u| = {np.abs(u).max():.4f}, max |v| = {np.abs(v).max():.4f} m/s; everything finite: {bool(np.isfinite(u).all() and np.isfinite(v).all())}")
