"""Seasonal ice in both hemispheres of a small TripolarGrid, with the numbers people report for such a run: Arctic and Antarctic ice
extent and volume, written as a series while the model steps.  The hemispheres are a csi.Regions map; every record is one
csi_regions_compute call -- two launches and a copy of a few hundred bytes --, no field is copied to the host and the sums come in the
library's reproducible order.

    python examples/tripolar_hemispheres.py [hours] [output directory]       (needs the GPU)
"""
import sys, os, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

hours = float(sys.argv[1]) if len(sys.argv) > 1 else 6.0
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(tempfile.mkdtemp(), "hemispheres")
dt = 600.0
grid = csi.TripolarGrid((64, 48), southernmost_latitude=-80.0, halo=(4, 4))
wet = grid.analytic_land()
_, lat = grid.nodes_2d(csi.Center, csi.Center)

dyn = csi.SeaIceMomentumEquation(grid, coriolis=csi.PointwiseCoriolis(*grid.coriolis_planes()), rheology=csi.ElastoViscoPlasticRheology(),
                                 top_momentum_stress=(0.08, 0.03), bottom_momentum_stress=csi.SemiImplicitStress(),
                                 solver=csi.SplitExplicitSolver(substeps=60))
model = csi.SeaIceModel(grid, dynamics=dyn, advection=csi.WENO(order=7), timestepper="SplitRungeKutta3")
model.set_mask(wet)
# the season: a thick, compact Arctic pack north of 65 N, thin marginal Antarctic ice south of 62 S, open water between
arctic, antarctic = wet & (lat > 65.0), wet & (lat < -62.0)
csi.set_(model, h=np.where(arctic, 2.0, np.where(antarctic, 0.6, 0.0)), aice=np.where(arctic, 0.95, np.where(antarctic, 0.5, 0.0)))

hemispheres = csi.Regions.hemispheres(grid)                      # "south" / "north" by the sign of the cell-centre latitude
model.output_writers["hemispheres"] = csi.RegionalSeriesWriter(hemispheres, csi.IterationInterval(6), out, extent_threshold=0.15)
steps = int(hours * 3600 / dt)
t0 = time.perf_counter()
for _ in range(steps):
    csi.time_step(model, dt)
model.synchronize()
wall = time.perf_counter() - t0
model.output_writers["hemispheres"].close()

series = csi.load_regional_series(out)
now = model.regional_diagnostics(hemispheres)
whole = model.diagnostics("tracers")
print(f"{steps} steps of {dt:.0f} s on TripolarGrid(64 x 48) in {wall:.2f} s; {len(series['time'])} records in {out}")
print("   time [h]   " + "   ".join(f"{n:>5} extent [1e12 m2]  volume [1e12 m3]" for n in series["names"]))
for k, t in enumerate(series["time"]):
    print(f"   {t / 3600:8.2f}   " + "   ".join(f"{series['ice_extent'][k, r] / 1e12:24.6f}  {series['ice_volume'][k, r] / 1e12:16.6f}" for r in range(2)))
print(f"now: north {now['north']['cells']} cells, max h {now['north']['max_h']:.3f} m; south {now['south']['cells']} cells, max h {now['south']['max_h']:.3f} m; "
      f"unassigned {now.unassigned_cells}")
print(f"both hemispheres' cells are all the active cells: {int(now.cells.sum())} == {whole.active_cells}; "
      f"volume north + south = {now.ice_volume.sum():.6e}, whole grid {whole.ice_volume:.6e} (another tree over the same terms)")
print(f"launches made by the regional reduction: {model.ctx.regions_stats()}")
