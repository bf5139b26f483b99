"""The anticyclone case of examples/ice_advected_by_anticyclone.py with the reference example's output: h, aice, u, v every five
iterations (examples/ice_advected_by_anticyclone.jl:161-163, JLD2Writer with IterationInterval(5)) plus a daily average of h and aice.
Records are packed on the device and cross the bus while the model steps on; the files are growable .npy files.

    python examples/anticyclone_with_output.py [N] [steps] [directory]       (needs the GPU)
"""
import sys, os, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
out = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="anticyclone_output_")
L = 512e3
grid = csi.RectilinearGrid((N, N), x=(0.0, L), y=(0.0, L), topology=(csi.Bounded, csi.Bounded), halo=(4, 4))
xu, yu = grid.xnodes(csi.Face)[None, :], grid.ynodes(csi.Center)[:, None]
xv, yv = grid.xnodes(csi.Center)[None, :], grid.ynodes(csi.Face)[:, None]
tau0 = 0.1
dyn = csi.SeaIceMomentumEquation(grid, coriolis=csi.FPlane(f=1e-4), rheology=csi.ElastoViscoPlasticRheology(),
                                 top_momentum_stress=(-tau0 * (2 * yu - L) / L + 0 * xu, tau0 * (2 * xv - L) / L + 0 * yv),
                                 bottom_momentum_stress=csi.SemiImplicitStress(), solver=csi.SplitExplicitSolver(substeps=120))
model = csi.SeaIceModel(grid, dynamics=dyn, advection=csi.WENO(order=7), timestepper="SplitRungeKutta3")
xc, yc = grid.xnodes(csi.Center)[None, :], grid.ynodes(csi.Center)[:, None]
csi.set_(model, h=0.3 + 0.005 * (np.sin(60 * xc / 1000e3) + np.sin(30 * yc / 1000e3)), aice=np.ones((N, N)), u=0.0, v=0.0)

dt, day = 600.0, 86400.0
model.output_writers["fields"] = csi.OutputWriter(model, ["h", "aice", "u", "v"], csi.IterationInterval(5), os.path.join(out, "fields"),
                                                  overwrite_existing=True)
model.output_writers["daily"] = csi.OutputWriter(model, {"h": model.ice_thickness, "aice": model.ice_concentration},
                                                 csi.AveragedTimeInterval(day), os.path.join(out, "daily"), dtype="f64", overwrite_existing=True)
for n in range(steps):
    csi.time_step(model, csi.aligned_time_step(model, dt))        # lands on the ends of the averaging windows
for w in model.output_writers.values():
    w.close()

fields, daily = csi.load_output(os.path.join(out, "fields")), csi.load_output(os.path.join(out, "daily"))
print(f"{out}: {len(fields['time'])} records of h, aice, u, v {fields['h'].shape[1:]} / {fields['u'].shape[1:]} at iterations "
      f"{list(fields['iteration'][:4])} ...; {len(daily['time'])} daily average(s)")
print(f"last record: t = {fields['time'][-1] / 3600:.2f} h, max |u| = {np.abs(fields['u'][-1]).max():.4f} m/s, mean h = {fields['h'][-1].mean():.4f} m")
