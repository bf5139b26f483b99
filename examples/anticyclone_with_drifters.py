"""The anticyclone case of examples/ice_advected_by_anticyclone.py with Lagrangian drifters: one drifter at the centre of every fourth
cell in each direction, advected on the device after every step with the velocities the step leaves (one launch, two midpoint sub-steps),
their tracks -- position, the ice velocity and thickness under them -- written every five iterations as growable .npy files.

    python examples/anticyclone_with_drifters.py [N] [steps] [directory]       (needs the GPU)
"""
import sys, os, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
out = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="anticyclone_drifters_")
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

model.drifters = csi.Drifters.at_cell_centers(grid, stride=4, substeps=2)
model.output_writers["tracks"] = csi.DrifterWriter(model.drifters, csi.IterationInterval(5), os.path.join(out, "tracks"),
                                                   columns=("xi", "eta", "u", "v", "h"), overwrite_existing=True)
dt = 600.0
for n in range(steps):
    csi.time_step(model, dt)
model.output_writers["tracks"].close()

tracks = csi.load_tracks(os.path.join(out, "tracks"))
x0, y0 = tracks["xi"][0] * grid.dx, tracks["eta"][0] * grid.dy
x1, y1 = tracks["xi"][-1] * grid.dx, tracks["eta"][-1] * grid.dy
drift = np.hypot(x1 - x0, y1 - y0)
print(f"{out}: {tracks['xi'].shape[0]} records of {model.drifters.n} drifters at iterations {list(tracks['iteration'][:4])} ...")
print(f"after {tracks['time'][-1] / 3600:.2f} h: mean drift {drift.mean():.1f} m, largest {drift.max():.1f} m; speed under the fastest "
      f"{np.hypot(tracks['u'][-1], tracks['v'][-1]).max():.4f} m/s; status {model.drifters.status_counts(model)}")
