"""The anticyclone case of examples/ice_advected_by_anticyclone.py with its force balance: the power of each term of the momentum
equation -- wind input, ocean drag, Coriolis, the work of the stress divergence, user forcing -- printed every ten steps, and maps of the
wind force, the ocean drag and the internal force on the ice (N m^-2, at the u and v points) written every five iterations, computed
on the device from the stepped state immediately before each record.  The last lines show what a coupler reads: the stress the ocean
receives.

    python examples/anticyclone_force_balance.py [N] [steps] [directory]       (needs the GPU)
"""
import sys, os, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
out = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="anticyclone_force_balance_")
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

dt = 600.0
names = ["top_x", "top_y", "bottom_x", "bottom_y", "internal_x", "internal_y"]
model.output_writers["forces"] = csi.OutputWriter(model, names, csi.IterationInterval(5), os.path.join(out, "forces"), overwrite_existing=True)
for n in range(steps):
    csi.time_step(model, dt)
    if (n + 1) % 10 == 0:
        b = model.momentum_budget()
        print(f"iteration {n + 1:4d}: wind {b.top: .4e} W, ocean drag {b.bottom: .4e} W, Coriolis {b.coriolis: .1e} W, "
              f"internal {b.internal: .4e} W, forcing {b.forcing: .1e} W, residual {b.residual: .4e} W")
model.output_writers["forces"].close()

rec = csi.load_output(os.path.join(out, "forces"))
print(f"{out}: {len(rec['time'])} records of {', '.join(names)}; top_x {rec['top_x'].shape[1:]}, top_y {rec['top_y'].shape[1:]}")
print(f"last record: t = {rec['time'][-1] / 3600:.2f} h, max |wind force| = {np.abs(rec['top_x'][-1]).max():.4f} N m^-2, "
      f"max |ocean drag| = {np.abs(rec['bottom_x'][-1]).max():.4f} N m^-2, max |internal force| = {np.abs(rec['internal_x'][-1]).max():.4f} N m^-2")
# what the ocean reads every coupling step: -BOTTOM, the drag on the ice per unit area of the cell, with its sign turned
bx, by = model.compute_momentum_terms("bottom")
model.synchronize()
print(f"stress on the ocean: x in [{(-bx.interior_numpy()).min():.4f}, {(-bx.interior_numpy()).max():.4f}] N m^-2, "
      f"y in [{(-by.interior_numpy()).min():.4f}, {(-by.interior_numpy()).max():.4f}] N m^-2")
