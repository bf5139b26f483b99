"""The anticyclone case of examples/ice_advected_by_anticyclone.py with deformation maps: shear and divergence (and h) every five
iterations, computed on the device from the stepped state immediately before each record, and the discrete energy budget of the stress
divergence (test/test_rheology_energy_budget.jl) printed along the way.

    python examples/anticyclone_with_deformation.py [N] [steps] [directory]       (needs the GPU)
"""
import sys, os, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
out = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="anticyclone_deformation_")
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
model.output_writers["deformation"] = csi.OutputWriter(model, ["h", "shear", "divergence"], csi.IterationInterval(5),
                                                       os.path.join(out, "deformation"), overwrite_existing=True)
for n in range(steps):
    csi.time_step(model, dt)
    if (n + 1) % 10 == 0:
        b = model.energy_budget()
        print(f"iteration {n + 1:4d}: work of the stress divergence {b.internal_work: .6e} W, stress power {b.stress_power: .6e} W, "
              f"imbalance {b.imbalance:.1e}, kinetic energy {b.kinetic_energy:.6e} J")
model.output_writers["deformation"].close()

rec = csi.load_output(os.path.join(out, "deformation"))
day = 86400.0
print(f"{out}: {len(rec['time'])} records of h, shear, divergence {rec['shear'].shape[1:]} at iterations {list(rec['iteration'][:4])} ...")
print(f"last record: t = {rec['time'][-1] / 3600:.2f} h, max shear = {rec['shear'][-1].max() * day:.4f} / day, "
      f"divergence in [{rec['divergence'][-1].min() * day:.4f}, {rec['divergence'][-1].max() * day:.4f}] / day")
