"""The anticyclone case of examples/ice_advected_by_anticyclone.py run under a TimeStepWizard, with progress lines and a volume series
that never copy a field: every number below comes from model.diagnostics() -- two launches and a 168-byte copy per call.

    python examples/anticyclone_with_wizard.py [N] [steps]       (needs the GPU)
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
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

wizard = csi.TimeStepWizard(cfl=0.2, max_change=1.1, min_change=0.5, max_dt=600.0)
dt = 120.0
V0 = model.diagnostics("tracers").ice_volume
print(f"{'iter':>5} {'time [h]':>9} {'dt [s]':>8} {'max|u|':>9} {'max|v|':>9} {'max h':>8} {'volume [km^3]':>14} {'drift':>10}")
for n in range(steps):
    csi.time_step(model, dt)
    if (n + 1) % 5 == 0:
        csi.assert_finite(model)                 # raises, naming the fields, before a NaN spreads
        d = model.diagnostics()
        print(f"{model.clock.iteration:5d} {model.clock.time / 3600:9.3f} {dt:8.2f} {d.max_abs_u:9.5f} {d.max_abs_v:9.5f} {d.max_h:8.4f} "
              f"{d.ice_volume / 1e9:14.6f} {(d.ice_volume - V0) / V0:10.2e}")
        dt = wizard(model, dt)                   # every few iterations, as a TimeStepWizard callback does
print(f"advection timescale {csi.cell_advection_timescale(model):.1f} s; ice extent {model.diagnostics('tracers').ice_extent / 1e6:.0f} km^2")
