"""The advection-only anticyclone case (tests/test_gpu_steps.py anticyclone_case; examples/ice_advected_by_anticyclone.py's family) with two
advected tracers: a dye that marks the thick ice of the initial state, and the age of the ice.  Both are stepped on the device inside every
time_step, with the velocities, scheme and mode of h (include/csi.h, "advected ice tracers and ice age"); the age is written every ten
iterations.  The run checks the invariant 0 <= age <= t after every step, to the 3e-7 per RK3 step by which WENO-Z's eps may let a
uniform age drift (include/csi.h).

    python examples/anticyclone_with_ice_age.py [N] [steps] [directory]       (needs the GPU)
"""
import sys, os, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import climaseaice_jl_amd as csi

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
out = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="anticyclone_ice_age_")
L = N * 1000.0
grid = csi.RectilinearGrid((N, N), x=(0.0, L), y=(0.0, L), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
xf, yc = grid.xnodes(csi.Face)[None, :], grid.ynodes(csi.Center)[:, None]
xc, yf = grid.xnodes(csi.Center)[None, :], grid.ynodes(csi.Face)[:, None]
V = 0.5
u = V * np.sin(2 * np.pi * yc / L) * np.cos(2 * np.pi * xf / L)
v = -V * np.sin(2 * np.pi * xc / L) * np.cos(2 * np.pi * yf / L)
X, Y = np.meshgrid(grid.xnodes(csi.Center), grid.ynodes(csi.Center))
h = 0.3 + 0.2 * np.exp(-((X - L / 3) ** 2 + (Y - L / 2) ** 2) / (L / 20) ** 2)
aice = np.clip(1 - 0.1 * np.random.default_rng(2).random((N, N)), 0, 1)
aice[N // 4:N // 3, N // 4:N // 3] = 0.0          # open water: the age stays zero until ice is carried in
h[N // 4:N // 3, N // 4:N // 3] = 0.0

model = csi.SeaIceModel(grid, dynamics=None, advection=csi.WENO(order=7), timestepper="SplitRungeKutta3",
                        tracers=("dye", csi.IceAge(units="days")))
csi.set_(model, h=h, aice=aice, u=u, v=v, dye=(h > 0.35).astype(float))
model.output_writers["age"] = csi.OutputWriter(model, ["age", "dye", "aice"], csi.IterationInterval(10), os.path.join(out, "fields"),
                                               overwrite_existing=True)
dt = 120.0
for n in range(steps):
    csi.time_step(model, dt)
    model.synchronize()
    age = model.tracer("age").interior_numpy()
    days = model.clock.time / 86400.0
    assert age.min() >= 0.0 and age.max() <= days * (1 + 3e-7 * (n + 1)), (n, age.min(), age.max(), days)
model.output_writers["age"].close()

a = model.ice_concentration.interior_numpy()
filled = (aice == 0) & (a > 0)
print(f"{out}: after {model.clock.time / 3600:.2f} h the oldest ice is {age.max() * 24:.2f} h old (the run: {days * 24:.2f} h); "
      f"{int(filled.sum())} cells of the open-water patch hold ice now, mean age {24 * age[filled].mean() if filled.any() else 0.0:.2f} h; "
      f"dye: {model.tracer('dye').interior_numpy().sum():.3f} (start {float((h > 0.35).sum()):.3f}); "
      f"launches (stencil, point-wise): {model.ctx.tracers_stats()}, layout {model.ctx.tracers_last()}")
