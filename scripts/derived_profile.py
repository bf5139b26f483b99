"""What the derived fields and the energy budget cost on the device, and what the same quantities cost through the host.  Needs the GPU.

    python scripts/derived_profile.py [sizes, default 2048,4096]        one child process per measurement, each under its own time
                                                                        limit; stops at the first failure
    python scripts/derived_profile.py --child kernels|host N            one measurement (also what to put behind `rocprofv3
                                                                        --kernel-trace --stats --` for the kernels' device times)

kernels  the benchmark's model (EVP, 120 sub-steps, WENO7, periodic uniform grid) after one RK3 step.  Host clock around batches of 16
         csi_derived_compute calls that end in a wait for the context's stream -- an upper bound of the kernel time, launch gaps included
         -- for three masks: shear + divergence, the four strain-group fields, all seven; compulsory bytes per cell: u, v once (16 B),
         with the stress group sigma11, sigma22, sigma12, P once (32 B), 8 B per field written; against 8 TB/s.  The whole call of
         csi_budget_compute (two launches, a 24-byte copy, the wait), per group: u, v, sigma (40 B per cell), + h, aice (56 B).
host     the same quantities the only way there was before: Field.numpy() of u, v (and sigma, P), then the NumPy restatement of
         tests/derived_ref.py for shear + divergence, for all seven and for the budget sums.  One repeat (seconds at 4096^2).
Prints one JSON line per measurement."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PEAK = 8.0e12      # B/s: HBM (MI355X)
LIMITS = {"kernels": 240, "host": 420}


def make_model(N):
    import numpy as np
    import climaseaice_jl_amd as csi
    L = 2000.0 * N
    g = csi.RectilinearGrid((N, N), x=(0.0, L), y=(0.0, L), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
    dyn = csi.SeaIceMomentumEquation(g, coriolis=csi.FPlane(f=1e-4), rheology=csi.ElastoViscoPlasticRheology(), top_momentum_stress=(0.05, 0.02),
                                     bottom_momentum_stress=csi.SemiImplicitStress(), solver=csi.SplitExplicitSolver(substeps=120))
    m = csi.SeaIceModel(g, dynamics=dyn, advection=csi.WENO(order=7), timestepper="SplitRungeKutta3")
    rng = np.random.default_rng(1)
    x = (np.arange(N) + 0.5) / N
    csi.set_(m, h=0.3 + 0.05 * np.sin(6.28 * x)[None, :] * np.cos(6.28 * x)[:, None] + 0.01 * rng.random((N, N)), aice=0.9 + 0.1 * rng.random((N, N)),
             u=0.01 * rng.standard_normal((N, N)), v=0.01 * rng.standard_normal((N, N)))
    csi.time_step(m, 120.0)
    m.synchronize()
    return csi, m


def spread(ts):
    ts = sorted(ts)
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1], reps=len(ts))


MASKS = {"shear_divergence": (("shear", "divergence"), 16 + 2 * 8), "strain_group": (("divergence", "shear", "deformation", "speed"), 16 + 4 * 8),
         "all_seven": (("divergence", "shear", "deformation", "speed", "sigma_I", "sigma_II", "stress_power"), 48 + 7 * 8)}


def child_kernels(N, batches=7, calls=16):
    csi, m = make_model(N)
    from climaseaice_jl_amd.derived import mask_of
    cells = N * N
    out = dict(measure="kernels", N=N, cells=cells)
    for name, (fields, per) in MASKS.items():
        for f in fields:
            m.derived_field(f)
        mask = mask_of(fields)
        ts = []
        for b in range(batches + 2):
            m.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                m.ctx.derived_compute(mask)
            m.synchronize()
            if b >= 2:
                ts.append((time.perf_counter() - t0) / calls)
        r = spread(ts)
        r.update(bytes=per * cells, floor_ms=1e3 * per * cells / PEAK, share_of_8TBs=per * cells / PEAK / (1e-3 * r["median_ms"]))
        out[name] = r
    for what, per in (("stress", 40), ("kinetic", 32), ("all", 56)):
        ts = []
        for b in range(batches + 2):
            m.synchronize()
            t0 = time.perf_counter()
            m.energy_budget(what)
            if b >= 2:
                ts.append(time.perf_counter() - t0)
        r = spread(ts)
        r.update(bytes=per * cells, floor_ms=1e3 * per * cells / PEAK, share_of_8TBs=per * cells / PEAK / (1e-3 * r["median_ms"]))
        out["budget_" + what] = r
    b = m.energy_budget()
    out["budget"] = dict(internal_work=b.internal_work, stress_power=b.stress_power, imbalance=b.imbalance, kinetic_energy=b.kinetic_energy)
    print(json.dumps(out), flush=True)


def child_host(N):
    csi, m = make_model(N)
    import derived_ref as ref
    f = m.dynamics.auxiliaries.fields
    fields = {"u": m.velocities.u, "v": m.velocities.v, "s11": f.s11, "s22": f.s22, "s12": f.s12, "P": f.P, "h": m.ice_thickness,
              "a": m.ice_concentration}
    out = dict(measure="host", N=N)
    for name, need, work in (("shear_divergence", ("u", "v"), lambda r: r.fields(("shear", "divergence"))),
                             ("all_seven", ("u", "v", "s11", "s22", "s12", "P"), lambda r: r.fields()),
                             ("budget_all", tuple(fields), lambda r: r.budget())):
        m.synchronize()
        t0 = time.perf_counter()
        par = {k: fields[k].numpy() for k in need}
        t1 = time.perf_counter()
        work(ref.Ref(m.grid, par, None, rho=m.sea_ice_density))
        t2 = time.perf_counter()
        out[name] = dict(download_ms=1e3 * (t1 - t0), numpy_ms=1e3 * (t2 - t1), total_ms=1e3 * (t2 - t0))
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        {"kernels": child_kernels, "host": child_host}[sys.argv[2]](int(sys.argv[3]))
        return 0
    sizes = [int(s) for s in (sys.argv[1] if len(sys.argv) > 1 else "2048,4096").split(",")]
    for N in sizes:
        for what in ("kernels", "host"):
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(N)], timeout=LIMITS[what]).returncode
            except subprocess.TimeoutExpired:
                print(f"derived_profile: {what} at {N} ran into its time limit; stopping", flush=True)
                return 124
            if rc != 0:
                print(f"derived_profile: {what} at {N} failed with status {rc}; stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
