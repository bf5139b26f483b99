#!/usr/bin/env python3
"""Times the ViscousRheology split-explicit sub-cycle (two launches per sub-step, csrc/momentum_viscous.hip) on bench.py's workload:
the 2048 x 2048 periodic f-plane grid (cases.make_case as bench.py builds it), STRICT and FAST.

Per mode: device time of the sub-step loop from the context's HIP events (csi_last_subcycle_ms, recorded around the launches of one
time_step_momentum! call), the median over --reps calls after --warmup; us per sub-step, cell-updates/s and the fraction of a
compulsory-bytes roofline: per launch every point reads u, v, h, aice and writes its component -- 5 x 8 B per cell per launch,
80 B per cell per sub-step -- against 8 TB/s (HBM peak) and against the 6.3 TB/s copy rate of MI355X_MICROARCH-style measurements.
The shader clock is sampled beside a repetition of the timed loop (bench.ClockSampler).  Prints one JSON line.

  python scripts/viscous_subcycle_bench.py [--n 2048] [--substeps 120] [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

BYTES_PER_CELL_SUBSTEP = 80.0      # two launches x (u, v, h, aice read + one component written) x 8 B
HBM_PEAK, COPY_RATE = 8.0e12, 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--substeps", type=int, default=120)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nu", type=float, default=1000.0)
    a = ap.parse_args()
    import numpy as np
    import cases
    import climaseaice_jl_amd as csi
    from bench import ClockSampler

    n, sub = a.n, a.substeps
    out = {"workload": f"viscous_subcycle_fplane_periodic_{n}x{n}_{sub}substeps", "bytes_per_cell_substep": BYTES_PER_CELL_SUBSTEP}
    for mode in ("strict", "fast"):
        c = cases.make_case(Nx=n, Ny=n, substeps=sub, topo=("periodic", "periodic"), patches=True, random_uv=0.02)
        orig = csi.SeaIceMomentumEquation
        csi.SeaIceMomentumEquation = lambda g, **k: orig(g, **dict(k, rheology=csi.ViscousRheology(nu=a.nu)))
        try:
            m = cases.csi_model(c, mode=mode)
        finally:
            csi.SeaIceMomentumEquation = orig
        for _ in range(a.warmup):
            csi.time_step_momentum(m, c["dt"])
        ms = []
        for _ in range(a.reps):
            csi.time_step_momentum(m, c["dt"])
            m.synchronize()
            ms.append(m.ctx.last_subcycle_ms())
        with ClockSampler(m.device.index or 0) as clk:
            for _ in range(a.reps):
                csi.time_step_momentum(m, c["dt"])
            m.synchronize()
        launches, substeps = m.ctx.last_launches()
        t = float(np.median(ms)) * 1e-3 / sub          # seconds per sub-step
        u = m.velocities.u.interior_numpy()
        out[mode] = {"us_per_substep": t * 1e6, "cell_updates_per_s": n * n / t,
                     "roofline_fraction_8TBs": n * n * BYTES_PER_CELL_SUBSTEP / t / HBM_PEAK,
                     "roofline_fraction_copy_6p3TBs": n * n * BYTES_PER_CELL_SUBSTEP / t / COPY_RATE,
                     "launches": launches, "substeps": substeps, "ms_samples": ms, "finite": bool(np.all(np.isfinite(u))),
                     "clock": clk.summary()}
        m.ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
