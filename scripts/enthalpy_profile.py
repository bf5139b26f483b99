#!/usr/bin/env python3
"""Times the enthalpy-method column model's step kernel (csrc/enthalpy.hip) in its two forms:

  on_chip    k_enthalpy_steps<true>: the state of 64 columns per wave in LDS, n sub-steps per launch (n = 1, 8, 64 = the cap)
  per_step   k_enthalpy_steps<false>: one launch per step on the caller's arrays (CSI_ENTH_PATH=1 for the context)

Every figure is the wall time of `calls` time_steps(dt, n) calls followed by ONE wait for the stream, divided by calls * n: many
launches per measurement, `reps` measurements, median and spread (min .. max).  At these column counts a launch takes far longer than
its submission, so the host side does not show.  Per cell and step the per-step form moves 56 bytes at least (H, T, kappa read; H, T,
phi, kappa written) and both forms make three IEEE divisions.  One JSON line per configuration.

  python scripts/enthalpy_profile.py [--sizes 512,1024,2048] [--nz 20] [--deep 1024:64] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK = 8e12
BYTES_PER_CELL_STEP = 56


def measure(csi, np, N, Nz, n, forced, reps, target_cell_steps):
    os.environ["CSI_ENTH_PATH"] = str(forced)          # read when the model's context is created
    g = csi.ColumnGrid((N, N, Nz), z=(-1, 0))
    rng = np.random.default_rng(1)
    m = csi.EnthalpyMethodSeaIceModel(g, boundary_conditions=dict(T=csi.FieldBoundaryConditions(top=csi.ValueBoundaryCondition(-5.0),
                                                                                                 bottom=csi.ValueBoundaryCondition(1.1))))
    m.set(T=np.linspace(1.1, -4.0, Nz)[:, None, None] + rng.uniform(-0.5, 0.5, (Nz, N, N)))
    m.update_state()
    dt = 0.1 * g.minimum_zspacing() ** 2 / 1e-5
    calls = max(2, int(target_cell_steps / (N * N * Nz * n)))
    m.time_steps(dt, n)
    m.synchronize()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            m.time_steps(dt, n)
        m.synchronize()
        per.append((time.perf_counter() - t0) / (calls * n))
    ll = m.last_launch()
    med = statistics.median(per)
    cells = N * N * Nz
    out = dict(form=ll["form"], N=N, Nz=Nz, n=n, launches_per_call=ll["launches"], lds_bytes=ll["lds_bytes"], calls=calls, reps=reps,
               us_per_substep_median=round(med * 1e6, 2), us_min=round(min(per) * 1e6, 2), us_max=round(max(per) * 1e6, 2),
               gcell_steps_per_s=round(cells / med / 1e9, 2), gdivisions_per_s=round(3 * cells / med / 1e9, 1))
    if ll["form"] == "per_step":
        out["share_of_8_tb_per_s_at_56_b"] = round(BYTES_PER_CELL_STEP * cells / med / PEAK, 3)
    else:
        out["waves_per_cu"] = csi._lib.enthalpy_plan(Nz, forced)["waves_per_cu"]
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--nz", type=int, default=20)
    ap.add_argument("--deep", default="1024:64", help="N:Nz of the deep case")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--work", type=float, default=4e10, help="cell-steps per measurement (some tenths of a second each)")
    a = ap.parse_args()
    import numpy as np
    import climaseaice_jl_amd as csi
    cap = csi._lib.ENTH_MAX_SUBSTEPS
    cases = [(int(s), a.nz) for s in a.sizes.split(",") if s]
    if a.deep:
        cases.append(tuple(int(x) for x in a.deep.split(":")))
    for N, Nz in cases:
        print(json.dumps(measure(csi, np, N, Nz, 1, 1, a.reps, a.work)), flush=True)
        for n in sorted({1, 8, 64, cap}):
            print(json.dumps(measure(csi, np, N, Nz, n, 2, a.reps, a.work)), flush=True)


if __name__ == "__main__":
    main()
