"""What an output record costs the stepping thread, what the two output kernels take and how fast a record crosses the bus.  Needs the GPU.

    python scripts/output_profile.py [sizes, default 2048,4096]          one child process per measurement, each under its own time
                                                                         limit; stops at the first failure
    python scripts/output_profile.py --child steps|kernels|copy N        one measurement (also what to put behind `rocprofv3
                                                                         --kernel-trace --stats --` for the kernels' device times)

steps    wall time of 20 RK3 steps (EVP, 120 sub-steps, WENO7; the benchmark's model) ending in a device synchronise, three ways,
         alternating, five repeats: no output; an OutputWriter for h, aice, u, v in fp32 with IterationInterval(5) (records at
         iterations 0, 5, 10, 15, 20: five records, all drained and written to files inside the timed window); the same records taken the
         only way there was before -- Field.interior_numpy() per field, converted to fp32 on the host, kept in memory (no file is written:
         the comparison favours this way).  Per record = (with - without) / 5.  The writer's host part (waiting for the slot, file write)
         is timed by itself.
kernels  host clock around batches of csi_output_accumulate / csi_output_snapshot calls that end in a wait for the context's stream (the
         copies run on the copy stream and are not waited for); compulsory bytes per element: pack to fp32 12 B, to fp64 16 B,
         accumulate 24 B, against 8 TB/s.  An upper bound of the kernel time (launch gaps included).
copy     snapshot -> csi_output_wait of one record, minus nothing: pack launch + copy; bytes over that time against the 63 GB/s link.
Prints one JSON line per measurement."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
PEAK, LINK = 8.0e12, 63.0e9      # B/s: HBM, host link (MI355X)
NAMES = ["h", "aice", "u", "v"]
LIMITS = {"steps": 420, "kernels": 180, "copy": 120}


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
    return csi, m


def spread(ts):
    ts = sorted(ts)
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1], reps=len(ts))


def child_steps(N, steps=20, every=5, reps=5):
    import numpy as np
    csi, m = make_model(N)
    dt = 120.0
    tmp = tempfile.mkdtemp(prefix="output_profile_")
    host = {"t": 0.0}

    def run(kind, rep):
        m.output_writers.clear()
        m.clock.iteration, m.clock.time = 0, 0.0
        kept = []
        w = None
        t0 = time.perf_counter()
        if kind == "writer":
            w = csi.OutputWriter(m, NAMES, csi.IterationInterval(every), os.path.join(tmp, f"w{rep}"), dtype="f32", slots=2)
            m.output_writers["w"] = w
            drain = w._drain_one

            def timed_drain():
                a = time.perf_counter()
                drain()
                host["t"] += time.perf_counter() - a
            w._drain_one = timed_drain
        t_create = time.perf_counter() - t0
        t0 = time.perf_counter()
        for k in range(steps + 1):
            if kind == "numpy" and k % every == 0:
                kept.append([csi.bound_fields(m)[n][0].interior_numpy().astype(np.float32) for n in NAMES])
            if k < steps:
                csi.time_step(m, dt)
        if w is not None:
            w.close()
        m.synchronize()
        return time.perf_counter() - t0, t_create

    for kind in ("none", "writer", "numpy"):       # warm-up of every way
        run(kind, "warm_" + kind)
    ts = {"none": [], "writer": [], "numpy": []}
    host["t"] = 0.0
    for rep in range(reps):
        for kind in ts:
            ts[kind].append(run(kind, rep)[0])
    records = steps // every + 1
    out = dict(measure="steps", N=N, steps=steps, records=records, record_MB=4 * N * N * 4 / 1e6,
               none=spread(ts["none"]), writer=spread(ts["writer"]), numpy=spread(ts["numpy"]))
    out["step_ms"] = out["none"]["median_ms"] / steps
    for kind in ("writer", "numpy"):
        out[kind + "_per_record_ms"] = (out[kind]["median_ms"] - out["none"]["median_ms"]) / records
    out["writer_host_part_per_record_ms"] = 1e3 * host["t"] / (reps * records)      # waiting for the slot + writing the files
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out), flush=True)


def child_kernels(N, batches=7):
    csi, m = make_model(N)
    L = csi._lib
    slots = {n: csi.bound_fields(m)[n][1] for n in NAMES}
    cells = 4 * N * N
    out = dict(measure="kernels", N=N, elements=cells)
    for name, dtype, avg, per in (("pack_f32", L.OUT_F32, 0, 12), ("pack_f64", L.OUT_F64, 0, 16), ("accumulate", L.OUT_F32, 1, 24)):
        nslots = 4
        h = m.ctx.output_create([(slots[n], dtype, avg, 0, 0.0) for n in NAMES], nslots)
        ts = []
        for b in range(batches + 2):
            m.synchronize()
            t0 = time.perf_counter()
            if avg:
                for _ in range(16):
                    m.ctx.output_accumulate(h, 1.0)
                calls = 16
            else:
                taken = [m.ctx.output_snapshot(h) for _ in range(nslots)]
                calls = nslots
            m.synchronize()                  # the context's stream: the launches, not the copies
            t = (time.perf_counter() - t0) / calls
            if not avg:
                for s in taken:
                    m.ctx.output_release(h, s)
            if b >= 2:
                ts.append(t)
        if avg:                              # (what a pack launch of averaged fields takes: it reads and clears the accumulators)
            m.ctx.output_release(h, m.ctx.output_snapshot(h))
        m.ctx.output_destroy(h)
        r = spread(ts)
        r.update(bytes=per * cells, floor_ms=1e3 * per * cells / PEAK, share_of_8TBs=per * cells / PEAK / (1e-3 * r["median_ms"]))
        out[name] = r
    print(json.dumps(out), flush=True)


def child_copy(N, reps=9):
    csi, m = make_model(N)
    L = csi._lib
    h = m.ctx.output_create([(csi.bound_fields(m)[n][1], L.OUT_F32, 0, 0, 0.0) for n in NAMES], 1)
    nbytes = m.ctx.output_record_bytes(h)
    ts = []
    for r in range(reps + 2):
        m.synchronize()
        t0 = time.perf_counter()
        s = m.ctx.output_snapshot(h)
        t_call = time.perf_counter() - t0
        m.ctx.output_wait(h, s)
        t = time.perf_counter() - t0
        m.ctx.output_release(h, s)
        if r >= 2:
            ts.append((t, t_call))
    m.ctx.output_destroy(h)
    out = dict(measure="copy", N=N, record_bytes=nbytes, snapshot_to_wait=spread([t for t, _ in ts]), snapshot_call=spread([c for _, c in ts]))
    out["GB_per_s"] = nbytes / (1e-3 * out["snapshot_to_wait"]["median_ms"]) / 1e9
    out["share_of_link"] = out["GB_per_s"] * 1e9 / LINK
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        {"steps": child_steps, "kernels": child_kernels, "copy": child_copy}[sys.argv[2]](int(sys.argv[3]))
        return 0
    sizes = [int(s) for s in (sys.argv[1] if len(sys.argv) > 1 else "2048,4096").split(",")]
    for N in sizes:
        for what in ("kernels", "copy", "steps"):
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(N)], timeout=LIMITS[what]).returncode
            except subprocess.TimeoutExpired:
                print(f"output_profile: {what} at {N} ran into its time limit; stopping", flush=True)
                return 124
            if rc != 0:
                print(f"output_profile: {what} at {N} failed with status {rc}; stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
