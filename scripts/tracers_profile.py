"""What the advected tracers cost on the device (profiles/r30_tracers.md).  Needs the GPU.

    python scripts/tracers_profile.py [--sizes 2048,4096] [--out FILE.md]

On an N x N periodic uniform grid with the anticyclone's prescribed velocities, WENO7, FAST mode; every figure is the host clock around
`reps` back-to-back calls on the library's stream, closed by one wait, divided by reps (at these sizes a launch lasts 0.1 ms and more,
the launch overhead of a few microseconds is inside the figure) -- NOT a kernel trace.
  stencil   csi_tracers_tendencies for 1, 2, 4, 8 tracers, all plain or all weighted by concentration, with 1, 2 and 4 tracers per
            thread forced through CSI_TRACERS_NTR (read when the context is created), beside csi_compute_tracer_tendencies, the h + aice
            launch of k_tendencies, in the same process
  finish    csi_tracers_tendencies + csi_tracers_update minus the former: the point-wise launch, and its compulsory bytes -- 8 (c*) +
            8 (aice) + 8 (c) per cell and tracer -- as a share of 8 TB/s
  step      a whole RK3 time_step with and without csi.IceAge()
  host      the host route to an age: Field.numpy() of u, v, aice (a stream drain and three whole-parent copies) and one NumPy update
CSI_HIP_LIBRARY selects the build."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PEAK = 8.0e12


def model_of(N, n, weighted, ntr, stepper="SplitRungeKutta3"):
    import numpy as np
    import climaseaice_jl_amd as csi
    if ntr:
        os.environ["CSI_TRACERS_NTR"] = str(ntr)
    else:
        os.environ.pop("CSI_TRACERS_NTR", None)
    L = N * 1000.0
    g = csi.RectilinearGrid((N, N), x=(0.0, L), y=(0.0, L), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
    specs = [csi.Tracer(f"t{k}", weighting="concentration" if weighted else None) for k in range(n)] if n >= 0 else [csi.IceAge()]
    m = csi.SeaIceModel(g, dynamics=None, advection=csi.WENO(order=7), timestepper=stepper, mode="fast", tracers=specs)
    xf, yc = g.xnodes(csi.Face)[None, :], g.ynodes(csi.Center)[:, None]
    xc, yf = g.xnodes(csi.Center)[None, :], g.ynodes(csi.Face)[:, None]
    rng = np.random.default_rng(1)
    csi.set_(m, h=0.3 + 0.2 * rng.random((N, N)), aice=0.5 + 0.5 * rng.random((N, N)),
             u=0.5 * np.sin(2 * np.pi * yc / L) * np.cos(2 * np.pi * xf / L), v=-0.5 * np.sin(2 * np.pi * xc / L) * np.cos(2 * np.pi * yf / L),
             **{s.name: rng.random((N, N)) for s in specs})
    m.synchronize()
    return csi, m


def per_call(m, call, reps=20, warm=3):
    for _ in range(warm):
        call()
    m.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    m.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def main():
    sizes = [2048, 4096]
    out = None
    a = sys.argv[1:]
    while a:
        k = a.pop(0)
        if k == "--sizes":
            sizes = [int(x) for x in a.pop(0).split(",")]
        elif k == "--out":
            out = a.pop(0)
    rows = []
    for N in sizes:
        csi, m = model_of(N, 0, False, 0)
        rows.append(dict(N=N, what="k_tendencies h + aice", us=per_call(m, lambda: m.ctx.call("csi_compute_tracer_tendencies", 7)), layout=m.ctx.last_advection()))
        rows.append(dict(N=N, what="RK3 step, no tracers", us=per_call(m, lambda: csi.time_step(m, 120.0), reps=10)))
        t0 = time.perf_counter()
        u, v, aa = m.velocities.u.numpy(), m.velocities.v.numpy(), m.ice_concentration.numpy()
        age = (aa > 0) * (aa + 120.0)
        rows.append(dict(N=N, what="host route: numpy() of u, v, aice + one NumPy update", us=1e6 * (time.perf_counter() - t0)))
        print(json.dumps(rows[-3]), json.dumps(rows[-2]), json.dumps(rows[-1]), flush=True)
        del m, u, v, aa, age
        csi, m = model_of(N, -1, True, 0)
        rows.append(dict(N=N, what="RK3 step with csi.IceAge()", us=per_call(m, lambda: csi.time_step(m, 120.0), reps=10)))
        print(json.dumps(rows[-1]), flush=True)
        del m
        for n in (1, 2, 4, 8):
            for weighted in (False, True):
                for ntr in (1, 2, 4):
                    if ntr > n:
                        continue
                    csi, m = model_of(N, n, weighted, ntr)
                    m.ctx.call("csi_compute_tracer_tendencies", 7)
                    first = lambda: m.ctx.tracers_tendencies(7, 120.0, False)      # noqa: E731

                    def both():
                        m.ctx.tracers_tendencies(7, 120.0, False)
                        m.ctx.tracers_update(120.0)
                    t1 = per_call(m, first)
                    lay = m.ctx.tracers_last()
                    t2 = per_call(m, both)
                    fin = t2 - t1
                    share = (24.0 * N * N * n) / (fin * 1e-6) / PEAK if fin > 0 else float("nan")
                    rows.append(dict(N=N, what="stencil", n=n, weighted=weighted, ntr=lay["tracers_per_thread"], groups=lay["groups"], us=t1,
                                     us_per_tracer=t1 / n, finish_us=fin, finish_share_of_8TBs=share))
                    print(json.dumps(rows[-1]), flush=True)
                    del m
    if out:
        with open(out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
