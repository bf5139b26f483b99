"""What the Lagrangian drifters cost on the device, beside an RK3 step and beside the host route.  Needs the GPU.

    python scripts/drifters_profile.py [--out FILE.md] [--N 2048]     one child process per measurement, each under its own time limit;
                                                                      stops at the first failure; the table of profiles/r28_drifters.md
                                                                      goes to FILE.md (and to the standard output)
    python scripts/drifters_profile.py --child headline|per_point|host N     one measurement, one JSON line

headline   the benchmark's model (EVP, 120 sub-steps, WENO7, N x N periodic uniform grid, f-plane) after one RK3 step: the wall time of an
           RK3 step (3 repeats), then csi_drifters_advance for n = 2^14, 2^20 and N^2 drifters seeded at cell centres (strides N / 128,
           N / 1024, 1), m = 1 and 4 sub-steps, the list in grid order and in a random permutation.  Host clock around batches of 32 calls
           that end in a wait for the context's stream -- an upper bound of the kernel time, launch gaps included (at 2^14 drifters it IS
           the launch rate); median and spread of 5 batches after 2 warm-up batches.  Then a DrifterWriter's record (the sample launch, the
           wait, the synchronous copy, the file appends) for 2^14 and 2^20 drifters.
per_point  the same advances on the same grid given by twelve per-point metric planes (CSI_METRIC_FULL): sixteen loads per rate evaluation
           instead of eight.  A model without dynamics; u, v smooth fields.
host       what there was before: Field.numpy() of u and v (a stream drain and two whole-parent copies), then the NumPy restatement
           tests/drifters_ref.py for N^2 drifters, one sub-step.  One repeat.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
LIMITS = {"headline": 300, "per_point": 240, "host": 300}
DT = 120.0


def headline_model(N):
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
    csi.time_step(m, DT)
    m.synchronize()
    return csi, m


def per_point_model(N):
    import numpy as np
    import climaseaice_jl_amd as csi
    L = 2000.0 * N
    g = csi.RectilinearGrid((N, N), x=(0.0, L), y=(0.0, L), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
    g = csi.OrthogonalCurvilinearGrid.from_grid(g, distort=0.1, seed=2)
    m = csi.SeaIceModel(g, timestepper="ForwardEuler")
    x = (np.arange(N) + 0.5) / N
    csi.set_(m, u=0.1 * np.sin(6.28 * x)[None, :] * np.cos(12.56 * x)[:, None], v=0.1 * np.cos(6.28 * x)[None, :] * np.sin(6.28 * x)[:, None])
    m.synchronize()
    return csi, m


def spread(ts):
    ts = sorted(ts)
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1], reps=len(ts))


def advances(csi, m, N, batches=5, calls=32):
    import numpy as np
    rows = []
    for n_name, stride in (("2^14", N // 128), ("2^20", N // 1024), ("N^2", 1)):
        base = csi.Drifters.at_cell_centers(m.grid, stride=stride)
        xi0, eta0, _ = base.numpy()
        perm = np.random.default_rng(0).permutation(xi0.size)
        for order, (xi, eta) in (("grid", (xi0, eta0)), ("shuffled", (xi0[perm], eta0[perm]))):
            for msub in (1, 4):
                d = csi.Drifters(m.grid, xi, eta, device=m.device)
                ts = []
                for b in range(batches + 2):
                    m.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        d.advance(m, DT, msub)
                    m.synchronize()
                    if b >= 2:
                        ts.append((time.perf_counter() - t0) / calls)
                r = spread(ts)
                r.update(n=int(xi0.size), n_name=n_name, order=order, substeps=msub,
                         drifter_substeps_per_s=xi0.size * msub / (1e-3 * r["median_ms"]), status=d.status_counts(m))
                rows.append(r)
    return rows


def writer_records(csi, m, N, reps=5):
    """A DrifterWriter's record -- the sample launch, the wait, the synchronous copy of five columns and the status, six file appends --
    for 2^14 and 2^20 drifters: wall time per record."""
    import tempfile
    rows = []
    for n_name, stride in (("2^14", N // 128), ("2^20", N // 1024)):
        d = csi.Drifters.at_cell_centers(m.grid, stride=stride)
        with tempfile.TemporaryDirectory() as tmp:
            w = csi.DrifterWriter(d, csi.IterationInterval(1), os.path.join(tmp, "tracks"), columns=("xi", "eta", "u", "v", "h"))
            ts = []
            for k in range(reps + 1):
                m.synchronize()
                t0 = time.perf_counter()
                w.write(m)
                if k:
                    ts.append(time.perf_counter() - t0)
            w.close()
        r = spread(ts)
        r.update(n=d.n, n_name=n_name, bytes=d.n * 44)
        rows.append(r)
    return rows


def child_headline(N):
    csi, m = headline_model(N)
    ts = []
    for _ in range(3):
        m.synchronize()
        t0 = time.perf_counter()
        csi.time_step(m, DT)
        m.synchronize()
        ts.append(time.perf_counter() - t0)
    print(json.dumps(dict(measure="headline", N=N, rk3_step=spread(ts), advances=advances(csi, m, N), writer=writer_records(csi, m, N))), flush=True)


def child_per_point(N):
    csi, m = per_point_model(N)
    print(json.dumps(dict(measure="per_point", N=N, advances=advances(csi, m, N))), flush=True)


def child_host(N):
    csi, m = headline_model(N)
    import drifters_ref as ref
    d = csi.Drifters.at_cell_centers(m.grid)
    xi, eta, _ = d.numpy()
    G = ref.RefGrid.of(m.grid)
    m.synchronize()
    t0 = time.perf_counter()
    u, v = m.velocities.u.numpy(), m.velocities.v.numpy()
    t1 = time.perf_counter()
    ref.advance(G, u, v, xi, eta, DT, 1)
    t2 = time.perf_counter()
    print(json.dumps(dict(measure="host", N=N, n=int(xi.size), download_ms=1e3 * (t1 - t0), numpy_ms=1e3 * (t2 - t1), total_ms=1e3 * (t2 - t0))), flush=True)


def markdown(records):
    lines = []
    for rec in records:
        if "advances" not in rec:
            continue
        step = rec.get("rk3_step")
        lines.append(f"\n**{rec['measure']}**, N = {rec['N']}" + (f"; RK3 step {step['median_ms']:.1f} ms (min {step['min_ms']:.1f}, max {step['max_ms']:.1f}, {step['reps']} repeats)"
                                                                 if step else "") + "\n")
        lines.append("| n | order | m | ms per advance (median, min – max of 5) | drifter-sub-steps / s |" + (" share of an RK3 step |" if step else ""))
        lines.append("|---|---|---|---|---|" + ("---|" if step else ""))
        for r in rec["advances"]:
            row = f"| {r['n_name']} = {r['n']} | {r['order']} | {r['substeps']} | {r['median_ms']:.3f} ({r['min_ms']:.3f} – {r['max_ms']:.3f}) | {r['drifter_substeps_per_s']:.3g} |"
            lines.append(row + (f" {100 * r['median_ms'] / step['median_ms']:.2f} % |" if step else ""))
    for rec in records:
        for r in rec.get("writer", []):
            lines.append(f"\n**writer record**, {r['n_name']} = {r['n']} drifters, five columns and the status ({r['bytes'] / 1e6:.2f} MB, copied synchronously): "
                         f"{r['median_ms']:.3f} ms per record (min {r['min_ms']:.3f}, max {r['max_ms']:.3f}, {r['reps']} repeats)")
    for rec in records:
        if rec["measure"] == "host":
            lines.append(f"\n**host route**, N = {rec['N']}, n = {rec['n']}, one sub-step: u.numpy() + v.numpy() {rec['download_ms']:.1f} ms, the NumPy restatement "
                         f"{rec['numpy_ms']:.0f} ms, together {rec['total_ms']:.0f} ms\n")
    return "\n".join(lines) + "\n"


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--child"]:
        {"headline": child_headline, "per_point": child_per_point, "host": child_host}[argv[1]](int(argv[2]))
        return 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    N = int(argv[argv.index("--N") + 1]) if "--N" in argv else 2048
    records = []
    for what in ("headline", "per_point", "host"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(N)], timeout=LIMITS[what], capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            print(f"drifters_profile: {what} ran into its time limit; stopping", flush=True)
            return 124
        if p.returncode != 0:
            print(p.stdout + p.stderr)
            print(f"drifters_profile: {what} failed with status {p.returncode}; stopping", flush=True)
            return p.returncode
        print(p.stdout, end="", flush=True)
        records.append(json.loads(p.stdout.strip().splitlines()[-1]))
    text = markdown(records)
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
