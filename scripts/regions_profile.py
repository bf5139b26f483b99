"""What the per-region integrals cost on the device, beside the plain tracer group and beside the host route.  Needs the GPU.

    python scripts/regions_profile.py [--out FILE.md] [--sizes 2048,4096]     one child process per grid size and route, each under its own
                                                                              time limit; stops at the first failure; the table of
                                                                              profiles/r29_regions.md goes to FILE.md (and to the
                                                                              standard output)
    python scripts/regions_profile.py --child device|host N                   one measurement, one JSON line

device   a model without dynamics on an N x N uniform periodic grid (h, aice bound; no snow, no mask): the wall time of a whole
         model.regional_diagnostics call (two launches, the copy of the folded slots, the wait) for three maps -- hemispheres (2 regions,
         split at row N / 2), 16 latitude bands of N / 16 rows, and a checkerboard of 8 x 8-cell squares that puts all 64 regions into
         every 64 x 64 tile (the longest region loop) -- and of model.diagnostics("tracers") on the same box.  Host clock around single
         calls, which end in a wait; median and spread of 30 calls after 5 warm-up calls.  Compulsory bytes: 8 (h) + 8 (aice) + 4 (id) per
         cell for the regions, 16 for the tracer group; the share of 8 TB/s they reach in the whole call.
host     what there was before: Field.interior_numpy() of h and aice (a stream drain and two whole-parent copies), Az, then one
         np.bincount per sum and a sort-free minimum / maximum per region (np.minimum.at); 3 repeats.  CSI_HIP_LIBRARY selects the build.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
LIMITS = {"device": 240, "host": 300}
PEAK = 8.0e12


def model_of(N):
    import numpy as np
    import climaseaice_jl_amd as csi
    L = 2000.0 * N
    g = csi.RectilinearGrid((N, N), x=(0.0, L), y=(0.0, L), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
    m = csi.SeaIceModel(g, dynamics=None, advection=None, timestepper="ForwardEuler")
    rng = np.random.default_rng(1)
    csi.set_(m, h=0.3 + 2.0 * rng.random((N, N)), aice=rng.random((N, N)))
    m.synchronize()
    return csi, m


def maps_of(N):
    import numpy as np
    j, i = np.mgrid[0:N, 0:N]
    return {"hemispheres (2)": ((j >= N // 2).astype(np.int32), 2), "16 bands": ((j // (N // 16)).astype(np.int32), 16),
            "64 in every tile": (((j // 8 % 8) * 8 + i // 8 % 8).astype(np.int32), 64)}


def spread(ts):
    ts = sorted(ts)
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1], reps=len(ts))


def timed(call, reps=30, warm=5):
    ts = []
    for k in range(reps + warm):
        t0 = time.perf_counter()
        call()
        if k >= warm:
            ts.append(time.perf_counter() - t0)
    return spread(ts)


def child_device(N):
    csi, m = model_of(N)
    rows = []
    r = timed(lambda: m.diagnostics("tracers"))
    r.update(what="tracer group", regions=0, bytes_per_cell=16)
    rows.append(r)
    for name, (ids, n) in maps_of(N).items():
        regions = csi.Regions(m.grid, ids, names=[str(k) for k in range(n)])
        got = m.regional_diagnostics(regions)
        assert int(got.cells.sum()) == N * N and got.unassigned_cells == 0
        r = timed(lambda: m.regional_diagnostics(regions))
        r.update(what=name, regions=n, bytes_per_cell=20, partial_bytes=csi._lib.regions_layout(N, N, n)[1])
        rows.append(r)
    for r in rows:
        r["share_of_peak"] = r["bytes_per_cell"] * N * N / (1e-3 * r["median_ms"]) / PEAK
    print(json.dumps(dict(measure="device", N=N, rows=rows)), flush=True)


def child_host(N):
    import numpy as np
    csi, m = model_of(N)
    ids, n = maps_of(N)["16 bands"]
    az = np.full((N, N), m.grid.dx * m.grid.dy)
    ts = {"download_ms": [], "numpy_ms": []}
    for _ in range(3):
        t0 = time.perf_counter()
        h, a = m.ice_thickness.interior_numpy(), m.ice_concentration.interior_numpy()
        t1 = time.perf_counter()
        flat = ids.ravel()
        out = [np.bincount(flat, weights=w.ravel(), minlength=n) for w in ((h * a) * az, a * az, np.where(a >= 0.15, az, 0.0), az)]
        lo, hi = np.full(n, np.inf), np.full(n, -np.inf)
        np.minimum.at(lo, flat, h.ravel())
        np.maximum.at(hi, flat, h.ravel())
        t2 = time.perf_counter()
        ts["download_ms"].append(1e3 * (t1 - t0))
        ts["numpy_ms"].append(1e3 * (t2 - t1))
    assert len(out) == 4 and np.isfinite(lo).all() and np.isfinite(hi).all()
    print(json.dumps(dict(measure="host", N=N, regions=n, library=os.environ.get("CSI_HIP_LIBRARY", "(this build)"),
                          download_ms=sorted(ts["download_ms"])[1], numpy_ms=sorted(ts["numpy_ms"])[1])), flush=True)


def markdown(records):
    lines = []
    for rec in records:
        if rec["measure"] == "device":
            N = rec["N"]
            base = rec["rows"][0]["median_ms"]
            lines.append(f"\n**device**, {N} x {N}\n")
            lines.append("| call | regions | ms per call (median, min – max of 30) | against the tracer group | compulsory B / cell | share of 8 TB/s | record buffer |")
            lines.append("|---|---|---|---|---|---|---|")
            for r in rec["rows"]:
                buf = f"{r['partial_bytes'] / 1e6:.2f} MB" if "partial_bytes" in r else "–"
                lines.append(f"| {r['what']} | {r['regions'] or '–'} | {r['median_ms']:.3f} ({r['min_ms']:.3f} – {r['max_ms']:.3f}) | {r['median_ms'] / base:.2f} x | "
                             f"{r['bytes_per_cell']} | {100 * r['share_of_peak']:.1f} % | {buf} |")
        else:
            lines.append(f"\n**host route**, {rec['N']} x {rec['N']}, {rec['regions']} regions, library {rec['library']}: interior_numpy of h and aice "
                         f"{rec['download_ms']:.0f} ms, bincount and extrema {rec['numpy_ms']:.0f} ms (median of 3)\n")
    return "\n".join(lines) + "\n"


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--child"]:
        {"device": child_device, "host": child_host}[argv[1]](int(argv[2]))
        return 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    sizes = [int(s) for s in (argv[argv.index("--sizes") + 1] if "--sizes" in argv else "2048,4096").split(",")]
    records = []
    for N in sizes:
        for what in ("device", "host"):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(N)], timeout=LIMITS[what], capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                print(f"regions_profile: {what} at {N} ran into its time limit; stopping", flush=True)
                return 124
            if p.returncode != 0:
                print(p.stdout + p.stderr)
                print(f"regions_profile: {what} at {N} failed with status {p.returncode}; stopping", flush=True)
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
