"""Time per call of the device diagnostics (csi_diagnostics_compute) against the two ways there were before: Field.numpy() + NumPy, and
torch reductions on the device.  Needs the GPU.

    python scripts/diagnostics_profile.py [sizes, default 2048,4096] [--no-library]

Steady state: every way is warmed up, then timed with a host clock around calls that end in a device synchronise (the library's call
waits for its stream itself).  Compulsory bytes: 16 B per cell for the velocity group (u, v); all groups add h, aice, hs (24 B) and the
mask byte; uniform metrics (no planes).  --no-library: only the two older ways (for a library built before the entry point existed,
selected with CSI_HIP_LIBRARY).  Prints one JSON line per size."""
import json
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np
import torch

import climaseaice_jl_amd as csi

PEAK = 8.0e12      # B/s, HBM (MI355X)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return dict(median_ms=1e3 * ts[len(ts) // 2], min_ms=1e3 * ts[0], max_ms=1e3 * ts[-1], reps=reps)


def main():
    sizes = [int(s) for s in (sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "2048,4096").split(",")]
    library = "--no-library" not in sys.argv
    for N in sizes:
        L = 2000.0 * N
        g = csi.RectilinearGrid((N, N), x=(0.0, L), y=(0.0, L), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
        m = csi.SeaIceModel(g, dynamics=None, advection=None, timestepper="ForwardEuler", ice_thermodynamics=csi.SlabThermodynamics(),
                            snow_thermodynamics=csi.snow_slab_thermodynamics())
        rng = np.random.default_rng(1)
        mask = rng.random((N, N)) > 0.1
        m.set_mask(mask)
        csi.set_(m, h=0.3 + rng.random((N, N)), aice=rng.random((N, N)), u=0.1 * rng.standard_normal((N, N)), v=0.1 * rng.standard_normal((N, N)),
                 hs=0.1 * rng.random((N, N)))
        out = dict(N=N, cells=N * N, library=os.environ.get("CSI_HIP_LIBRARY", "default"))
        cells = N * N
        if library:
            for name, what, nbytes in (("velocity", 1, 16 * cells), ("all", 3, 41 * cells)):
                r = timed(lambda: m.ctx.diagnostics_compute(what, 0.15), 200, warm=10)
                r.update(compulsory_bytes=nbytes, floor_ms=1e3 * nbytes / PEAK, share_of_8TBs=nbytes / PEAK / (1e-3 * r["median_ms"]))
                out["device_" + name] = r
        H = g.Hx
        dx, dy = g.dx, g.dy
        fu, fv, fh, fa, fs = m.velocities.u, m.velocities.v, m.ice_thickness, m.ice_concentration, m.snow_thickness
        act = mask

        def numpy_velocity():
            m.synchronize()
            u, v = fu.numpy()[H:-H, H:-H], fv.numpy()[H:-H, H:-H]
            inv = (np.abs(u) / dx + np.abs(v) / dy).max()
            return 1.0 / inv, np.abs(u).max(), np.abs(v).max(), np.isfinite(u).all(), np.isfinite(v).all()

        def numpy_all():
            r = numpy_velocity()
            h, a, s = (f.numpy()[H:-H, H:-H] for f in (fh, fa, fs))
            az = dx * dy
            return r, (h * a * az)[act].sum(), (a * az)[act].sum(), az * np.count_nonzero(act & (a >= 0.15)), (s * a * az)[act].sum(), \
                h[act].min(), h[act].max(), a[act].min(), a[act].max(), s[act].max(), np.isfinite(h).all(), np.isfinite(a).all(), np.isfinite(s).all()

        tmask = torch.from_numpy(mask).to(m.device)

        def torch_velocity():
            m.synchronize()
            u, v = fu.data[H:-H, H:-H], fv.data[H:-H, H:-H]
            inv = (u.abs() / dx + v.abs() / dy).max()
            return (1.0 / inv).item(), u.abs().max().item(), v.abs().max().item(), torch.isfinite(u).all().item(), torch.isfinite(v).all().item()

        def torch_all():
            r = torch_velocity()
            h, a, s = (f.data[H:-H, H:-H] for f in (fh, fa, fs))
            az = dx * dy
            z = torch.zeros((), dtype=torch.float64, device=m.device)
            big = torch.full((), float("inf"), dtype=torch.float64, device=m.device)
            vals = [torch.where(tmask, h * a * az, z).sum(), torch.where(tmask, a * az, z).sum(), (tmask & (a >= 0.15)).sum() * az,
                    torch.where(tmask, s * a * az, z).sum(), torch.where(tmask, h, big).min(), torch.where(tmask, h, -big).max(),
                    torch.where(tmask, a, big).min(), torch.where(tmask, a, -big).max(), torch.where(tmask, s, -big).max(),
                    torch.isfinite(h).all(), torch.isfinite(a).all(), torch.isfinite(s).all()]
            return r, [x.item() for x in vals]

        out["numpy_velocity"] = timed(numpy_velocity, 5, warm=1)
        out["numpy_all"] = timed(numpy_all, 5, warm=1)
        out["torch_velocity"] = timed(torch_velocity, 50, warm=5)
        out["torch_all"] = timed(torch_all, 50, warm=5)
        print(json.dumps(out), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
