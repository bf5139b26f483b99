"""What the momentum term fields and their power cost on the device, and what the same quantities cost through the host.  Needs the GPU.

    python scripts/momentum_terms_profile.py [sizes, default 2048,4096]     one child process per measurement, each under its own time
                                                                            limit; stops at the first failure
    python scripts/momentum_terms_profile.py --child kernels|host N         one measurement (also what to put behind `rocprofv3
                                                                            --kernel-trace --stats --` for the kernels' device times)

kernels  the benchmark's model (EVP, 120 sub-steps, WENO7, periodic uniform grid, a number on top, a SemiImplicitStress below) after one
         RK3 step.  Host clock around batches of 16 csi_momentum_terms_compute calls that end in a wait for the context's stream -- an
         upper bound of the kernel time, launch gaps included -- for two masks: all ten fields, and TOP + BOTTOM only (the coupler's
         call; the instantiation without sigma loads).  Compulsory bytes per cell: u, v, h, aice once (32 B), with the internal term
         sigma11, sigma22, sigma12 once (24 B), 8 B per field written; against 8 TB/s.  The whole call of csi_momentum_budget_compute
         (two launches, a 40-byte copy, the wait) for all groups (56 B per cell) and for the external group (32 B).
host     the same quantities the only way there was before: Field.numpy() of u, v, h, aice (and sigma), then a NumPy restatement of
         the terms for THIS configuration (uniform metrics, doubly periodic, no land, FPlane, a number on top, an ocean at rest below;
         the general restatement of tests/momentum_terms_ref.py walks the points in Python and is for checking only) and the ordered
         sums of tests/diagnostics_ref.py.  It uses no new entry point, so CSI_HIP_LIBRARY may point it at an older build.  One repeat.
         With a build that has the entry points the child also checks its fields against the device's, bit for bit.
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
TOP = (0.05, 0.02)
F0 = 1e-4


def make_model(N):
    import numpy as np
    import climaseaice_jl_amd as csi
    L = 2000.0 * N
    g = csi.RectilinearGrid((N, N), x=(0.0, L), y=(0.0, L), topology=(csi.Periodic, csi.Periodic), halo=(4, 4))
    dyn = csi.SeaIceMomentumEquation(g, coriolis=csi.FPlane(f=F0), rheology=csi.ElastoViscoPlasticRheology(), top_momentum_stress=TOP,
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


MASKS = {"all_ten": (("coriolis", "top", "bottom", "internal", "forcing"), 56 + 10 * 8), "top_bottom": (("top", "bottom"), 32 + 4 * 8)}


def child_kernels(N, batches=7, calls=16):
    csi, m = make_model(N)
    from climaseaice_jl_amd.momentum_terms import expand, mask_of
    cells = N * N
    out = dict(measure="kernels", N=N, cells=cells)
    for name, (terms, per) in MASKS.items():
        for f in expand(terms):
            m.momentum_term(f)
        mask = mask_of(terms)
        ts = []
        for b in range(batches + 2):
            m.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                m.ctx.momentum_terms_compute(mask)
            m.synchronize()
            if b >= 2:
                ts.append((time.perf_counter() - t0) / calls)
        r = spread(ts)
        r.update(bytes=per * cells, floor_ms=1e3 * per * cells / PEAK, share_of_8TBs=per * cells / PEAK / (1e-3 * r["median_ms"]))
        out[name] = r
    for what, per in (("all", 56), ("external", 32)):
        ts = []
        for b in range(batches + 2):
            m.synchronize()
            t0 = time.perf_counter()
            m.momentum_budget(what)
            if b >= 2:
                ts.append(time.perf_counter() - t0)
        r = spread(ts)
        r.update(bytes=per * cells, floor_ms=1e3 * per * cells / PEAK, share_of_8TBs=per * cells / PEAK / (1e-3 * r["median_ms"]))
        out["budget_" + what] = r
    b = m.momentum_budget()
    out["budget"] = {k: getattr(b, k) for k in ("coriolis", "top", "bottom", "internal", "forcing", "residual")}
    print(json.dumps(out), flush=True)


def host_terms(m, par, internal):
    """The term fields over i = 1 .. Nx, j = 1 .. Ny of the benchmark's configuration from the parents, in the documented order."""
    import numpy as np
    g = m.grid
    Nx, Ny, Hx, Hy = g.Nx, g.Ny, g.Hx, g.Hy
    met = g.metrics()
    dx, dy, rho = met["dx"], met["dy"], m.sea_ice_density
    at = lambda a, di=0, dj=0: a[Hy + dj:Hy + dj + Ny, Hx + di:Hx + di + Nx]
    avg4 = lambda a, pts: ((at(a, *pts[0]) + at(a, *pts[1])) / 2 + (at(a, *pts[2]) + at(a, *pts[3])) / 2) / 2
    u, v, h, a = par["u"], par["v"], par["h"], par["a"]
    mass = h * rho * a
    bot = m.dynamics.external_momentum_stresses.bottom
    C = bot.rho_e * bot.Cd
    out = {}
    for comp, own, other, (di, dj), pts, sign, tau in (("x", u, v, (-1, 0), ((-1, 0), (0, 0), (-1, 1), (0, 1)), -1.0, TOP[0]),
                                                       ("y", v, u, (0, -1), ((0, -1), (1, -1), (0, 0), (1, 0)), 1.0, TOP[1])):
        mi = (at(mass, di, dj) + at(mass)) / 2
        ai = (at(a, di, dj) + at(a)) / 2
        bar = avg4(other, pts)
        cross = (sign * F0) * bar                      # x_f_cross_U = -f v-bar, y_f_cross_U = f u-bar
        du, dv = 0.0 - at(own), 0.0 - bar
        tbot = C * np.sqrt(du * du + dv * dv) * du
        zero = mi <= 0
        out["coriolis_" + comp] = np.where(zero, 0.0, mi * (-cross))
        out["top_" + comp] = np.where(zero, 0.0, -(ai * tau))
        out["bottom_" + comp] = np.where(zero, 0.0, ai * tbot)
        out["forcing_" + comp] = np.zeros((Ny, Nx))
        if internal:
            s11, s22, s12 = par["s11"], par["s22"], par["s12"]
            sD = lambda i, j: at(s11, i, j) + at(s22, i, j)
            sT = lambda i, j: at(s11, i, j) - at(s22, i, j)
            if comp == "x":
                d = dy * (sD(0, 0) - sD(-1, 0)) / 2
                T = ((dy * dy) * sT(0, 0) - (dy * dy) * sT(-1, 0)) / dy / 2
                S = ((dx * dx) * at(s12, 0, 1) - (dx * dx) * at(s12)) / dx
            else:
                d = dx * (sD(0, 0) - sD(0, -1)) / 2
                T = -((dx * dx) * sT(0, 0) - (dx * dx) * sT(0, -1)) / dx / 2
                S = ((dy * dy) * at(s12, 1, 0) - (dy * dy) * at(s12)) / dy
            out["internal_" + comp] = np.where(zero, 0.0, (d + T + S) / (dx * dy))
    return out


def child_host(N):
    import numpy as np
    csi, m = make_model(N)
    import diagnostics_ref as dref
    f = m.dynamics.auxiliaries.fields
    fields = {"u": m.velocities.u, "v": m.velocities.v, "h": m.ice_thickness, "a": m.ice_concentration, "s11": f.s11, "s22": f.s22, "s12": f.s12}
    g = m.grid
    az = g.metrics()["dx"] * g.metrics()["dy"]
    inner = lambda a: a[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx]
    out = dict(measure="host", N=N, library=os.environ.get("CSI_HIP_LIBRARY", "default"))

    def budget(par, t):
        return {k: dref.ordered_sum((inner(par["u"]) * t[k + "_x"]) * az + (inner(par["v"]) * t[k + "_y"]) * az)
                for k in ("coriolis", "top", "bottom", "internal", "forcing")}
    last = None
    for name, need, internal, work in (("top_bottom", ("u", "v", "h", "a"), False, None), ("all_ten", tuple(fields), True, None),
                                       ("budget_all", tuple(fields), True, budget)):
        m.synchronize()
        t0 = time.perf_counter()
        par = {k: fields[k].numpy() for k in need}
        t1 = time.perf_counter()
        t = host_terms(m, par, internal)
        if work is not None:
            work(par, t)
        t2 = time.perf_counter()
        out[name] = dict(download_ms=1e3 * (t1 - t0), numpy_ms=1e3 * (t2 - t1), total_ms=1e3 * (t2 - t0))
        last = t
    if hasattr(m.ctx.L, "csi_momentum_terms_compute"):      # a build with the entry points: the host route gives the device's bits
        names = [n for n in last]
        dev = {n: m.momentum_term(n) for n in names}
        m.compute_momentum_terms("coriolis", "top", "bottom", "internal", "forcing")
        m.synchronize()
        out["equal_to_device"] = {n: bool(np.array_equal(dev[n].interior_numpy(), last[n])) for n in names}
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
                print(f"momentum_terms_profile: {what} at {N} ran into its time limit; stopping", flush=True)
                return 124
            if rc != 0:
                print(f"momentum_terms_profile: {what} at {N} failed with status {rc}; stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
