"""Measurements of forcing time series on a source grid of their own (profiles/r23_regrid.md).  Run on the GPU box, one JSON line per call:

python scripts/regrid_profile.py launch [N] [reps]     k_time_series_regrid alone (DEVICE backend) from a 640 x 320 periodic source onto N^2 points:
                                                       one scalar slot, and six slots of which two are the components of a pair; HIP-event pairs
                                                       around batches of `reps` updates; the share of the compulsory bytes -- the map plus the store,
                                                       32 B per scalar point, 48 B per point of a pair -- at 8 TB/s.  Beside it k_time_series with one
                                                       and six slots on the same box (24 B per point); with CSI_HIP_LIBRARY naming an older build only
                                                       that part runs.
python scripts/regrid_profile.py step <model_grid|source_grid> [N] [steps]
                                                       OMIP-style N^2 momentum step (120 sub-steps, FAST, 30 % land) with SIX HOST-backend series,
                                                       window 3, a slice boundary every 10 steps: slices on the model grid (the path a build without
                                                       regridding has; CSI_HIP_LIBRARY may name such a build) against slices on a 640 x 320 source
                                                       grid; the steps that bring a new slice into the window are listed, and the host memory per
                                                       series slice.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import cases
import climaseaice_jl_amd as csi

PEAK_HBM = 8.0e12      # bytes / s, MI355X HBM3E peak
L = csi._lib
FC, CF, CC = (csi.Face, csi.Center), (csi.Center, csi.Face), (csi.Center, csi.Center)
HAS_REGRID = hasattr(L.load(), "csi_regrid_stats")


def source_grid():
    return csi.SourceGrid(np.arange(640) * 0.5625, np.linspace(-90.0, 90.0, 320), periodic_x=True)


def timed(m, stream, reps, update):
    """Microseconds per update: five batches of `reps` updates, each between a pair of HIP events on the library's stream."""
    import torch
    for k in range(5):
        update(k, 5)
    m.synchronize()
    runs = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(reps):
            update(k, reps)
        e1.record(stream)
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) / reps * 1e3)
    return float(np.median(runs)), [round(x, 1) for x in runs]


def launch(N, reps):
    import torch
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    g = csi.LatitudeLongitudeGrid((N, N), longitude=(0.0, 360.0), latitude=(-80.0, 88.0), topology=(csi.Periodic, csi.Bounded), halo=(4, 4))
    times = np.array([0.0, 1.0])
    tp = times.ctypes.data_as(C.POINTER(C.c_double))
    out = dict(what="regrid_launch", N=N, reps=reps, library=os.environ.get("CSI_HIP_LIBRARY", "this build"))

    def model():
        return csi.SeaIceModel(g, dynamics=None, advection=None, timestepper="ForwardEuler", stream=stream.cuda_stream)

    def bind(m, slot, loc, keep):
        fld = csi.Field(loc, g, m.device, slot.lower())
        m._bind(slot, fld)
        keep.append(fld)
        return tuple(reversed(g.interior_size(*loc)))

    update = lambda m: (lambda k, n: m.ctx.time_series_update(0.05 + 0.9 * k / n))      # noqa: E731
    # k_time_series on the model grid: one and six slots
    for count, slots in ((1, ["SNOWFALL"]), (6, ["TOP_U", "TOP_V", "BOT_U", "BOT_V", "TOP_HEAT_FLUX", "SNOWFALL"])):
        m, keep = model(), []
        for slot in slots:
            ny, nx = bind(m, slot, FC if slot.endswith("_U") else CF if slot.endswith("_V") else CC, keep)
            data = torch.rand((2, ny, nx), dtype=torch.float64, device=m.device)
            st = L.TimeSeries(2, L.TIME_LINEAR, L.SERIES_DEVICE, 0, 0.0, tp, C.c_void_p(data.data_ptr()), nx, nx * ny)
            torch.cuda.synchronize()
            m.ctx.call("csi_time_series_set", L.F[slot], C.byref(st))
            keep += [data, st]
        us, runs = timed(m, stream, reps, update(m))
        nbytes = 24 * N * N * count
        out[f"model_grid_{count}"] = dict(us_per_launch=round(us, 1), runs_us=runs, compulsory_bytes=nbytes, share_of_bound=round(nbytes / PEAK_HBM * 1e6 / us, 3))
        del m, keep
    if HAS_REGRID:
        src = source_grid()
        sy, sx = src.shape
        for count, slots in ((1, [("SNOWFALL", None)]), (6, [("TOP_U", 0), ("TOP_V", 1), ("BOT_U", None), ("BOT_V", None), ("TOP_HEAT_FLUX", None), ("SNOWFALL", None)])):
            m, keep, maps, nbytes = model(), [], {}, 0
            for slot, comp in slots:
                loc = FC if slot.endswith("_U") else CF if slot.endswith("_V") else CC
                ny, nx = bind(m, slot, loc, keep)
                if (loc, comp is not None) not in maps:
                    X, Y = g.target_nodes(*loc)
                    px = np.array([L.regrid_plan_axis(src.x, True, 0.0, v) for v in X])
                    py = np.array([L.regrid_plan_axis(src.y, False, 0.0, v) for v in Y])
                    b = lambda a, axis: np.broadcast_to(a[None, :] if axis == 0 else a[:, None], (ny, nx))      # noqa: E731
                    rot = (np.full((ny, nx), np.cos(0.3)), np.full((ny, nx), np.sin(0.3))) if comp is not None else (None, None)
                    maps[(loc, comp is not None)] = m.ctx.regrid_map_create({FC: 0, CF: 1, CC: 2}[loc], b(px[:, 0], 0), b(px[:, 1], 0), b(py[:, 0], 1), b(py[:, 1], 1),
                                                                            b(px[:, 2], 0), b(py[:, 2], 1), src.shape, *rot)
                data = [torch.rand((2, sy, sx), dtype=torch.float64, device=m.device) for _ in range(2 if comp is not None else 1)]
                sts = [L.TimeSeries(2, L.TIME_LINEAR, L.SERIES_DEVICE, 0, 0.0, tp, C.c_void_p(d.data_ptr()), sx, sx * sy) for d in data]
                torch.cuda.synchronize()
                m.ctx.call("csi_time_series_set_regridded", L.F[slot], C.byref(sts[0]), maps[(loc, comp is not None)],
                           C.byref(sts[1]) if comp is not None else None, comp or 0)
                keep += data + sts
                nbytes += (48 if comp is not None else 32) * ny * nx
            us, runs = timed(m, stream, reps, update(m))
            assert m.ctx.regrid_stats()[0] == 5 + 5 * reps
            out[f"source_grid_{count}"] = dict(us_per_launch=round(us, 1), runs_us=runs, compulsory_bytes=nbytes, source_slice_bytes=8 * sx * sy,
                                               share_of_bound=round(nbytes / PEAK_HBM * 1e6 / us, 3))
            del m, keep
    print(json.dumps(out))


def step(mode, N, steps):
    c = cases.make_case(Nx=N, Ny=N, grid="latlon", substeps=120, patches=False, noise=0.05, topo=("periodic", "bounded"), land=0.3, field_forcing=True)
    g, dt, nt = c["g"], c["dt"], 4
    times = np.arange(nt) * 10.0 * dt                      # a slice boundary every 10 steps
    backend = csi.InMemory(3)
    if mode == "model_grid":
        base = dict(TOP_U=c["top_u"], TOP_V=c["top_v"], BOT_U=c["ue_f"], BOT_V=c["ve_f"], FREE_DRIFT_U=0.5 * c["ue_f"], FREE_DRIFT_V=0.5 * c["ve_f"])
        loc = {"U": FC, "V": CF}
        v = {k: csi.FieldTimeSeries(g, loc[k[-1]], times, np.stack([a * (1.0 + 0.01 * n) for n in range(nt)]), time_indexing=csi.Cyclical(), backend=backend)
             for k, a in base.items()}
        slice_bytes = int(v["TOP_U"].data[0].nbytes)
    else:
        src = csi.SourceGrid(np.arange(640) * (70.0 / 640) - 5.0, np.linspace(15.0, 75.0, 320))      # covers the case's 60 x 50 degrees
        lam, phi, n = np.deg2rad(src.x)[None, None, :], np.deg2rad(src.y)[None, :, None], np.arange(nt)[:, None, None]
        pair = lambda s: csi.RegriddedVectorTimeSeries(g, src, times, s * np.cos(6 * lam) * np.cos(3 * phi) * (1.0 + 0.01 * n),      # noqa: E731
                                                       s * np.sin(4 * lam) * np.sin(6 * phi) * (1.0 + 0.01 * n), time_indexing=csi.Cyclical(), backend=backend)
        tau, ocean, drift = pair(0.01), pair(0.05), pair(0.02)
        v = dict(TOP_U=tau.x, TOP_V=tau.y, BOT_U=ocean.x, BOT_V=ocean.y, FREE_DRIFT_U=drift.x, FREE_DRIFT_V=drift.y)
        slice_bytes = int(tau.east[0].nbytes)
    orig = csi.SeaIceMomentumEquation
    csi.SeaIceMomentumEquation = lambda g_, **k: orig(g_, **dict(k, top_momentum_stress=(v["TOP_U"], v["TOP_V"]),
                                                                 bottom_momentum_stress=csi.SemiImplicitStress(ue=v["BOT_U"], ve=v["BOT_V"]),
                                                                 free_drift=dict(u=v["FREE_DRIFT_U"], v=v["FREE_DRIFT_V"])))
    try:
        m = cases.csi_model(dict(c, field_forcing=False), mode="fast")
    finally:
        csi.SeaIceMomentumEquation = orig
    for n in range(3):
        m.clock.time = n * dt
        csi.time_step_momentum(m, dt)
    m.synchronize()
    wall, crossing = [], []
    for n in range(3, 3 + steps):
        before = m.time_series_status("TOP_U")[1]
        m.clock.time = n * dt
        t0 = time.perf_counter()
        csi.time_step_momentum(m, dt)
        m.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        crossing.append(m.time_series_status("TOP_U")[1] > before)              # the step brought a new slice into the window
    wall, crossing = np.array(wall), np.array(crossing, dtype=bool)
    print(json.dumps(dict(what="omip_step_host_series", mode=mode, N=N, steps=steps, library=os.environ.get("CSI_HIP_LIBRARY", "this build"),
                          path=m.ctx.last_path()["level"], series=len(v), host_bytes_per_slice=slice_bytes,
                          median_ms=round(float(np.median(wall)), 3), min_ms=round(float(wall.min()), 3), max_ms=round(float(wall.max()), 3),
                          steps_with_upload=int(crossing.sum()), ms_with_upload=[round(float(x), 3) for x in wall[crossing]],
                          median_ms_without_upload=round(float(np.median(wall[~crossing])), 3), uploads=m.time_series_status("TOP_U")[1])))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "launch":
        launch(int(sys.argv[2]) if len(sys.argv) > 2 else 2048, int(sys.argv[3]) if len(sys.argv) > 3 else 50)
    elif what == "step":
        step(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 2048, int(sys.argv[4]) if len(sys.argv) > 4 else 30)
    else:
        sys.exit(__doc__)
