"""Measurements of the forcing time series (profiles/r13_time_series.md).  Run on the GPU box, one JSON line per call:

python scripts/time_series_profile.py launch [N] [reps]          the interpolation launch alone (DEVICE backend, two slices per series) with
                                                                 1, 4, 8 and 11 series-driven slots: microseconds per launch from a batch of
                                                                 `reps` updates behind one synchronisation, and its share of the compulsory
                                                                 24 B per point and slot at 8 TB/s
python scripts/time_series_profile.py step <host_set|device|host|none> [N] [steps]
                                                                 OMIP-style N^2 momentum step of profiles/r10_free_drift.md (120 sub-steps, FAST,
                                                                 30 % land) with SIX forcing arrays (stress, ocean velocities, prescribed
                                                                 free-drift fields):
                                                                   none      the arrays never change (the sub-cycle alone)
                                                                   host_set  a host Field.set of every array before each step: the only path of a
                                                                             build without time series (CSI_HIP_LIBRARY selects such a build)
                                                                   device    six series, all slices on the device
                                                                   host      six series in host memory, window = 3, a slice boundary every 10 steps
                                                                             (the steps that bring a new slice into the window are listed)
"""
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
LOC = {"U": (csi.Face, csi.Center), "V": (csi.Center, csi.Face)}


def launch(N, reps):
    import ctypes as C
    import torch
    g = csi.RectilinearGrid((N, N), x=(0.0, N * 1e3), y=(0.0, N * 1e3), topology=(csi.Periodic, csi.Bounded), halo=(4, 4))
    m = csi.SeaIceModel(g, dynamics=None, advection=None, timestepper="ForwardEuler")
    times = np.array([0.0, 1.0])
    keep, out, done = [], {}, 0
    for count in (1, 4, 8, 11):
        for slot in L.SERIES_SLOTS[done:count]:
            loc = LOC[slot[-1]] if slot[-2:] in ("_U", "_V") else (csi.Center, csi.Center)
            fld = csi.Field(loc, g, m.device, slot.lower())
            m._bind(slot, fld)
            nx, ny = g.interior_size(*loc)
            data = torch.rand((2, ny, nx), dtype=torch.float64, device=m.device)
            st = L.TimeSeries(2, L.TIME_LINEAR, L.SERIES_DEVICE, 0, 0.0, times.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(data.data_ptr()), nx, nx * ny)
            torch.cuda.synchronize()
            m.ctx.call("csi_time_series_set", L.F[slot], C.byref(st))
            keep += [fld, data, st]
        done = count
        for k in range(5):
            m.ctx.time_series_update(0.1 * k)
        m.synchronize()
        runs = []
        for _ in range(5):
            t0 = time.perf_counter()
            for k in range(reps):
                m.ctx.time_series_update(0.05 + 0.9 * k / reps)
            m.synchronize()
            runs.append((time.perf_counter() - t0) / reps * 1e6)
        nbytes = 24 * N * N * count
        us = float(np.median(runs))
        out[str(count)] = dict(us_per_launch=round(us, 1), runs_us=[round(x, 1) for x in runs], compulsory_bytes=nbytes,
                               bound_us_at_peak_hbm=round(nbytes / PEAK_HBM * 1e6, 1), share_of_bound=round(nbytes / PEAK_HBM * 1e6 / us, 3))
    print(json.dumps(dict(what="time_series_launch", N=N, reps=reps, slots=out)))


def step(mode, N, steps):
    c = cases.make_case(Nx=N, Ny=N, substeps=120, patches=False, noise=0.05, topo=("periodic", "bounded"), land=0.3, field_forcing=True)
    g, dt, nt = c["g"], c["dt"], 4
    times = np.arange(nt) * 10.0 * dt                      # a slice boundary every 10 steps
    base = dict(TOP_U=c["top_u"], TOP_V=c["top_v"], BOT_U=c["ue_f"], BOT_V=c["ve_f"], FREE_DRIFT_U=0.5 * c["ue_f"], FREE_DRIFT_V=0.5 * c["ve_f"])
    series = mode in ("device", "host")

    def value(slot):
        if not series:
            return base[slot]
        data = np.stack([base[slot] * (1.0 + 0.01 * n) for n in range(nt)])
        return csi.FieldTimeSeries(g, LOC[slot[-1]], times, data, time_indexing=csi.Cyclical(), backend=csi.InMemory(3) if mode == "host" else csi.InMemory())
    v = {k: value(k) for k in base}
    orig = csi.SeaIceMomentumEquation
    csi.SeaIceMomentumEquation = lambda g_, **k: orig(g_, **dict(k, top_momentum_stress=(v["TOP_U"], v["TOP_V"]),
                                                                 bottom_momentum_stress=csi.SemiImplicitStress(ue=v["BOT_U"], ve=v["BOT_V"]),
                                                                 free_drift=dict(u=v["FREE_DRIFT_U"], v=v["FREE_DRIFT_V"])))
    try:
        m = cases.csi_model(dict(c, field_forcing=False), mode="fast")
    finally:
        csi.SeaIceMomentumEquation = orig
    fields = dict(TOP_U=m.external_stress_field("TOP", "U"), TOP_V=m.external_stress_field("TOP", "V"), BOT_U=m.external_stress_field("BOT", "U"),
                  BOT_V=m.external_stress_field("BOT", "V"), FREE_DRIFT_U=m.free_drift_field("u"), FREE_DRIFT_V=m.free_drift_field("v"))

    def one(n):
        m.clock.time = n * dt
        if mode == "host_set":
            for slot, fld in fields.items():
                fld.set(base[slot])
        csi.time_step_momentum(m, dt)

    for n in range(3):
        one(n)
    m.synchronize()
    wall, dev, crossing = [], [], []
    uploads = (lambda: m.time_series_status("TOP_U")[1]) if mode == "host" else (lambda: 0)
    for n in range(3, 3 + steps):
        before = uploads()
        t0 = time.perf_counter()
        one(n)
        m.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(m.ctx.last_subcycle_ms())
        crossing.append(uploads() > before)              # the step brought a new slice into the window
    wall, crossing = np.array(wall), np.array(crossing, dtype=bool)
    out = dict(what="omip_step", mode=mode, N=N, steps=steps, library=os.environ.get("CSI_HIP_LIBRARY", "this build"), path=m.ctx.last_path()["level"],
               forcing_arrays=len(fields), bytes_per_array=int(fields["TOP_U"].data.numel() * 8),
               median_ms=round(float(np.median(wall)), 3), min_ms=round(float(wall.min()), 3), max_ms=round(float(wall.max()), 3),
               subcycle_device_ms_median=round(float(np.median(dev)), 3))
    if mode == "host":
        out.update(steps_with_upload=int(crossing.sum()), ms_with_upload=[round(float(x), 3) for x in wall[crossing]],
                   median_ms_without_upload=round(float(np.median(wall[~crossing])), 3), max_ms_without_upload=round(float(wall[~crossing].max()), 3),
                   uploads=m.time_series_status("TOP_U")[1])
    print(json.dumps(out))


if __name__ == "__main__":
    what = sys.argv[1]
    if what == "launch":
        launch(int(sys.argv[2]) if len(sys.argv) > 2 else 2048, int(sys.argv[3]) if len(sys.argv) > 3 else 50)
    elif what == "step":
        step(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 2048, int(sys.argv[4]) if len(sys.argv) > 4 else 30)
    else:
        sys.exit(__doc__)
