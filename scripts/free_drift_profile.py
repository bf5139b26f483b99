"""Measurements of the free-drift additions (profiles/r10_free_drift.md).  Run on the GPU box:

python scripts/free_drift_profile.py subcycle <1|2> [N] [reps]   OMIP-style N^2 EVP sub-cycle (120 sub-steps, FAST, arrays, 30 % land) with
                                                              free-drift kind 1 (StressBalanceFreeDrift) or kind 2 (prescribed fields fed
                                                              the SAME values: the free-drift dynamics step of this library computes them);
                                                              CSI_HIP_LIBRARY selects another build for kind 1
python scripts/free_drift_profile.py dynamics [N]             the free-drift dynamics launch (periodic, arrays for tau and u_e, v_e) and, for a
                                                              yardstick, a kind-1 sub-cycle (its k_free_drift launch) -- run it under
                                                              rocprofv3 --kernel-trace --stats; prints the compulsory bytes of the launch
python scripts/free_drift_profile.py rk3 [N] [reps]           whole RK3 step, WENO7: free-drift-dynamics model beside the advection-only model
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


def dynamics_model(c, **kw):
    """cases.csi_model's stresses as StressBalanceFreeDrift(top, bottom), the model's whole dynamics"""
    orig = csi.SeaIceMomentumEquation
    csi.SeaIceMomentumEquation = lambda g, **k: csi.StressBalanceFreeDrift(top_momentum_stress=k.get("top_momentum_stress"),
                                                                           bottom_momentum_stress=k.get("bottom_momentum_stress"))
    try:
        return cases.csi_model(c, **kw)
    finally:
        csi.SeaIceMomentumEquation = orig


def stress_balance_fields(c):
    m = dynamics_model(c, mode="fast")
    csi.time_step_momentum(m, c["dt"])
    m.synchronize()
    return m.velocities.u.interior_numpy().copy(), m.velocities.v.interior_numpy().copy()


def timed(fn, sync, reps):
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


what = sys.argv[1]
if what == "subcycle":
    kind, N, reps = int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 2048, int(sys.argv[4]) if len(sys.argv) > 4 else 5
    c = cases.make_case(Nx=N, Ny=N, substeps=120, patches=False, noise=0.05, topo=("periodic", "bounded"), land=0.3, field_forcing=True, free_drift=True)
    if kind == 2:
        Fu, Fv = stress_balance_fields(c)
        nyu, nxu = c["u"].shape
        nyv, nxv = c["v"].shape
        Fu_full, Fv_full = np.zeros((nyu, nxu)), np.zeros((nyv, nxv))       # (wall faces beyond row Ny: peripheral, never read as free drift)
        Fu_full[:Fu.shape[0], :Fu.shape[1]] = Fu
        Fv_full[:Fv.shape[0], :Fv.shape[1]] = Fv
        orig = csi.SeaIceMomentumEquation
        csi.SeaIceMomentumEquation = lambda g, **k: orig(g, **dict(k, free_drift=dict(u=Fu_full, v=Fv_full)))
    m = cases.csi_model(c, mode="fast")
    for _ in range(2):
        csi.time_step_momentum(m, c["dt"])
    ms = timed(lambda: csi.time_step_momentum(m, c["dt"]), m.synchronize, reps)
    dev = m.ctx.last_subcycle_ms()
    print(json.dumps(dict(what="omip_subcycle", kind=kind, N=N, library=os.environ.get("CSI_HIP_LIBRARY", "this build"), path=m.ctx.last_path()["level"],
                          wall_ms=[round(x, 3) for x in ms], median_ms=round(float(np.median(ms)), 3), last_device_ms=round(dev, 3),
                          gcell_substeps_per_s=round(N * N * 120 / np.median(ms) / 1e6, 2))))
elif what == "dynamics":
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    c = cases.make_case(Nx=N, Ny=N, substeps=2, patches=False, noise=0.05, topo=("periodic", "periodic"), field_forcing=True, free_drift=True)
    m = dynamics_model(c, mode="fast")
    for _ in range(3):
        csi.time_step_momentum(m, c["dt"])
    ms = timed(lambda: csi.time_step_momentum(m, c["dt"]), m.synchronize, 10)
    dev = []
    for _ in range(10):
        csi.time_step_momentum(m, c["dt"])
        m.synchronize()
        dev.append(m.ctx.last_subcycle_ms() * 1e3)
    k1 = cases.csi_model(c, mode="fast")          # the yardstick: k_free_drift of a kind-1 sub-cycle at the same size
    for _ in range(5):
        csi.time_step_momentum(k1, c["dt"])
    k1.synchronize()
    # compulsory bytes of the launch, from the shapes: tau_x, tau_y, u_e, v_e read once, u, v written once (interior points; the halo
    # images are a boundary term)
    nbytes = 8 * (4 + 2) * N * N
    print(json.dumps(dict(what="free_drift_dynamics_launch", N=N, event_us=[round(x, 1) for x in dev], median_event_us=round(float(np.median(dev)), 1),
                          wall_ms_per_call=round(float(np.median(ms)), 4), compulsory_bytes=nbytes,
                          bound_us_at_peak_hbm=round(nbytes / PEAK_HBM * 1e6, 1), launches=m.ctx.last_launches())))
elif what == "rk3":
    N, reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2048, int(sys.argv[3]) if len(sys.argv) > 3 else 10
    c = cases.make_case(Nx=N, Ny=N, patches=False, noise=0.05, topo=("periodic", "periodic"), field_forcing=True, free_drift=True)
    out = {}
    for name in ("free_drift_dynamics", "advection_only"):
        if name == "free_drift_dynamics":
            m = dynamics_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7))
        else:
            m = csi.SeaIceModel(c["g"], advection=csi.WENO(order=7), timestepper="SplitRungeKutta3", mode="fast")
            csi.set_(m, h=c["h"], aice=c["a"], u=c["u"], v=c["v"])
        for _ in range(3):
            csi.time_step(m, 10.0)
        m.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            csi.time_step(m, 10.0)
        m.synchronize()
        out[name + "_us_per_step"] = round((time.perf_counter() - t0) / reps * 1e6, 1)
    print(json.dumps(dict(what="rk3_weno7", N=N, **out)))
