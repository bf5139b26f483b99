#!/usr/bin/env python3
"""Times the slab-ocean mixed layer (csrc/mixed_layer.hip) and the thermodynamic part of a step around it, for a plain run or a
`rocprofv3 --kernel-trace --stats` run (a trace goes in a run of its own):

  kernel_numbers   csi_mixed_layer_step alone, every input a number                     -> k_mixed_layer<0,0,0,0>, 32 B per cell
  kernel_arrays    the same with Fo, K, Ta, Qd and the bottom salinity per cell          -> k_mixed_layer<1,1,1,1>, 72 B per cell
  step_ocean       mixed layer + bare-ice step (the column path of time_step), numbers   -> k_mixed_layer + k_slab_flux<0,1,0,0>
  step_array       the bare-ice step alone with the bottom flux as an array             -> k_slab_flux<0,1,0,0>
  step_host_set    what the mixed layer replaces: a host Field.set of bottom_heat_flux before every bare-ice step
  numbers / arrays / emission   the three older thermodynamic configurations of scripts/heat_flux_profile.py; they run with an older
                   build of the library too (CSI_HIP_LIBRARY=... --configs numbers,arrays,emission), which is how the parent's times
                   are measured beside the new ones on one box

Compulsory bytes of the kernel: 32 B per cell (To and aice read, To' and Qb written) plus 8 per array that is read or written.  Each
configuration runs --warmup + --reps steps; the device time of the timed steps comes from HIP events around them (an upper bound:
the events bracket the library's stream from the outside).  One JSON line per configuration.

  python scripts/mixed_layer_profile.py [--n 2048] [--reps 50] [--warmup 5] [--configs a,b,...]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = ["kernel_numbers", "kernel_arrays", "step_ocean", "step_array", "step_host_set", "numbers", "arrays", "emission"]
KERNEL_BYTES = {"kernel_numbers": 32, "kernel_arrays": 32 + 5 * 8}
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    import numpy as np
    import torch
    import climaseaice_jl_amd as csi
    from test_gpu_heat_fluxes import mixed_state

    n = a.n
    h, aice, _, qt, qb, *_ = mixed_state(n, n, 43)
    rng = np.random.default_rng(45)
    Tf = -0.054 * 30.0
    To = Tf + 0.5 * rng.standard_normal((n, n))
    Fo, K, Ta = 100.0 * rng.standard_normal((n, n)), 5.0 + 20.0 * rng.random((n, n)), -25.0 + 30.0 * rng.random((n, n))
    Qd, S = 5.0 * rng.standard_normal((n, n)), 25.0 + 10.0 * rng.random((n, n))
    g = csi.RectilinearGrid((n, n), x=(0, 1), y=(0, 1), halo=(4, 4))
    for name in a.configs.split(","):
        ocean, top, bottom, salinity = None, -60.0, None, 30.0
        if name in ("kernel_numbers", "step_ocean"):
            ocean = csi.SlabOceanMixedLayer(30.0, temperature=To, surface_heat_flux=-20.0, coefficient=12.0, atmosphere_temperature=-15.0,
                                            deep_heat_flux=2.0)
        elif name == "kernel_arrays":
            ocean = csi.SlabOceanMixedLayer(30.0, temperature=To, surface_heat_flux=Fo, coefficient=K, atmosphere_temperature=Ta, deep_heat_flux=Qd)
            salinity = S
        elif name in ("step_array", "step_host_set"):
            bottom = qb
        elif name == "numbers":
            bottom = 4.0
        elif name == "arrays":
            top, bottom = qt, qb
        elif name == "emission":
            top, bottom = (csi.RadiativeEmission(), qt - 200.0), qb
        else:
            raise SystemExit(f"unknown configuration {name}")
        ice = csi.SlabThermodynamics(bottom_salinity=salinity, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        kw = dict(ocean=ocean) if ocean is not None else dict(bottom_heat_flux=bottom)
        m = csi.SeaIceModel(g, ice_thermodynamics=ice, timestepper="ForwardEuler", top_heat_flux=top, **kw)
        csi.set_(m, h=h, aice=aice)
        mf = csi.CenterField(g, m.device, "mass_flux")
        m._bind("MASS_FLUX", mf)
        sp = m._slab_params
        host = np.ascontiguousarray(qb)

        def step():
            if name.startswith("kernel"):
                m.ctx.mixed_layer_step(600.0, False)
                return
            if name == "step_ocean":
                m.ctx.mixed_layer_step(600.0, False)
            elif name == "step_host_set":      # the coupler's round trip: host array -> device field, then the step
                m.external_heat_fluxes.bottom.set(host)
                torch.cuda.synchronize()
            m.ctx.call("csi_slab_thermo_step", C.byref(sp), 600.0)

        for k in range(a.warmup):
            step()
        m.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.reps):
            step()
        m.synchronize()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.reps
        out = dict(config=name, n=n, reps=a.reps, library=os.path.basename(os.environ.get("CSI_HIP_LIBRARY", "libcsi_hip.so")),
                   us_per_step_upper_bound=round(us, 2))
        if name in KERNEL_BYTES:
            rate = KERNEL_BYTES[name] * n * n / (us * 1e-6)
            out.update(compulsory_bytes_per_cell=KERNEL_BYTES[name], tb_per_s_at_that_time=round(rate / 1e12, 2),
                       share_of_8_tb_per_s=round(rate / PEAK, 3))
        print(json.dumps(out), flush=True)
        del m


if __name__ == "__main__":
    main()
