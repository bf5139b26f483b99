#!/usr/bin/env python3
"""Times the bare-ice thermodynamic step under MeltingConstrainedFluxBalance in seven configurations, for a plain run or a
`rocprofv3 --kernel-trace --stats` run:

  numbers        top / bottom heat flux given as numbers                               -> k_slab (thermo.hip)
  arrays         per-cell top and bottom arrays                                        -> k_slab_flux<1,1,0,0>
  emission       (RadiativeEmission(), array) on top, array at the bottom               -> k_slab_flux<1,1,1,1> (secant per cell)
  linear         LinearHeatFlux(K, Ta) with numbers on top, a number at the bottom      -> k_slab_flux<0,0,0,1,1,0> (secant per cell)
  linear_arrays  LinearHeatFlux with K and Ta per cell                                  -> k_slab_flux<0,0,0,1,2,0>
  everything     (RadiativeEmission(), LinearHeatFlux per cell, array), bottom array, per-cell bottom salinity -> k_slab_flux<1,1,1,1,2,1>
  used           the numbers configuration with both used-flux outputs bound            -> k_slab_flux<0,0,0,0>

The first three are the configurations of scripts/heat_flux_profile.py and run with an older build of the library too
(CSI_HIP_LIBRARY=... --configs numbers,arrays,emission): that is how the parent's times are measured beside the new ones on one
box.  The state mixes open water, thin, consolidated and melting ice (tests/test_gpu_heat_fluxes.py mixed_state).  Each
configuration runs --warmup + --reps steps; the device time of the timed steps comes from HIP events around them (an upper bound:
the events bracket the library's stream from the outside).  Prints one JSON line per configuration with the compulsory bytes per
cell -- h, aice read and written, the mass flux written, plus the arrays read, Tu read and written under a secant solve, the used
fluxes written -- and the share of 8 TB/s those bytes reach at the measured time.

  python scripts/thermo_linear_profile.py [--n 2048] [--reps 50] [--warmup 5] [--configs a,b,...]
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

# compulsory bytes per cell and step
BYTES = {"numbers": 5 * 8, "arrays": 7 * 8, "emission": 9 * 8, "linear": 7 * 8, "linear_arrays": 9 * 8, "everything": 12 * 8, "used": 7 * 8}
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default=",".join(BYTES))
    a = ap.parse_args()
    import numpy as np
    import torch
    import climaseaice_jl_amd as csi
    from test_gpu_heat_fluxes import mixed_state

    n = a.n
    h, aice, _, qt, qb, *_ = mixed_state(n, n, 43)
    rng = np.random.default_rng(44)
    K, Ta, S = 5.0 + 20.0 * rng.random((n, n)), -25.0 + 30.0 * rng.random((n, n)), 25.0 + 10.0 * rng.random((n, n))
    g = csi.RectilinearGrid((n, n), x=(0, 1), y=(0, 1), halo=(4, 4))
    for name in a.configs.split(","):
        top, bottom, salinity = {
            "numbers": lambda: (-60.0, 4.0, 30.0),
            "arrays": lambda: (qt, qb, 30.0),
            "emission": lambda: ((csi.RadiativeEmission(), qt - 200.0), qb, 30.0),
            "linear": lambda: (csi.LinearHeatFlux(15.0, -10.0), 4.0, 30.0),
            "linear_arrays": lambda: (csi.LinearHeatFlux(K, Ta), 4.0, 30.0),
            "everything": lambda: ((csi.RadiativeEmission(), csi.LinearHeatFlux(K, Ta), qt - 200.0), qb, S),
            "used": lambda: (-60.0, 4.0, 30.0)}[name]()
        ice = csi.SlabThermodynamics(bottom_salinity=salinity, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        m = csi.SeaIceModel(g, ice_thermodynamics=ice, timestepper="ForwardEuler", top_heat_flux=top, bottom_heat_flux=bottom)
        if name == "used":
            m.heat_fluxes_used
        csi.set_(m, h=h, aice=aice)
        mf = csi.CenterField(g, m.device, "mass_flux")
        m._bind("MASS_FLUX", mf)
        sp = m._slab_params
        for k in range(a.warmup):
            m.ctx.call("csi_slab_thermo_step", C.byref(sp), 600.0)
        m.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.reps):
            m.ctx.call("csi_slab_thermo_step", C.byref(sp), 600.0)
        m.synchronize()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.reps
        rate = BYTES[name] * n * n / (us * 1e-6)
        print(json.dumps(dict(config=name, n=n, reps=a.reps, library=os.path.basename(os.environ.get("CSI_HIP_LIBRARY", "libcsi_hip.so")),
                              us_per_step_upper_bound=round(us, 2), compulsory_bytes_per_cell=BYTES[name],
                              tb_per_s_at_that_time=round(rate / 1e12, 2), share_of_8_tb_per_s=round(rate / PEAK, 3))), flush=True)
        del m


if __name__ == "__main__":
    main()
