#!/usr/bin/env python3
"""Times the bare-ice thermodynamic step at 2048 x 2048 in three configurations, for a `rocprofv3 --kernel-trace --stats` run:

  numbers    top / bottom heat flux given as numbers, MeltingConstrainedFluxBalance -> k_slab (thermo.hip)
  arrays     per-cell top and bottom arrays                                        -> k_slab_flux<1,1,0,0>
  emission   (RadiativeEmission(), array) on top, array at the bottom               -> k_slab_flux<1,1,1,1> (secant per cell)

The state mixes open water, thin, consolidated and melting ice (tests/test_gpu_heat_fluxes.py mixed_state).  Each configuration
runs --warmup + --reps steps; the device time of the timed steps comes from HIP events around them.  Prints one JSON line per
configuration with the compulsory bytes per cell (h, aice read and written, the mass flux written, plus the arrays read, and Tu
read and written under emission).

  rocprofv3 --kernel-trace --stats -d OUT -- python scripts/heat_flux_profile.py [--n 2048] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

BYTES = {"numbers": 5 * 8, "arrays": 7 * 8, "emission": 9 * 8}     # compulsory bytes per cell and step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import climaseaice_jl_amd as csi
    from test_gpu_heat_fluxes import mixed_state

    n = a.n
    h, aice, _, qt, qb, *_ = mixed_state(n, n, 43)
    g = csi.RectilinearGrid((n, n), x=(0, 1), y=(0, 1), halo=(4, 4))
    for name, top, bottom in (("numbers", -60.0, 4.0), ("arrays", qt, qb), ("emission", (csi.RadiativeEmission(), qt - 200.0), qb)):
        ice = csi.SlabThermodynamics(bottom_salinity=30.0, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        m = csi.SeaIceModel(g, ice_thermodynamics=ice, timestepper="ForwardEuler", top_heat_flux=top, bottom_heat_flux=bottom)
        csi.set_(m, h=h, aice=aice)
        mf = csi.CenterField(g, m.device, "mass_flux")
        m._bind("MASS_FLUX", mf)
        sp = m._slab_params
        import ctypes as C
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
        # (torch's events bracket the library's stream from the outside: an upper bound; the kernel trace has the launch times)
        us = e0.elapsed_time(e1) * 1e3 / a.reps
        gbs = BYTES[name] * n * n / (us * 1e-6) / 1e9
        print(json.dumps(dict(config=name, n=n, reps=a.reps, us_per_step_upper_bound=round(us, 2), compulsory_bytes_per_cell=BYTES[name],
                              gb_per_s_at_that_time=round(gbs, 1))), flush=True)
        del m


if __name__ == "__main__":
    main()
