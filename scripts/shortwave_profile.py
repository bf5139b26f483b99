#!/usr/bin/env python3
"""Times the bare-ice thermodynamic step under MeltingConstrainedFluxBalance with the SHORTWAVE top-flux term (csrc/thermo_flux.hip, the
SW_NUMBER / SW_CELL instantiations), for a plain run or a `rocprofv3 --kernel-trace --stats` run (a trace goes in a run of its own):

  sw_number      (ShortwaveRadiation(number), number, RadiativeEmission(1.02 sigma)), bottom a number  -> k_slab_flux<0,0,1,1,0,0,SW_NUMBER>
  sw_cell        the same with the shortwave flux per cell                                             -> k_slab_flux<0,0,1,1,0,0,SW_CELL>
  sw_everything  (emission, ShortwaveRadiation per cell, array), bottom array                          -> k_slab_flux<1,1,1,1,0,0,SW_CELL>
  numbers / arrays / emission   the three older configurations of scripts/heat_flux_profile.py; they run with an older build of the
                 library too (CSI_HIP_LIBRARY=... --configs numbers,arrays,emission), which is how the parent's times are measured
                 beside the new ones on one box

and on two states (--state):

  example   every cell a column of the Arctic-basin example in early summer -- 2-3.5 m of ice, Tu- a few degrees below the threshold,
            the June forcing -- so few cells sit at the jump and the secant ends after a handful of updates everywhere
  random    the draw of tests/thermo_shortwave_ref.py random_state -- h 0.05-4 m, shortwave 0-320 W m^-2, other fluxes 120-330 W m^-2,
            Tu- in -30...0 -- where lanes leave the secant after anything up to ~135 updates: what divergence costs

Every timed step starts from the same state: h, aice and Tu- are restored by device copies before it, outside the timed region, so
that the solve sees the same Tu- at every repetition.  Each repetition is timed on its own with a pair of HIP events recorded while
the device is idle -- restore, wait, event, step, wait for the library's stream, event -- and the times are averaged.  That is an
upper bound: a pair brackets one launch and one wait from the outside; `empty_us` is what a pair with no step between measures.
Compulsory bytes per cell: h, aice read and written, the mass flux written, Tu read and written (56), plus 8 per array read (the
shortwave flux, the top array, the bottom array).  One JSON line per configuration.

  python scripts/shortwave_profile.py [--n 2048] [--reps 30] [--warmup 3] [--state example|random] [--configs a,b,...]
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

CONFIGS = ["sw_number", "sw_cell", "sw_everything", "numbers", "arrays", "emission"]
BYTES = {"sw_number": 56, "sw_cell": 64, "sw_everything": 80, "numbers": 40, "arrays": 56, "emission": 72}
PEAK = 8e12
SIGMA = 5.67e-8 * 1.02


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--state", default="example")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    import numpy as np
    import torch
    import climaseaice_jl_amd as csi

    n = a.n
    rng = np.random.default_rng(3)
    if a.state == "random":
        h = rng.uniform(0.05, 4.0, (n, n))
        Tu0 = rng.uniform(-30, 0, (n, n))
        Fsw = -rng.uniform(0, 320, (n, n))
        Fin = -rng.uniform(120, 330, (n, n))
    else:
        h = rng.uniform(2.0, 3.5, (n, n))
        Tu0 = rng.uniform(-4.0, -0.5, (n, n))
        Fsw = -(200.0 + 30.0 * rng.random((n, n)))
        Fin = -(190.0 + 30.0 * rng.random((n, n)))
    aice = np.ones((n, n))
    qb = 2.0 + rng.random((n, n))
    g = csi.RectilinearGrid((n, n), x=(0, 1), y=(0, 1), halo=(4, 4))
    for name in a.configs.split(","):
        emission = csi.RadiativeEmission(1.0, SIGMA)
        if name == "sw_number":
            top, bottom = (csi.ShortwaveRadiation(float(Fsw.mean())), float(Fin.mean()), emission), 2.0
        elif name == "sw_cell":
            top, bottom = (csi.ShortwaveRadiation(Fsw), float(Fin.mean()), emission), 2.0
        elif name == "sw_everything":
            top, bottom = (emission, csi.ShortwaveRadiation(Fsw), Fin), qb
        elif name == "numbers":
            top, bottom = -60.0, 4.0
        elif name == "arrays":
            top, bottom = Fin + 250.0, qb
        elif name == "emission":
            top, bottom = (csi.RadiativeEmission(), Fin), qb
        else:
            raise SystemExit(f"unknown configuration {name}")
        ice = csi.SlabThermodynamics(bottom_salinity=30.0, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
        m = csi.SeaIceModel(g, ice_thermodynamics=ice, timestepper="ForwardEuler", top_heat_flux=top, bottom_heat_flux=bottom)
        csi.set_(m, h=h, aice=aice)
        tu = getattr(m.ice_thermodynamics, "top_surface_temperature", None)
        if tu is not None:
            tu.set(Tu0)
        mf = csi.CenterField(g, m.device, "mass_flux")
        m._bind("MASS_FLUX", mf)
        sp = m._slab_params
        fields = [m.ice_thickness, m.ice_concentration] + ([tu] if tu is not None else [])
        saved = [f.data.clone() for f in fields]

        def restore():
            for f, s in zip(fields, saved):
                f.data.copy_(s)
            torch.cuda.synchronize()

        def timed(step):
            total = 0.0
            for k in range(a.reps):
                restore()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if step:
                    m.ctx.call("csi_slab_thermo_step", C.byref(sp), 8 * 3600.0)
                m.synchronize()
                e1.record()
                torch.cuda.synchronize()
                total += e0.elapsed_time(e1) * 1e3
            return total / a.reps

        for k in range(a.warmup):
            restore()
            m.ctx.call("csi_slab_thermo_step", C.byref(sp), 8 * 3600.0)
            m.synchronize()
        empty_us = timed(False)
        us = timed(True)
        rate = BYTES[name] * n * n / (us * 1e-6)
        out = dict(config=name, state=a.state, n=n, reps=a.reps, library=os.path.basename(os.environ.get("CSI_HIP_LIBRARY", "libcsi_hip.so")),
                   us_per_step_upper_bound=round(us, 2), empty_us=round(empty_us, 2), compulsory_bytes_per_cell=BYTES[name],
                   share_of_8_tb_per_s=round(rate / PEAK, 3))
        if name.startswith("sw"):
            alpha = m.albedo_used
            m.ctx.call("csi_slab_thermo_step", C.byref(sp), 8 * 3600.0)
            m.synchronize()
            al = alpha.interior_numpy()
            out.update(cold_cells=int((al == 0.75).sum()), warm_cells=int((al == 0.64).sum()),
                       finite=bool(np.all(np.isfinite(m.ice_thickness.interior_numpy()))))
        print(json.dumps(out), flush=True)
        del m


if __name__ == "__main__":
    main()
