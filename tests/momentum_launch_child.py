"""Child process of tests/test_gpu_momentum_variants.py::test_viscous_subcycle_launches_in_a_kernel_trace (run under
`rocprofv3 --kernel-trace`): builds a viscous split-explicit model and calls time_step_momentum! once.
  python tests/momentum_launch_child.py TOPO_X TOPO_Y SUBSTEPS"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE, os.path.join(os.path.dirname(HERE), "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases
import climaseaice_jl_amd as csi


def main():
    tx, ty, sub = sys.argv[1], sys.argv[2], int(sys.argv[3])
    c = cases.make_case(Nx=32, Ny=24, topo=(tx, ty), substeps=sub, random_uv=0.02)
    orig = csi.SeaIceMomentumEquation
    csi.SeaIceMomentumEquation = lambda g, **k: orig(g, **dict(k, rheology=csi.ViscousRheology(nu=1000.0)))
    try:
        m = cases.csi_model(c, mode="fast")
    finally:
        csi.SeaIceMomentumEquation = orig
    m.synchronize()
    csi.time_step_momentum(m, c["dt"])
    m.synchronize()
    print("launches", m.ctx.last_launches())


if __name__ == "__main__":
    main()
